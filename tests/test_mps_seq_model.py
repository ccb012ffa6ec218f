"""CPU: the call sequences of tests/mps_seq_model.py on the NumPy backend.

The dry run holds every committed sequence (and every statement's dense vector to plain dense arithmetic at exact steps); the
conditions of the truncating steps, the coverage of the alphabet and the five planted faults are asserted here, so that the GPU test
(tests/test_hip_mps_call_sequences.py) runs sequences that are known to be sound and a harness that is known to catch what it is for."""
import collections

import pytest

from tests import mps_seq_model as sm


@pytest.fixture(scope="module")
def dry():
    """Every committed sequence once on the good backend, with the dense checks on."""
    return {key: sm.run_sequence(sm.NumpyBackend(), *key, min_gap=sm.DRY_GAP, dense_checks=True) for key in sm.SEQUENCES}


def test_the_committed_list():
    counts = collections.Counter(register for register, _ in sm.SEQUENCES)
    assert counts == {"n7": 8, "n2": 2, "n1": 1, "n16": 1} and len(set(sm.SEQUENCES)) == len(sm.SEQUENCES)


@pytest.mark.parametrize("key", sm.SEQUENCES, ids=lambda k: f"{k[0]}-{k[1]}")
def test_dry_run(dry, key):
    """The runner on the NumPy backend passes the sequence; the generator is deterministic; a sequence is 12 to 30 steps (4 to 6 at n = 16)."""
    runner, steps = dry[key], sm.generate(*key)
    print(f"{key}: {len(steps)} steps; " + sm.report(runner))
    low, high = (4, 6) if key[0] == "n16" else (12, 30)
    assert low <= len(steps) <= high and len(steps) == sm.LENGTH[key[0]] and sum(runner.counts.values()) == len(steps)
    again = sm.Generator(*key).run(sm.LENGTH[key[0]])
    assert [s["kind"] for s in again] == [s["kind"] for s in steps]
    assert all(sm.flat_step(a) == sm.flat_step(b) for a, b in zip(again, steps))


def test_truncating_decisions_keep_their_distance(dry):
    """Every truncating decision outside a degenerate cluster has a relative gap of 10 x MIN_GAP in the dry run (the runner asserts it
    step by step, with ``mps_trunc_ref.check_margins``); here: that such decisions were made at all, and the smallest gap met."""
    from tests.test_mps_compress_ref import MIN_GAP

    assert sm.MIN_GAP == MIN_GAP and sm.DRY_GAP == 10 * MIN_GAP
    gaps = {key: r.smallest_gap for key, r in dry.items()}
    print("smallest relative gap per sequence:", {f"{k[0]}-{k[1]}": f"{g:.3g}" for k, g in gaps.items()})
    assert min(gaps.values()) >= sm.DRY_GAP
    assert sum(g < float("inf") for g in gaps.values()) >= 6


def test_the_alphabet_is_covered(dry):
    """Every step kind, every variant, every editor-then-holder pair, a repeated slot and a mixed-route batch for each batched entry point;
    for every reader with two routes: method None, the forced method of a slot's own route, the other route, a slot listed twice."""
    counts, tags = collections.Counter(), set()
    for runner in dry.values():
        counts.update(runner.counts)
        tags |= runner.tags
    print("steps per kind:", dict(sorted(counts.items())))
    assert [k for k in sm.KINDS if not counts[k]] == []
    assert [v for v in sm.VARIANTS if v not in tags] == []
    assert {"structured:ghz", "structured:bell", "structured:w"} <= tags
    for register, kinds in (("n1", sm.N1_KINDS), ("n16", sm.N16_KINDS)):   # the model knows what a register does not admit
        used = collections.Counter()
        for key, runner in dry.items():
            if key[0] == register:
                used.update(runner.counts)
        assert set(used) <= set(kinds)
    assert any("from_vectors:fused" in r.tags for k, r in dry.items() if k[0] == "n16")
    for key in sm.APPLY_SWITCH_SEQUENCES:   # what the GPU test runs under both values of AQC_MPS_APPLY leaves a method to it
        assert key in sm.SEQUENCES and {"v_mul_mps:None", "v_dagger_mul_mps:None"} & dry[key].tags


@pytest.mark.parametrize("name", sm.REGRESSIONS)
def test_regression_cases_pass_the_dry_run(name):
    register, steps = sm.regression(name)
    sm.run_steps(sm.NumpyBackend(), register, steps, min_gap=sm.DRY_GAP)


FAULTS = {
    "no_bump": "an in-place editor that does not bump version",
    "alias": "a maker whose output shares its arrays with an input",
    "weight": "compress reports this call's dropped weight without the input's",
    "lane0": "a batched maker returns lane 0's result for a slot listed twice at lane 2",
    "leak": "a close that leaves one buffer behind",
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_faults_are_caught(fault):
    """A backend that differs from the good one in one line fails at least one committed sequence, and the message names the step."""
    caught = []
    for key in sm.SEQUENCES:
        try:
            sm.run_sequence(sm.NumpyBackend(fault), *key, min_gap=sm.DRY_GAP)
        except sm.Failure as err:
            assert sm.STEP_IN_MESSAGE.search(str(err)), str(err)
            caught.append((key, str(err)))
            break
    print(f"{fault} ({FAULTS[fault]}): first caught in {caught[0][0] if caught else None}: {caught[0][1] if caught else None}")
    assert caught
