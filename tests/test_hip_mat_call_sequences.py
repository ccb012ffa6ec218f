"""GPU: call sequences on one long-lived MATRIX workspace (ncols > 1), checked against the shadow model of tests/ws_model_mat.py.

The long-running entry points of the matrix workspace (aqc_ws_lbfgs_mat, aqc_ws_cd_sweep / _sweeps / _minimize,
aqc_ws_sketch_generate / _adam) leave thetas in use and buffers behind them; include/aqc_hip.h says which, per call, and the
model encodes those sentences.  The tests interleave them with the data and compute calls the way the function-level front doors
do on their one cached workspace per ansatz, compare every read with the oracle (1e-10), every long-running call's outputs with
its reference at the bounds of that call's own tests, and, read for read, across kernel families and switches (1e-12).
"""
import numpy as np
import pytest

from tests import ws_model as wm
from tests import ws_model_mat as mm
from tests.ws_model import BUF_X, BUF_Y

pytestmark = pytest.mark.gpu

# every switch these tests set: unset unless a configuration says otherwise, whatever the caller's environment holds
SWITCHES = ("AQC_KERNEL_FAMILY", "AQC_MIRROR_PLAN", "AQC_GRADS_DIRECT", "AQC_R_ONLY_LAST", "AQC_R_ONLY_MAX_SUBS", "AQC_UBUILD_MIRROR", "AQC_GRAPH",
            "AQC_THREADS", "AQC_SWEEP_REG_BITS", "AQC_LAZY_Z", "AQC_LOW_BITS", "AQC_CD_CHAIN", "AQC_KERNEL_V2", "AQC_TILE_BITS_APPLY",
            "AQC_TILE_BITS_SWEEP", "AQC_APPLY_PERSIST", "AQC_SPARSE_SWEEP", "AQC_SPARSE_MIN_ITEMS")
FAMILIES = {"per-group": {"AQC_KERNEL_FAMILY": "1"}, "register-blocked": {"AQC_KERNEL_FAMILY": "2"}}
# Switches of include/aqc_switches.def whose reader lies on a path a matrix sequence runs: V, V^H, the dense sweep and its gradient
# walk, the U builder, the one-call evaluation's graph, aqc_ws_cd_sweep's route, and -- with their kernel family -- the workgroup size
# of the per-group kernels and the register bits of the register-blocked sweep.  Off the path: the sparse and projected routes
# (AQC_SPARSE_*, AQC_PROJECTED*, AQC_SKIP_ZERO_W, AQC_UBUILD_SUBSET) need a basis state as lhs, which no matrix sequence sets;
# AQC_APPLY_PERSIST and AQC_SWEEP_GRID act on 2^12 tiles, which no shape here has; the tile switches lose to the tile arguments.
ON_PATH = {"own_vdag_plan": {"AQC_MIRROR_PLAN": "0"}, "partial_sums": {"AQC_GRADS_DIRECT": "0"}, "full_last_substage": {"AQC_R_ONLY_LAST": "0"},
           "no_r_only_by_size": {"AQC_R_ONLY_MAX_SUBS": "0"}, "own_ubuild_jobs": {"AQC_UBUILD_MIRROR": "0"}, "no_graph": {"AQC_GRAPH": "0"},
           "eager_z": {"AQC_LAZY_Z": "0"}, "low_bits_2": {"AQC_LOW_BITS": "2"}, "cd_chain": {"AQC_CD_CHAIN": "1"},
           "threads_128": {"AQC_KERNEL_FAMILY": "1", "AQC_THREADS": "128"}, "reg_bits_3": {"AQC_KERNEL_FAMILY": "2", "AQC_SWEEP_REG_BITS": "3"}}
_CACHE = {}


def _shape(name):
    if name not in _CACHE:
        from aqc_research_amd.engine import HipContext

        make, ncols, tile, lanes, fits, kind, seeds = mm.SHAPES[name]
        circ = make()
        _CACHE[name] = (circ, HipContext(circ), ncols, tile, lanes, fits, mm.MatOracle(circ))
    return _CACHE[name]


def _configure(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _maker(name):
    from aqc_research_amd.engine import Workspace

    _, ctx, ncols, tile, lanes = _shape(name)[:5]
    return lambda: Workspace(ctx, batch=lanes, ncols=ncols, tile_bits_apply=tile, tile_bits_sweep=tile)


def _run(monkeypatch, name, env, ops):
    circ, _, ncols, _, lanes, _, oracle = _shape(name)
    _configure(monkeypatch, env)
    return wm.run_sequence(_maker(name), circ, lanes, ops, oracle, kit=mm.MatKit(ncols), residuals=True)


def _cross_check(results):
    """The same sequence must read the same numbers under every configuration.  A long-running call returns its point with the
    last-bit differences between kernel families amplified (L-BFGS: 2e-10 after two iterations), and every later read depends
    on that point; so what is compared is each read's deviation from the model value computed from the point that configuration
    returned.  The calls' own outputs are held to their references in run_sequence."""
    first = next(iter(results))
    worst = (0.0, None)
    for cfg, reads in results.items():
        assert [(s, label) for s, label, _ in reads] == [(s, label) for s, label, _ in results[first]], f"{cfg} made other reads than {first}"
        for (step, label, got), (_, _, ref) in zip(reads, results[first]):
            d = wm.maxdiff(got, ref)
            if d > worst[0]:
                worst = (d, f"step {step} {label}: {first} vs {cfg}")
    print(f"configurations agree to {worst[0]:.3g} ({worst[1]})")
    assert worst[0] < 1e-12, f"configurations disagree by {worst[0]:.3g} at {worst[1]}"


# ---- the shapes are what the table says ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["default", "per-group"])
@pytest.mark.parametrize("name", ["sq6", "sq7", "sk7", "rect7"])
def test_table_shapes_run_two_stages_with_a_checkpoint(monkeypatch, name, family):
    """Two stages everywhere but sq6 on the matrix cores, whose smallest tile holds its six qubits; the workspace runs the plan
    the host-only planner names."""
    from aqc_research_amd import _lib

    _configure(monkeypatch, FAMILIES.get(family, {}))
    _, ctx, ncols, tile, _, fits, _ = _shape(name)
    ws = _maker(name)()
    try:
        stages = [ws.plan_info(which)[0] for which in (0, 1, 2)]
        print(name, family, "stages of V^H, the sweep, V:", stages, "tile bits", ws.plan_info(1)[1], "family", ws.kernel_family(1))
        assert stages == ([1, 1, 1] if name == "sq6" and family == "default" else [2, 2, 2])
        assert stages == mm.planned_stages(ctx, ncols, ws.plan_info(1)[1])
        if ncols == 1 << _shape(name)[0].num_qubits:
            assert bool(_lib.lib().aqc_ws_cd_fits_one_launch(ws.handle)) == fits
    finally:
        ws.close()


# ---- random sequences ------------------------------------------------------------------------------------------------------------

CASES = [(name, seed) for name, shape in mm.SHAPES.items() for seed in shape[6]]


@pytest.mark.parametrize("name,seed", CASES)
def test_random_sequence_matches_the_model_on_every_kernel_family(monkeypatch, name, seed):
    ops = mm.sequence(name, seed, _shape(name)[0])
    results = {"default": _run(monkeypatch, name, {}, ops)}
    for family, env in FAMILIES.items():
        results[family] = _run(monkeypatch, name, env, ops)
    _cross_check(results)


# every sequence under every switch (AQC_CD_CHAIN is read by aqc_ws_cd_sweep alone, which takes a one-lane workspace: sq6_1's sequences)
SWITCH_CASES = [(name, seed, switch) for switch in sorted(ON_PATH) for name, seed in CASES if (switch != "cd_chain" or name == "sq6_1")]


@pytest.mark.parametrize("name,seed,switch", SWITCH_CASES)
def test_random_sequence_matches_the_model_under_every_switch_on_its_path(monkeypatch, name, seed, switch):
    ops = mm.sequence(name, seed, _shape(name)[0])
    _cross_check({"default": _run(monkeypatch, name, {}, ops), switch: _run(monkeypatch, name, ON_PATH[switch], ops)})


# ---- directed sequences: one per finding (tests/ws_model_mat.py directed(); the CPU test checks their decision margins) --------------

_DIRECTED = {}


def _directed(key):
    if not _DIRECTED:
        _DIRECTED.update(mm.directed(lambda name: _shape(name)[0]))
    return _DIRECTED[key]


def _play(monkeypatch, key):
    name, ops, _ = _directed(key)
    return _run(monkeypatch, name, {}, ops)


def test_lbfgs_mat_returns_with_its_result_in_use(monkeypatch):
    """aqc_ws_optim.cpp aqc_ws_lbfgs_mat: lb_trial_kernel writes every trial into the workspace's theta buffer.  With one trial per
    line search a lane that rejects it ends at x_out with the rejected trial in the buffer.  What follows without a set_thetas --
    eval(NULL), apply, sketch_generate('eigen') -- must run at x_out."""
    name, ops, _ = _directed("lbfgs")
    call = [a for op, a in ops if op == "lbfgs_mat"][0]
    ref = mm.lbfgs_reference(_shape(name)[6], ops[1][1]["data"], ops[0][1]["data"], call["x0"], 2, 2, 1)
    rejected = [bool((it["step"] == 0)[it["active_in"]].any()) for it in ref["trace"]]
    assert rejected[-1] and min(mm.lbfgs_margins(ref)) > 1e-6, (rejected, min(mm.lbfgs_margins(ref)))   # the case really occurs, clear of a tie
    _play(monkeypatch, "lbfgs")


@pytest.mark.parametrize("name,route", [("sq6", "persistent"), ("sq6", "wide"), ("sq7", "wide"), ("sq7", "auto")])
def test_cd_minimize_leaves_its_best_thetas_in_use_on_every_route(monkeypatch, name, route):
    """aqc_ws_extra.cpp cd_minimize_checked: the persistent launch never touched the workspace's thetas.  On every route
    best_thetas are in use afterwards: V X from a fresh X and <W|Y> agree with the oracle at the thetas the call returned.  (On the
    wide route the earlier code left the last sweep's thetas; a sweep never raises the objective, so those are the best ones and
    this test cannot tell the two apart there -- DESIGN 6t.)"""
    _play(monkeypatch, f"cd_minimize:{name}:{route}")


@pytest.mark.parametrize("name", ["sq6", "sq6_1"])
def test_cd_sweeps_leave_the_returned_thetas_in_use(monkeypatch, name):
    _play(monkeypatch, f"cd_sweeps:{name}")


@pytest.mark.parametrize("kind", ["alt", "eigen"])
def test_adam_continues_from_its_own_point_whatever_was_called_in_between(monkeypatch, kind):
    """aqc_ws_sketch.cpp aqc_ws_sketch_adam: reset = 0 resumed from the workspace's thetas in use, which set_thetas and an
    evaluation of a validation point between two chunks move while m, v and t carry on.  Two chunks with such a visit in between
    equal one uninterrupted run of the same length bit for bit (the sums run in a fixed order)."""
    name, ops, extras = _directed(f"adam:{kind}")
    _play(monkeypatch, f"adam:{kind}")                                   # the uninterrupted run against the reference walk
    u, a, other = ops[4][1]["U"], ops[5][1], extras["other"]
    x0, idx = a["x0"], a["alt_idx"]
    kw = dict(tol=0.0, seed=a["seed"], **mm.ADAM_KW)
    whole_ws, ws = _maker(name)(), _maker(name)()
    try:
        for w in (whole_ws, ws):
            w.sketch_target(u)
        whole = whole_ws.sketch_adam(kind, x0, 4, 0.1, alt_idx=idx, **kw)
        first = ws.sketch_adam(kind, x0, 2, 0.1, alt_idx=None if idx is None else idx[:3], **kw)
        ws.upload(BUF_Y, ops[0][1]["data"])
        ws.upload(BUF_X, ops[1][1]["data"])
        _, g_val = ws.eval(other, True, False, True, BUF_X)              # a validation point
        ws.set_thetas(other[::-1].copy())
        second = ws.sketch_adam(kind, None, 2, 0.1, iter0=2, reset=0, alt_idx=None if idx is None else idx[2:], **kw)
    finally:
        whole_ws.close()
        ws.close()
    assert np.all(np.isfinite(g_val))
    assert np.array_equal(first["profile"], whole["profile"][:, :3]) and np.array_equal(second["profile"], whole["profile"][:, 2:])
    for key in ("x", "best_f", "best_x"):
        assert np.array_equal(second[key], whole[key]), key


@pytest.mark.parametrize("name,call", [("rect7", "lbfgs_mat"), ("sq7", "cd_minimize"), ("sk7", "sketch_adam")])
def test_results_copied_behind_a_long_running_call_are_the_evaluations_own(monkeypatch, name, call):
    """objective_launch + results_async, a long-running call that overwrites the gradients on the device, results_fetch: the
    fetch returns the evaluation's gradients."""
    _play(monkeypatch, f"results:{name}:{call}")


def test_long_running_calls_back_to_back(monkeypatch):
    """Each call starts from what the one before left in use and scribbled on: L-BFGS, the persistent and the wide coordinate
    descent on a square workspace; ADAM, L-BFGS and ADAM's continuation on a sketching one."""
    _play(monkeypatch, "back_to_back:sq6")
    _play(monkeypatch, "back_to_back:sk7")


def test_refused_identity_leaves_the_buffer_and_what_was_derived_from_it(monkeypatch):
    """aqc_api.cpp aqc_ws_set_identity on a rectangle is refused: the buffer, a gradient taken from it afterwards and everything
    else read later are as if the call had not been made."""
    _play(monkeypatch, "identity:rect7")
