"""CPU self-test of the call-sequence harness (tests/ws_model.py): the generator is deterministic and respects its
preconditions, and the runner passes against FakeWorkspace, the oracle's rendering of the engine.Workspace surface.  It
also shows the runner catches a workspace that keeps a stale result."""
import numpy as np
import pytest

from tests import ws_model as wm


def _circ(n=8, depth=10):
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    return ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", depth))


def _ops(circ, seed, batch, length=36, tile=5):
    return wm.Gen(seed, circ.num_qubits, batch, circ.num_thetas, circ.num_blocks, tile).sequence(length)


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_generator_is_deterministic_and_respects_preconditions(seed):
    circ = _circ()
    ops = _ops(circ, seed, 3)
    assert 25 <= len(ops) <= 45
    assert _same(ops, _ops(circ, seed, 3))
    assert not _same(ops, _ops(circ, seed + 100, 3))
    assert wm.checked_preconditions(ops, 3, circ.num_qubits)


def test_generator_draws_the_dangerous_pairs():
    circ = _circ()
    names = [op[0] for s in range(12) for op in _ops(circ, s, 3)]
    for want in ("objective_launch", "eval", "surrogate_eval", "apply", "grad", "copy_in", "copy_out", "use_theta_set",
                 "gather_setup", "set_combo", "upload_lane"):
        assert want in names, want
    bad = [op for s in range(12) for op in _ops(circ, s, 3) if op[1].get("bad")]
    assert bad, "no refused call drawn"


@pytest.mark.parametrize("seed,batch", [(0, 3), (1, 4), (2, 1), (3, 5)])
def test_runner_passes_against_the_oracle_workspace(seed, batch):
    circ = _circ()
    orc = wm.Oracle(circ)
    ops = _ops(circ, seed, batch)
    reads = wm.run_sequence(lambda: wm.FakeWorkspace(circ, batch, orc), circ, batch, ops, orc)
    assert len(reads) >= 5


class _StaleZ(wm.FakeWorkspace):
    """A workspace whose objective_launch keeps the Z of its first call: what a stale tile list looks like from outside."""

    def objective_launch(self, x, br=None, front=True):
        if getattr(self, "_z0", None) is None:
            super().objective_launch(x, br, front)
            self._z0 = self.b[wm.BUF_Z].copy()
            return
        self._br(br)
        self.b[wm.BUF_Z] = self._z0.copy()
        if self.gidx is not None:
            self.small = self.b[wm.BUF_Z][:, self.gidx]
        self.grad_from(x, br, front)


def test_runner_catches_a_stale_workspace():
    circ = _circ()
    orc = wm.Oracle(circ)
    rng = np.random.default_rng(5)
    ops = [("upload", {"buf": wm.BUF_Y, "data": np.eye(1, 256, 7).repeat(2, 0).astype(complex)}),
           ("set_basis", {"buf": wm.BUF_X, "idx": [1, 2]}),
           ("gather_setup", {"idx": [0, 1]}),
           ("set_thetas", {"th": rng.random((2, circ.num_thetas))}),
           ("objective_launch", {"x": wm.BUF_X, "br": None, "front": True}),
           ("set_thetas", {"th": rng.random((2, circ.num_thetas))}),
           ("objective_launch", {"x": wm.BUF_X, "br": None, "front": True}),
           ("results", {"kind": "get_grads"})]
    wm.run_sequence(lambda: wm.FakeWorkspace(circ, 2, orc), circ, 2, ops, orc)
    with pytest.raises(AssertionError, match="differs from the model"):
        wm.run_sequence(lambda: _StaleZ(circ, 2, orc), circ, 2, ops, orc)
