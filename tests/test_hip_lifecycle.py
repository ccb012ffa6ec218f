"""GPU: every handle behind the ABI owns its device and pinned memory (csrc/aqc_devbuf.h), so the library's count of live
allocations (aqc_live_buffers) is back at its earlier value after every destroy, grow-only buffers only grow, and a refused
creation leaves nothing.  Shapes: the smallest the other GPU tests use for each path."""
import ctypes
import gc

import numpy as np
import pytest

from oracle import aqc_oracle as orc

pytestmark = pytest.mark.gpu


def _live():
    from aqc_research_amd.engine import live_buffers

    return live_buffers()


@pytest.fixture
def baseline():
    gc.collect()   # handles earlier tests dropped without closing go now, not in the middle of a count
    return _live()


def _drop(ctx):
    ctx.__del__()   # aqc_destroy: the context and its one-shot workspaces
    assert ctx.handle is None


def _spin(n, ent="cx", depth=None):
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    return ParametricCircuit(n, ent, create_ansatz_structure(n, "spin", "full", 18 if depth is None else depth))


def _trotter(n, layers):
    from aqc_research_amd import TrotterAnsatz
    from aqc_research_amd.circuit_structures import make_trotter_like_circuit

    return TrotterAnsatz(n, make_trotter_like_circuit(n, layers), second_order=True)


def _rand_mps(n, bond, rng):
    """A Qiskit-style MPS tuple with every inner bond `bond` (capped by the register): what Workspace.mps_upload marshals."""
    dims = [min(bond, 1 << min(q, n - q)) for q in range(n + 1)]
    gam = [tuple(rng.standard_normal((dims[q], dims[q + 1])) + 1j * rng.standard_normal((dims[q], dims[q + 1])) for _ in range(2)) for q in range(n)]
    lam = [rng.uniform(0.5, 1.0, dims[q + 1]) for q in range(n - 1)]
    return gam, lam


def _state_vector_everything(monkeypatch, rng):
    """13 qubits, tile 8, 18 blocks, 4 lanes, sparse and projected routes forced: every lazily allocated member of the state-vector path."""
    from aqc_research_amd import _lib
    from aqc_research_amd.engine import BUF_X, BUF_Y, BUF_Z, HipContext, Workspace

    n, B = 13, 4
    monkeypatch.setenv("AQC_SPARSE_MIN_ITEMS", "1")
    monkeypatch.setenv("AQC_PROJECTED_VDAG_MIN_ELEMS", "1")
    circ = _spin(n)
    ctx = HipContext(circ)
    ws = Workspace(ctx, batch=B, tile_bits_apply=8, tile_bits_sweep=8)
    T = circ.num_thetas
    ws.upload(BUF_Y, np.stack([orc.rand_state(n, rng) for _ in range(B)]))
    ws.set_basis(BUF_X, np.arange(B, dtype=np.int64) * 37 + 5)
    flips = np.array([5] + [5 ^ (1 << q) for q in range(n)], dtype=np.int64)
    ws.gather_setup(flips)
    th = np.stack([orc.rand_thetas(T, rng) for _ in range(B)])
    ws.set_thetas(th)
    ws.objective_launch(BUF_X)
    ws.sync()
    for _ in range(2):   # graph capture, then replay
        ws.eval(th, vdag=True, gather=True, grad=True, x_buf=BUF_X)
    ws.download(BUF_Z)
    ws.vdot(BUF_X, BUF_Y)
    ws.gather(BUF_Y, flips[:3])
    ws.set_combo(BUF_X, np.tile(np.array([5, 6], dtype=np.int64), (B, 1)), np.tile(np.array([1.0, 0.5 + 0j]), (B, 1)))
    ws.theta_bank(np.stack([th, th]))
    weight, max_no = np.ones(B), np.zeros(B, dtype=np.int64)
    ws.surrogate_eval(th, weight, max_no)
    ws.surrogate_eval(th, weight, max_no, real_only=True)
    xo, f, i64 = np.empty_like(th), np.empty(B), ctypes.POINTER(ctypes.c_int64)
    nit, nfev = np.zeros(B, dtype=np.int64), ctypes.c_int64()
    _lib.check(ws._L.aqc_ws_lbfgs(ws.handle, _lib.dptr(th), 2, 4, 1e-6, 1e-10, 2.0, 4, -1, -1, 1, _lib.dptr(xo), _lib.dptr(f), None,
                                  nit.ctypes.data_as(i64), ctypes.byref(nfev), None, None))
    ws.results_async()
    ws.results_fetch()
    # the context's one-shot workspace (host-pointer entry points)
    out = np.empty(1 << n, dtype=np.complex128)
    _lib.check(ws._L.aqc_v_mul_vec(ctx.handle, _lib.dptr(th[0]), _lib.dptr(orc.rand_state(n, rng)), _lib.dptr(out)))
    return ctx, ws


def _second_scratch_pair(monkeypatch, rng):
    """test_three_or_more_stages_second_scratch_pair's smaller shape: w2 / zw2."""
    from aqc_research_amd.engine import BUF_X, BUF_Y, HipContext, Workspace

    n, B = 13, 3
    monkeypatch.setenv("AQC_SPARSE_MIN_ITEMS", "1")
    circ = _trotter(n, 2)
    ctx = HipContext(circ)
    ws = Workspace(ctx, batch=B, tile_bits_apply=9, tile_bits_sweep=9)
    assert ws.plan_info(1)[0] >= 3
    ws.upload(BUF_Y, np.stack([orc.rand_state(n, rng) for _ in range(B)]))
    ws.set_basis(BUF_X, np.full(B, 0x0AAA, dtype=np.int64))
    ws.gather_setup([0x0AAA, 0x0AAB])
    ws.set_thetas(np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(B)]))
    ws.objective_launch(BUF_X)
    ws.sync()
    return ctx, ws


def _sketched_adam(rng):
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.engine import HipContext, Workspace

    n, k, B, niter = 5, 8, 2, 1
    circ = ParametricCircuit(n, "cx", orc.spin_blocks(n, 12))
    ctx = HipContext(circ)
    ws = Workspace(ctx, batch=B, ncols=k)
    d = 1 << n
    ws.sketch_target(np.stack([np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0] for _ in range(B)]))
    th = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(B)])
    idx = np.stack([np.stack([rng.permutation(d)[:k] for _ in range(B)]) for _ in range(niter + 1)]).astype(np.int32)
    ws.sketch_adam("rand", th, niter, 0.1, seed=3)
    ws.sketch_adam("alt", th, niter, 0.1, alt_idx=idx, reset=1)
    ws.sketch_adam("eigen", th, niter, 0.1, seed=3, reset=1)
    return ctx, ws


def _coordinate_descent(monkeypatch, rng):
    from aqc_research_amd import ParametricCircuit, _lib
    from aqc_research_amd.engine import BUF_Y, HipContext, Workspace

    n = 6
    d = 1 << n
    circ = ParametricCircuit(n, "cx", orc.spin_blocks(n, 6))
    ctx = HipContext(circ)
    ws = Workspace(ctx, batch=1, ncols=d)
    ws.upload(BUF_Y, np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0][None])
    th, fobj = orc.rand_thetas(circ.num_thetas, rng), np.zeros(2)
    _lib.check(ws._L.aqc_ws_cd_sweeps(ws.handle, _lib.dptr(th), _lib.dptr(fobj), 2, -1))
    monkeypatch.setenv("AQC_CD_CHAIN", "1")   # the wide walk: the driver's buffers belong to the workspace
    _lib.check(ws._L.aqc_ws_cd_sweep(ws.handle, _lib.dptr(th), _lib.dptr(fobj)))
    return ctx, ws


def _mps_slots(rng):
    from aqc_research_amd.engine import BUF_X, HipContext, Workspace

    n = 8
    ctx = HipContext(_spin(n, depth=8))
    ws = Workspace(ctx, batch=2)
    for bond in (2, 6):   # one shape, then a larger one into the same slot
        ws.mps_upload(0, _rand_mps(n, bond, rng))
        ws.mps_to_vec(0, BUF_X, 1)
    ws.mps_upload(1, _rand_mps(n, 3, rng))
    ws.mps_dot(0, 1)
    ws.sync()
    return ctx, ws


def _mps_engines(monkeypatch, rng):
    """One evaluation on the single-lane engine and one on the lockstep lanes; returns what is still alive."""
    from aqc_research_amd import mps_engine as me
    from aqc_research_amd.model_sp_lhs.trotter import neel_state_index

    monkeypatch.setenv("AQC_MPS_APPLY", "single")   # (the default route keeps a module-level lane alive: not this test's handle)
    n, lanes = 8, 2
    circ = _trotter(n, 1)
    th = 0.3 * orc.rand_thetas(circ.num_thetas, rng)
    basis = me.DeviceMPS.basis_state(n, neel_state_index(n))
    target = me.v_mul_mps(circ, th, basis, trunc_thr=1e-12, method="single")
    vh = me.v_dagger_mul_mps(circ, th, target, trunc_thr=1e-12, method="single")
    me.fast_dot_gradient_mps(circ, th, basis, vh, trunc_thr=1e-12, method="single")
    basis.dot(vh)
    vh.to_qiskit()
    me.svd(rng.standard_normal((7, 3)) + 0j)
    ls = me.LockstepLanes(n, lanes).set_targets(target).set_lhs(basis)
    ls.evaluate(circ, np.stack([th, 1.1 * th]), trunc_thr=1e-9)
    ls.set_lhs_basis(np.zeros((lanes, n), dtype=np.uint8))
    ls.gate2_stats(enable=False)
    return [basis, target, vh, ls]


def test_nothing_outlives_its_handle(baseline, monkeypatch):
    from aqc_research_amd.engine import qr, zgemm

    rng = np.random.default_rng(2024)
    for build in (_state_vector_everything, _second_scratch_pair, _coordinate_descent):
        ctx, ws = build(monkeypatch, rng)
        assert _live()[0] > baseline[0] and _live()[1] > baseline[1]
        ws.close()
        _drop(ctx)
        assert _live() == baseline, build.__name__
    for build in (_sketched_adam, _mps_slots):
        ctx, ws = build(rng)
        ws.close()
        _drop(ctx)
        assert _live() == baseline, build.__name__
    a = rng.standard_normal((16, 4)) + 1j * rng.standard_normal((16, 4))
    qr(a)
    zgemm(a, a, conj_trans_a=True)
    assert _live() == baseline   # call-scoped buffers
    alive = _mps_engines(monkeypatch, rng)
    assert _live()[0] > baseline[0]
    for h in alive:
        h.close()
    assert _live() == baseline


def test_grow_only_means_grow_only(baseline):
    from aqc_research_amd.engine import HipContext, Workspace

    rng = np.random.default_rng(7)
    n = 8
    ctx = HipContext(_spin(n, depth=8))
    ws = Workspace(ctx, batch=2)

    def grows(requests, buffers):
        """requests small, large, small over `buffers` grow-only buffers"""
        start = _live()
        first, largest, again = [(req(), _live())[1] for req in requests]
        assert 0 <= first[0] - start[0] <= buffers           # at most one allocation per buffer on first use
        assert first[0] <= largest[0] <= start[0] + buffers  # a larger request replaces a block, it does not add one
        assert again == largest                              # the smaller repeat changes nothing
        assert first[1] == largest[1] == start[1]            # (no pinned block involved at these sizes)

    grows([lambda k=k: ws.gather_setup(list(range(k))) for k in (3, 9, 3)], buffers=2)   # the index list and the gathered amplitudes
    mps = {b: _rand_mps(n, b, rng) for b in (2, 8)}
    grows([lambda b=b: ws.mps_upload(0, mps[b]) for b in (2, 8, 2)], buffers=2)           # the slot's tensors and the Schmidt staging
    ws.close()
    _drop(ctx)
    assert _live() == baseline


def test_a_refused_creation_leaves_nothing(baseline):
    from aqc_research_amd.engine import HipContext, Workspace

    ctx = HipContext(_spin(6, depth=6))
    assert _live() == baseline   # a context holds no device memory of its own
    with pytest.raises(RuntimeError, match="ncols must be >= 1"):
        Workspace(ctx, batch=1, ncols=0)
    assert _live() == baseline
    with pytest.raises(RuntimeError, match="beyond this build's limit"):
        Workspace(ctx, batch=1, ncols=1 << 26)   # 6 + 26 address bits per lane
    assert _live() == baseline
    _drop(ctx)
    assert _live() == baseline
