"""Objective by projection: its independent tile launches in pairs (apply_pair_kernel / sweep_pair_kernel, csrc/aqc_kernels3.hip;
projected_pairs, csrc/aqc_ws_project.cpp) against the single launches (AQC_PROJECTED_PAIRS=0).  Every item is computed by the code
of the single launches, so the results must agree bit for bit: the bound on the difference is 0."""
import functools

import numpy as np
import pytest

from tests.helpers import TOL, maxdiff
from oracle import aqc_oracle as orc

pytestmark = pytest.mark.gpu


def _circ(n, depth):
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    return ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", depth))


def _trotter(n, layers):
    from aqc_research_amd import TrotterAnsatz
    from aqc_research_amd.circuit_structures import make_trotter_like_circuit

    return TrotterAnsatz(n, make_trotter_like_circuit(n, layers), second_order=True)


def _ws(circ, batch, monkeypatch, tile, pairs):
    from aqc_research_amd.engine import HipContext, Workspace

    monkeypatch.setenv("AQC_SPARSE_SWEEP", "1")
    monkeypatch.setenv("AQC_LAZY_Z", "1")
    monkeypatch.setenv("AQC_SPARSE_MIN_ITEMS", "1")
    monkeypatch.setenv("AQC_PROJECTED_VDAG_MIN_ELEMS", "1")
    monkeypatch.setenv("AQC_PROJECTED_PAIRS", "1" if pairs else "0")
    return Workspace(HipContext(circ), batch=batch, tile_bits_apply=tile, tile_bits_sweep=tile)


B = 40


@functools.lru_cache(maxsize=None)
def _case(kind, n, arg, tile, case):
    """Circuit, thetas, targets, basis and gather indices of one shape, and the oracle's results for a few lanes (computed once)."""
    rng = np.random.default_rng(4100 + n + tile + (7 if case == "shifted" else 0))
    circ = _trotter(n, arg) if kind == "trotter" else _circ(n, arg)
    tg = np.stack([orc.rand_state(n, rng) for _ in range(B)])
    ths = [np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(B)]) for _ in range(2)]
    hi = n - tile
    if case == "zero":
        basis = np.zeros(B, dtype=np.int64)
        gather = np.array([0] + [1 << q for q in range(n)], dtype=np.int64)
    else:   # the same index on the first stage's bits, different ones above; the gather set moves above only
        basis = np.array([5 | ((b * 7) % (1 << hi)) << tile for b in range(B)], dtype=np.int64)
        gather = np.array([5 | (f << tile) for f in sorted({0, 1, 2, (1 << hi) - 1, 1 << (hi - 1)})], dtype=np.int64)
    ref = {}
    for b in (0, 13, B - 1):
        vh = orc.v_dagger_mul_vec(circ, ths[1][b], tg[b])
        x = np.zeros(1 << n, complex)
        x[basis[b]] = 1.0
        ref[b] = (vh[gather], orc.grad_of_dot_product(circ, ths[1][b], x, vh))
    return circ, tg, ths, basis, gather, ref


def _kinds(ws):
    from aqc_research_amd._lib import K_APPLY_LIST, K_APPLY_VIRTUAL, K_SWEEP_LIST, K_SWEEP_VIRTUAL

    return tuple(ws.profile_get(k)[0] for k in (K_APPLY_LIST, K_APPLY_VIRTUAL, K_SWEEP_LIST, K_SWEEP_VIRTUAL))


def _run(circ, tg, ths, basis, gather, monkeypatch, tile, pairs):
    """eval and objective_launch for both theta sets, then which launches one more objective_launch made."""
    from aqc_research_amd.engine import BUF_X, BUF_Y

    ws = _ws(circ, B, monkeypatch, tile, pairs)
    info = ws.projected_info()
    ws.upload(BUF_Y, tg)
    ws.set_basis(BUF_X, basis)
    ws.gather_setup(gather)
    got = []
    for th in ths:
        hs, g = ws.eval(th, vdag=True, gather=True, grad=True, x_buf=BUF_X, block_range=(0, circ.num_blocks), front_layer=True)
        got.append((hs.copy(), g.copy()))
    for th in ths:
        ws.set_thetas(th)
        ws.objective_launch(BUF_X)
        got.append((ws.gather_fetch().copy(), ws.get_grads().copy()))
    ws.profile(True)
    ws.set_thetas(ths[0])
    ws.objective_launch(BUF_X)
    ws.sync()
    kinds = _kinds(ws)
    ws.profile(False)
    ws.close()
    return got, kinds, info


def _assert_identical(on, off):
    for (hs1, g1), (hs0, g0) in zip(on, off):
        print("max |pairs - single launches|: amplitudes", maxdiff(hs1, hs0), "gradients", maxdiff(g1, g0))
        assert maxdiff(hs1, hs0) == 0.0 and maxdiff(g1, g0) == 0.0


@pytest.mark.parametrize("grid", [None, "3"])
@pytest.mark.parametrize("case", ["zero", "shifted"])
def test_pairs_equal_the_single_launches(case, grid, monkeypatch):
    """14 qubits, 40 blocks, 2^12 tiles, 40 lanes: one virtual stage of the real plans' tile size, so all three pairs run.  With
    AQC_SWEEP_GRID=3 (6 apply and 3 sweep workgroups for 40 + 40 items) every workgroup walks several items of both lists and one
    share is shorter than the others: the phase change inside a workgroup is exercised many times over."""
    circ, tg, ths, basis, gather, ref = _case("spin", 14, 40, 12, case)
    if grid:
        monkeypatch.setenv("AQC_SWEEP_GRID", grid)
    on, kinds_on, info = _run(circ, tg, ths, basis, gather, monkeypatch, 12, True)
    off, kinds_off, _ = _run(circ, tg, ths, basis, gather, monkeypatch, 12, False)
    assert info, "this shape has a projected route"
    # (list apply, virtual apply, list sweep, virtual sweep) launches of one objective_launch
    assert kinds_off == (2, 2, 1, 1), kinds_off
    assert kinds_on == (0, 2, 1, 0), kinds_on   # the pairs are recorded as virtual apply (two) and list sweep (one)
    _assert_identical(on, off)
    for b, (hs_ref, g_ref) in ref.items():
        for hs, g in (on[1], on[3]):   # eval and objective_launch with the second theta set
            assert maxdiff(hs[b], hs_ref) < TOL and maxdiff(g[b], g_ref) < TOL


@pytest.mark.parametrize("kind,n,arg,tile,paired", [("spin", 14, 24, 8, False), ("trotter", 14, 2, 12, False), ("spin", 13, 18, 8, True),
                                                    ("spin", 15, 30, 10, True), ("spin", 14, 24, 11, True)])
def test_shapes_off_the_headline_form(kind, n, arg, tile, paired, monkeypatch):
    """Two virtual stages (14 qubits, 24 blocks, 2^8 tiles) and a Trotter circuit whose virtual tiles are smaller than the real ones: the
    route keeps its single launches.  One virtual stage of 2^8, 2^10 and 2^11 tiles: no persistent walk, the pair is the two lists
    behind each other in one grid.  The same bits either way."""
    circ, tg, ths, basis, gather, ref = _case(kind, n, arg, tile, "zero")
    on, kinds_on, info = _run(circ, tg, ths, basis, gather, monkeypatch, tile, True)
    off, kinds_off, _ = _run(circ, tg, ths, basis, gather, monkeypatch, tile, False)
    print("projected route:", info, "launches with pairs", kinds_on, "without", kinds_off)
    assert info, "this shape has a projected route"
    assert kinds_on == ((0, 2, 1, 0) if paired else kinds_off), kinds_on
    _assert_identical(on, off)
    for b, (hs_ref, g_ref) in ref.items():
        assert maxdiff(on[3][0][b], hs_ref) < TOL and maxdiff(on[3][1][b], g_ref) < TOL


def test_pairs_alternate_with_other_calls_on_one_workspace(monkeypatch):
    """Pairs, then a surrogate evaluation and a dense sweep (which need what the paired route does not: all of Z, the full-size
    stages), then pairs again with new thetas: the last results equal those of a fresh workspace."""
    from aqc_research_amd.engine import BUF_X, BUF_Y, BUF_Z

    circ, tg, ths, basis, gather, _ = _case("spin", 14, 40, 12, "zero")
    ws = _ws(circ, B, monkeypatch, 12, True)
    ws.upload(BUF_Y, tg)
    ws.set_basis(BUF_X, basis)
    ws.gather_setup(gather)
    ws.set_thetas(ths[0])
    ws.objective_launch(BUF_X)
    ws.sync()
    w = np.full(B, 0.3)
    mx = np.arange(B, dtype=np.int64) % len(gather)
    ws.surrogate_eval(ths[0], w.copy(), mx.copy(), 2, (0, circ.num_blocks), True)
    ws.set_basis(BUF_X, basis)
    ws.set_thetas(ths[0])
    ws.apply(True, BUF_Y, BUF_Z)   # the whole V^H
    ws.grad()                  # a sweep outside the one-call evaluations
    ws.set_thetas(ths[1])
    ws.objective_launch(BUF_X)
    again = (ws.gather_fetch().copy(), ws.get_grads().copy())
    ws.close()
    fresh = _ws(circ, B, monkeypatch, 12, True)
    fresh.upload(BUF_Y, tg)
    fresh.set_basis(BUF_X, basis)
    fresh.gather_setup(gather)
    fresh.set_thetas(ths[1])
    fresh.objective_launch(BUF_X)
    first = (fresh.gather_fetch().copy(), fresh.get_grads().copy())
    fresh.close()
    _assert_identical([again], [first])
