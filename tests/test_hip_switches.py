"""GPU: a workspace keeps the switches it was created with (include/aqc_switches.def), whatever the environment says afterwards."""
import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests.helpers import TOL, maxdiff
from tests.test_hip_fused_loads import _BIG, _CASES, _env

pytestmark = pytest.mark.gpu


def test_switches_belong_to_the_workspace():
    """Three workspaces in one process, the middle one created under AQC_GRAPH=0: each reads back its own value, and with the variable
    gone again the same one-call evaluation gives the same bits on all three (a graph replay runs the same kernels)."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure
    from aqc_research_amd.engine import BUF_X, BUF_Y, HipContext, Workspace

    n = 9
    rng = np.random.default_rng(909)
    circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", 14))
    th = orc.rand_thetas(circ.num_thetas, rng)[None, :]
    tg = orc.rand_state(n, rng)[None, :]
    flips = np.array([0, 1, 1 << (n - 1)], dtype=np.int64)
    ctx = HipContext.of(circ)
    with _env(AQC_GRAPH=None):
        a = Workspace(ctx, batch=1)
        with _env(AQC_GRAPH="0"):
            b = Workspace(ctx, batch=1)
        c = Workspace(ctx, batch=1)
        assert [w.switch("AQC_GRAPH") for w in (a, b, c)] == [1, 0, 1]
        with pytest.raises(RuntimeError):
            a.switch("AQC_CD_CHAIN")   # read by the call, not kept by the workspace
        results = []
        for w in (a, b, c):
            w.upload(BUF_Y, tg)
            w.set_basis(BUF_X, 0)
            w.gather_setup(flips)
            for _ in range(2):   # (the second call replays what the first captured, where the workspace uses graphs)
                hs, g = w.eval(th, gather=True)
            results.append((hs.copy(), g.copy()))
            w.close()
    vh = orc.v_dagger_mul_vec(circ, th[0], tg[0])
    x = np.zeros(1 << n, complex)
    x[0] = 1.0
    ref = orc.grad_of_dot_product(circ, th[0], x, vh)
    for name, (hs, g) in zip("ABC", results):
        da, dg = maxdiff(hs[0], vh[flips]), maxdiff(g[0], ref)
        print(f"workspace {name} vs oracle: amplitudes {da:.3e} gradients {dg:.3e}")
        assert da < TOL and dg < TOL, name
        assert np.array_equal(hs, results[0][0]) and np.array_equal(g, results[0][1]), name


@pytest.mark.parametrize("case", ["uvalid_mask", "partial_projections"])
def test_fused_pass_block_count_belongs_to_the_workspace(case):
    """The in-process twin of test_fused_pass_with_four_blocks_per_wave: one workspace created under AQC_PROJECTED_FUSED_QB=2 and one
    under =4 in the same process, each held to the oracle at that test's tolerance (lane 2's target scaled by 2^40, as there)."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure
    from aqc_research_amd.engine import BUF_X, BUF_Y, HipContext, Workspace

    n, blocks, tile, want, _ = _CASES[case]
    rng = np.random.default_rng(4200 + 100 * n + blocks)
    circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", blocks))
    th = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(3)])
    tg = np.stack([orc.rand_state(n, rng) for _ in range(3)])
    tg[2] *= _BIG
    scale = np.array([1.0, 1.0, 1.0 / _BIG])[:, None]
    flips = np.array([0] + [1 << q for q in range(n)], dtype=np.int64)
    x = np.zeros(1 << n, complex)
    x[0] = 1.0
    oracle = []
    for b in range(3):
        vh = orc.v_dagger_mul_vec(circ, th[b], tg[b] * scale[b, 0])
        oracle.append((vh[flips], orc.grad_of_dot_product(circ, th[b], x, vh)))
    route = dict(AQC_PROJECTED_FUSED=None, AQC_PROJECTED_VDAG=None, AQC_PROJECTED_FUSED_MAX_SHARES=None, AQC_SPARSE_SWEEP="1", AQC_LAZY_Z="1",
                 AQC_SPARSE_MIN_ITEMS="1", AQC_PROJECTED_VDAG_MIN_ELEMS="1")
    made = {}
    for qb in (2, 4):
        with _env(AQC_PROJECTED_FUSED_QB=str(qb), **route):
            made[qb] = Workspace(HipContext(circ), batch=3, tile_bits_apply=tile, tile_bits_sweep=tile)
    with _env(AQC_PROJECTED_FUSED_QB=None):   # both exist, and the variable is gone, before either runs
        for qb, ws in made.items():
            assert ws.switch("AQC_PROJECTED_FUSED_QB") == qb
            info = ws.projected_info()
            for key, val in want.items():
                assert info[key] == val, (key, info)
            ws.upload(BUF_Y, tg)
            ws.set_basis(BUF_X, 0)
            ws.gather_setup(flips)
            ws.set_thetas(th)
            ws.objective_launch(BUF_X)
            amps, grads = ws.gather_fetch() * scale, ws.get_grads() * scale
            ws.close()
            for b in range(3):
                da, dg = maxdiff(amps[b], oracle[b][0]), maxdiff(grads[b], oracle[b][1])
                print(f"{case} qb={qb} lane {b} vs oracle: amplitudes {da:.3e} gradients {dg:.3e}")
                assert da < TOL and dg < TOL, (qb, b)
