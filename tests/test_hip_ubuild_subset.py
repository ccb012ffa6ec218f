"""The U builder of the objective-by-projection route (ensure_umat, csrc/aqc_ws_sweep.cpp): with AQC_UBUILD_SUBSET=1 it builds the plane
sets that route reads -- V^H's last stage, the sweep's first stage, the virtual plans -- and a later caller that needs every set builds
them from the unchanged thetas.  The unitaries are the same whichever list a job came from, so every result equals that of a workspace
that always builds everything (AQC_UBUILD_SUBSET=0) bit for bit: the bound on the difference is 0; against the compiled CPU oracle 1e-10."""
import functools

import numpy as np
import pytest

from tests.helpers import maxdiff
from oracle import aqc_oracle as orc
from oracle import aqc_ref as cref

pytestmark = pytest.mark.gpu

ORACLE_TOL = 1e-10
B = 4
# the two smallest shapes of test_objective_by_projection_equals_the_stages_of_vdag: 2^8 tiles (two virtual stages) and 2^12 (one, the headline's form)
SHAPES = [(14, 24, 8), (14, 40, 12)]


def _ws(circ, monkeypatch, tile, subset="1", mirror="1"):
    from aqc_research_amd.engine import HipContext, Workspace

    monkeypatch.setenv("AQC_SPARSE_SWEEP", "1")
    monkeypatch.setenv("AQC_LAZY_Z", "1")
    monkeypatch.setenv("AQC_SPARSE_MIN_ITEMS", "1")
    monkeypatch.setenv("AQC_PROJECTED_VDAG_MIN_ELEMS", "1")
    monkeypatch.setenv("AQC_UBUILD_SUBSET", subset)
    monkeypatch.setenv("AQC_UBUILD_MIRROR", mirror)   # 0: V^H has U-builder jobs of its own, the subset takes those of its last stage
    return Workspace(HipContext(circ), batch=B, tile_bits_apply=tile, tile_bits_sweep=tile)


@functools.lru_cache(maxsize=None)
def _case(n, depth, tile):
    """Circuit, targets, two theta sets, the gather set (|0> and its flips: inside the lhs tile below bit `tile`, outside above) and the
    oracle's V^H y, amplitudes and gradient of every lane for both theta sets -- computed once, never modified."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    rng = np.random.default_rng(5200 + n + tile)
    circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", depth))
    tg = np.stack([orc.rand_state(n, rng) for _ in range(B)])
    ths = [np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(B)]) for _ in range(2)]
    gather = np.array([0] + [1 << q for q in range(n)], dtype=np.int64)
    x = np.zeros(1 << n, complex)
    x[0] = 1.0
    ref = []
    for th in ths:
        vh = np.stack([cref.v_dagger_mul_vec(circ, th[b], tg[b]) for b in range(B)])
        g = np.stack([cref.grad_of_dot_product(circ, th[b], x, vh[b]) for b in range(B)])
        for a in (vh, g):
            a.setflags(write=False)
        ref.append((vh, g))
    return circ, tg, ths, gather, ref


def _start(ws, tg, gather):
    from aqc_research_amd.engine import BUF_X, BUF_Y

    ws.upload(BUF_Y, tg)
    ws.set_basis(BUF_X, 0)
    ws.gather_setup(gather)


def _launch(ws, th):
    from aqc_research_amd.engine import BUF_X

    ws.set_thetas(th)
    ws.objective_launch(BUF_X)
    return ws.gather_fetch().copy(), ws.get_grads().copy()


def _same(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        d = maxdiff(a, b)
        print(f"{what}: result {i}: max |subset - everything| = {d}")
        assert d == 0.0


def _near(a, b, what):
    d = maxdiff(a, b)
    print(f"{what}: max |HIP - oracle| = {d:.3e}")
    assert d <= ORACLE_TOL


@pytest.mark.parametrize("n,depth,tile,mirror", [SHAPES[0] + ("1",), SHAPES[1] + ("1",), SHAPES[0] + ("0",)])
def test_subset_equals_everything_and_the_oracle(n, depth, tile, mirror, monkeypatch):
    """Amplitudes and gradients of objective_launch for two theta sets; the launch profile says which list ran: with the subset a
    download of Z (the whole V^H from Y) builds the remaining plane sets by a second U-builder launch, without it nothing is left to build."""
    from aqc_research_amd._lib import K_COEF
    from aqc_research_amd.engine import BUF_Z

    circ, tg, ths, gather, ref = _case(n, depth, tile)
    got, coef = {}, {}
    for subset in ("1", "0"):
        ws = _ws(circ, monkeypatch, tile, subset, mirror)
        assert ws.projected_info(), "this shape has a projected route"
        _start(ws, tg, gather)
        got[subset] = [a for th in ths for a in _launch(ws, th)]
        ws.profile(True)
        got[subset] += list(_launch(ws, ths[0]))
        ws.sync()
        first = ws.profile_get(K_COEF)
        got[subset].append(ws.download(BUF_Z))
        coef[subset] = (first, ws.profile_get(K_COEF))
        ws.profile(False)
        ws.close()
    print("U-builder launches (count, ms) after objective_launch / after download(Z): subset", coef["1"], "everything", coef["0"])
    assert coef["1"][0][0] == 1 and coef["1"][1][0] == 2, "the subset ran, and the reader of the whole V^H built the rest"
    assert coef["0"][0][0] == 1 and coef["0"][1][0] == 1
    _same(got["1"], got["0"], "objective_launch")
    for i, (vh, g) in enumerate(ref):
        _near(got["1"][2 * i], vh[:, gather], "amplitudes")
        _near(got["1"][2 * i + 1], g, "gradients")
    _near(got["1"][6], ref[0][0], "Z after download")


# ---- call sequences: every step returns the arrays it delivered and the oracle's values for them -----------------------------------
def _step_launch(k):
    def step(ws, c):
        hs, g = _launch(ws, c["ths"][k])
        return [(hs, c["ref"][k][0][:, c["gather"]], "amplitudes"), (g, c["ref"][k][1], "gradients")]
    return step


def _step_download(k):   # a reader of all of Z: the whole V^H from Y, by every stage
    def step(ws, c):
        from aqc_research_amd.engine import BUF_Z

        return [(ws.download(BUF_Z), c["ref"][k][0], "Z")]
    return step


def _step_dense_grad(k):   # a sweep by its stages over every tile, thetas unchanged
    def step(ws, c):
        ws.grad()
        return [(ws.get_grads().copy(), c["ref"][k][1], "gradients of the dense sweep")]
    return step


def _step_new_thetas_apply(k):
    def step(ws, c):
        from aqc_research_amd.engine import BUF_Y, BUF_Z

        ws.set_thetas(c["ths"][k])
        ws.apply(True, BUF_Y, BUF_Z)
        return []
    return step


def _step_evals(gather, order):   # aqc_ws_eval with new thetas: captured once, replayed afterwards
    def step(ws, c):
        from aqc_research_amd.engine import BUF_X

        for k in order:
            hs, g = ws.eval(c["ths"][k], vdag=True, gather=gather, grad=True, x_buf=BUF_X, block_range=(0, c["circ"].num_blocks), front_layer=True)
        k = order[-1]
        out = [(g.copy(), c["ref"][k][1], "gradients")]
        if gather:
            out.append((hs.copy(), c["ref"][k][0][:, c["gather"]], "amplitudes"))
        return out
    return step


SEQUENCES = {
    "download": [_step_launch(0), _step_download(0)],
    "dense_grad": [_step_launch(0), _step_dense_grad(0)],
    "new_thetas_apply": [_step_launch(0), _step_new_thetas_apply(1), _step_download(1)],
    # few lanes: with the gather the amplitudes ride in the walk and V^H runs its stages (everything is built); without it the graph
    # holds the route by projection, whose U-builder node builds the subset
    "graph_replay": [_step_launch(1), _step_evals(True, (1, 0, 1)), _step_evals(False, (0, 1, 0, 1)), _step_download(1)],
}


def _run_steps(steps, monkeypatch, c, tile, subset):
    ws = _ws(c["circ"], monkeypatch, tile, subset)
    _start(ws, c["tg"], c["gather"])
    out = [step(ws, c) for step in steps]
    ws.close()
    return out


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_no_stale_planes_after_the_subset(name, monkeypatch):
    """Call sequences on ONE workspace in which the subset is followed by a reader of plane sets it did not build.  After each step:
    the same bits as a FRESH workspace that always builds everything and has run the sequence up to that step, and the oracle's values."""
    n, depth, tile = SHAPES[0]
    circ, tg, ths, gather, ref = _case(n, depth, tile)
    c = dict(circ=circ, tg=tg, ths=ths, gather=gather, ref=ref)
    steps = SEQUENCES[name]
    got = _run_steps(steps, monkeypatch, c, tile, "1")
    for k in range(len(steps)):
        if not got[k]:
            continue
        fresh = _run_steps(steps[: k + 1], monkeypatch, c, tile, "0")[k]
        _same([a for a, _, _ in got[k]], [a for a, _, _ in fresh], f"{name}, step {k}")
        for a, want, what in got[k]:
            _near(a, want, f"{name}, step {k}: {what}")


def test_a_captured_evaluation_by_projection_builds_the_subset(monkeypatch):
    """Profiling switches the graphs off, so the replayed U builder cannot be counted directly.  What it left can: once the replays
    are over, the first reader of the whole V^H (download of Z) launches the U builder again when the graph built the subset, and
    launches nothing when everything was built."""
    from aqc_research_amd._lib import K_COEF
    from aqc_research_amd.engine import BUF_Z

    n, depth, tile = SHAPES[0]
    circ, tg, ths, gather, ref = _case(n, depth, tile)
    c = dict(circ=circ, tg=tg, ths=ths, gather=gather, ref=ref)
    count, z = {}, {}
    for subset in ("1", "0"):
        ws = _ws(circ, monkeypatch, tile, subset)
        _start(ws, tg, gather)
        _step_evals(False, (0, 1, 0, 1))(ws, c)
        ws.profile(True)
        z[subset] = ws.download(BUF_Z)
        count[subset] = ws.profile_get(K_COEF)[0]
        ws.profile(False)
        ws.close()
    print("U-builder launches of download(Z) after the replays: subset", count["1"], "everything", count["0"])
    assert count == {"1": 1, "0": 0}
    _same([z["1"]], [z["0"]], "Z after the replays")
    _near(z["1"], ref[1][0], "Z after the replays")
