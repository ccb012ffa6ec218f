"""GPU: objective by projection with the VIRTUAL stage walked back from (M_end, Y_end) (projected_virtual_backwalk, csrc/aqc_ws_project.cpp).

Where the real member walks back (tests/test_hip_backwalk.py) and the virtual plans have one stage each of a tile size that has the
backward form, the launch that takes Y_end down to Y_0 is the virtual stage's backward walk: it forms the virtual plan's R on its way,
the sweep launches no virtual stage and its first stage -- the real walk -- goes alone.  The launch kinds of an evaluation do not show
it, aqc_ws_virtual_backwalk does.
References, as for the real member: V^H by its stages (AQC_PROJECTED_VDAG=0) to 1e-13 -- the bound the suite holds every pair of routes
to: the same sums in another order, fp64 --, the C oracle at the suite's TOL, and the single launches (AQC_PROJECTED_PAIRS=0) bit for
bit.  Shapes: the smallest at which each code path exists (persistent 2^12 form, one and two items per persistent workgroup; four
waves without the persistent walk; the other entanglers; a 2nd-order Trotter ansatz) and two where the route must stay off (two
virtual stages; 2^11 tiles, which have no backward form)."""
import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests.helpers import TOL, maxdiff
from tests.test_hip_backwalk import _cases, _spin, _trotter

pytestmark = pytest.mark.gpu

ROUTES = 1e-13

# name: (circuit, tile, lanes)
ON_ROUTE = {
    "k12": (lambda: _spin(14, "cx", 40), 12, 5),
    "k12_two_items_per_workgroup": (lambda: _spin(14, "cx", 40), 12, 260),
    "k10_four_waves": (lambda: _spin(13, "cx", 30), 10, 5),
    "k12_cz": (lambda: _spin(14, "cz", 40), 12, 5),
    "k12_cp": (lambda: _spin(14, "cp", 40), 12, 5),
    "trotter2_n12": (lambda: _trotter(12, 2), 10, 5),
}
OFF_ROUTE = {
    "k8_two_virtual_stages": (lambda: _spin(14, "cx", 24), 8, 5),
    "k11_no_backward_form": (lambda: _spin(14, "cx", 24), 11, 5),
}
MODES = {   # environment of a workspace
    "route": {},
    "stages": {"AQC_PROJECTED_VDAG": "0"},
    "singles": {"AQC_PROJECTED_PAIRS": "0"},   # the plain Y_0 launch writes Y_0 behind the same walk, which stores nothing
}
_KEYS = ("AQC_PROJECTED_VDAG", "AQC_PROJECTED_PAIRS", "AQC_MIRROR_PLAN", "AQC_R_ONLY_LAST")


def _ws(circ, batch, tile, mode, monkeypatch):
    from aqc_research_amd.engine import HipContext, Workspace

    for k in _KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("AQC_PROJECTED_VDAG_MIN_ELEMS", "1")
    monkeypatch.setenv("AQC_SPARSE_MIN_ITEMS", "1")
    return Workspace(HipContext(circ), batch=batch, tile_bits_apply=tile, tile_bits_sweep=tile)


def _counts(ws):
    from aqc_research_amd._lib import K_APPLY_LIST, K_APPLY_VIRTUAL, K_SWEEP_LIST, K_SWEEP_VIRTUAL

    return tuple(ws.profile_get(k)[0] for k in (K_APPLY_LIST, K_APPLY_VIRTUAL, K_SWEEP_LIST, K_SWEEP_VIRTUAL))


def _inputs(circ, tile, B):
    n = circ.num_qubits
    rng = np.random.default_rng(5300 + n + tile + B)
    tg = np.stack([orc.rand_state(n, rng) for _ in range(min(B, 8))])
    tg = tg[np.arange(B) % len(tg)] * np.exp(1j * np.arange(B))[:, None]   # (many lanes: a few states, a phase per lane)
    th8 = [np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(min(B, 8))]) for _ in range(2)]
    ths = [t[(np.arange(B) + 3 * i) % len(t)] + 1e-3 * np.arange(B)[:, None] for i, t in enumerate(th8)]
    return tg, tg[::-1].copy(), ths


def _walk(ws, circ, tg, tg2, ths, cases):
    """Everything a mode is asked for, in one fixed order of calls; every result copied."""
    from aqc_research_amd.engine import BUF_X, BUF_Y, BUF_Z

    nb = circ.num_blocks
    out = {}
    ws.upload(BUF_Y, tg)
    for name, (basis, gather) in cases.items():
        ws.set_basis(BUF_X, basis)
        ws.gather_setup(gather)
        for i, th in enumerate(ths):   # aqc_ws_eval: the second call of a key replays the captured graph
            hs, g = ws.eval(th, vdag=True, gather=True, grad=True, x_buf=BUF_X, block_range=(0, nb), front_layer=True)
            out[(name, "eval", i)] = (hs.copy(), g.copy())
        for i, th in enumerate(ths):   # without a gather
            _, g = ws.eval(th, vdag=True, gather=False, grad=True, x_buf=BUF_X, block_range=(0, nb), front_layer=True)
            out[(name, "eval_grad", i)] = (np.zeros(0), g.copy())
        for i, th in enumerate(ths):
            ws.set_thetas(th)
            ws.objective_launch(BUF_X)
            out[(name, "launch", i)] = (ws.gather_fetch().copy(), ws.get_grads().copy())
        ws.objective_launch(BUF_X)   # the same call again
        out[(name, "again")] = (ws.gather_fetch().copy(), ws.get_grads().copy())
        ws.objective_launch(BUF_X, block_range=(1, max(2, nb // 2)), front_layer=False)
        out[(name, "restricted")] = (ws.gather_fetch().copy(), ws.get_grads().copy())
    out["z"] = ws.download(BUF_Z)   # a later reader of Z (the last call: the shifted case, thetas ths[-1])
    # a sequence on the same workspace: launch, eval with new thetas, a new target, eval, launch
    seq = []
    ws.set_thetas(ths[0])
    ws.objective_launch(BUF_X)
    seq.append((ws.gather_fetch().copy(), ws.get_grads().copy()))
    hs, g = ws.eval(ths[1], vdag=True, gather=True, grad=True, x_buf=BUF_X, block_range=(0, nb), front_layer=True)
    seq.append((hs.copy(), g.copy()))
    ws.upload(BUF_Y, tg2)
    hs, g = ws.eval(ths[0], vdag=True, gather=True, grad=True, x_buf=BUF_X, block_range=(0, nb), front_layer=True)
    seq.append((hs.copy(), g.copy()))
    ws.objective_launch(BUF_X)   # (the thetas of the last eval)
    seq.append((ws.gather_fetch().copy(), ws.get_grads().copy()))
    out["seq"] = seq
    ws.profile(True)             # which launches one evaluation makes
    ws.objective_launch(BUF_X)
    ws.sync()
    out["counts"] = _counts(ws)
    ws.profile(False)
    return out


@pytest.mark.parametrize("shape", sorted(ON_ROUTE))
def test_virtual_walk_back_equals_the_stages_of_vdag_the_single_launches_and_the_oracle(shape, monkeypatch):
    make, tile, B = ON_ROUTE[shape]
    circ = make()
    n = circ.num_qubits
    tg, tg2, ths = _inputs(circ, tile, B)
    cases = _cases(n, tile, B)
    res = {}
    for mode in MODES:
        ws = _ws(circ, B, tile, mode, monkeypatch)
        info = ws.projected_info()
        assert info and info["stages"] == 1 and info["tile_bits"] == tile, "the shape was chosen for one virtual stage of the real tile size"
        assert ws.virtual_backwalk() == 1, mode   # static per workspace: the plans decide, not the switches of a call
        res[mode] = _walk(ws, circ, tg, tg2, ths, cases)
        ws.close()

    # launch kinds of one objective_launch: (list applies, virtual applies, list sweeps, virtual sweeps)
    assert res["route"]["counts"] == (0, 2, 1, 0), res["route"]["counts"]
    assert res["singles"]["counts"] == (2, 2, 1, 1), res["singles"]["counts"]

    route = res["route"]
    lanes = sorted({0, B // 2, B - 1})
    for key, val in route.items():
        if key in ("counts", "z", "seq"):
            continue
        assert maxdiff(val[0], res["stages"][key][0]) < ROUTES and maxdiff(val[1], res["stages"][key][1]) < ROUTES, key
        # pairs and single launches run the same bodies: not one bit apart
        assert np.array_equal(val[0], res["singles"][key][0]) and np.array_equal(val[1], res["singles"][key][1]), key
    for step, (a, b_) in enumerate(zip(route["seq"], res["singles"]["seq"])):
        assert np.array_equal(a[0], b_[0]) and np.array_equal(a[1], b_[1]), step
    for name, (basis, gather) in cases.items():
        assert np.array_equal(route[(name, "again")][0], route[(name, "launch", 1)][0])   # determinism
        assert np.array_equal(route[(name, "again")][1], route[(name, "launch", 1)][1])
        # graph replays and launches compute the same
        assert maxdiff(route[(name, "eval", 1)][1], route[(name, "launch", 1)][1]) < ROUTES
        assert maxdiff(route[(name, "eval_grad", 1)][1], route[(name, "launch", 1)][1]) < ROUTES
        r_hs, r_g = route[(name, "restricted")]
        s_g = res["stages"][(name, "restricted")][1]
        assert np.array_equal(r_g == 0, s_g == 0) and 0 < np.count_nonzero(r_g) < r_g.size   # outside the range: exact zeros
        for b in lanes:
            x = np.zeros(1 << n, complex)
            x[basis[b]] = 1.0
            for i, th in enumerate(ths):
                vh = orc.v_dagger_mul_vec(circ, th[b], tg[b])
                ref = orc.grad_of_dot_product(circ, th[b], x, vh)
                for how in ("eval", "launch"):
                    assert maxdiff(route[(name, how, i)][0][b], vh[gather]) < TOL, (name, how, i, b)
                    assert maxdiff(route[(name, how, i)][1][b], ref) < TOL, (name, how, i, b)
                assert maxdiff(route[(name, "eval_grad", i)][1][b], ref) < TOL, (name, i, b)
                if i == 1:
                    inside = r_g[b] != 0
                    assert maxdiff(r_hs[b], vh[gather]) < TOL and maxdiff(r_g[b][inside], ref[inside]) < TOL
                    if name == "shifted":   # the Z a later reader gets is the whole V^H y
                        assert maxdiff(route["z"][b], vh) < TOL
    assert maxdiff(route["z"], res["stages"]["z"]) < ROUTES
    # the sequence: against the stages and, its last two steps (new target), against the oracle
    basis, gather = cases["shifted"]
    for step, (a, b_) in enumerate(zip(route["seq"], res["stages"]["seq"])):
        assert maxdiff(a[0], b_[0]) < ROUTES and maxdiff(a[1], b_[1]) < ROUTES, step
    for b in lanes:
        x = np.zeros(1 << n, complex)
        x[basis[b]] = 1.0
        vh = orc.v_dagger_mul_vec(circ, ths[0][b], tg2[b])
        ref = orc.grad_of_dot_product(circ, ths[0][b], x, vh)
        for step in (2, 3):
            assert maxdiff(route["seq"][step][0][b], vh[gather]) < TOL and maxdiff(route["seq"][step][1][b], ref) < TOL, (step, b)


@pytest.mark.parametrize("shape", sorted(OFF_ROUTE))
def test_route_is_off_where_the_virtual_stage_cannot_walk_back(shape, monkeypatch):
    """Two virtual stages (the gradient walk conjugates one sub-stage per plan) and 2^11 tiles (no backward form): the launches of an
    evaluation are those of the forward virtual stage(s), the results the stages' to the routes' bound and the oracle's to TOL."""
    from aqc_research_amd.engine import BUF_X, BUF_Y

    make, tile, B = OFF_ROUTE[shape]
    circ = make()
    n = circ.num_qubits
    tg, _, ths = _inputs(circ, tile, B)
    basis, gather = _cases(n, tile, B)["shifted"]
    res = {}
    for mode in ("route", "stages"):
        ws = _ws(circ, B, tile, mode, monkeypatch)
        info = ws.projected_info()
        assert info, "the shape was chosen for its route"
        assert ws.virtual_backwalk() == 0
        ws.upload(BUF_Y, tg)
        ws.set_basis(BUF_X, basis)
        ws.gather_setup(gather)
        out = []
        for th in ths:
            ws.set_thetas(th)
            ws.objective_launch(BUF_X)
            out.append((ws.gather_fetch().copy(), ws.get_grads().copy()))
        ws.profile(True)
        ws.objective_launch(BUF_X)
        ws.sync()
        res[mode] = (out, _counts(ws), info)
        ws.profile(False)
        ws.close()
    out, counts, info = res["route"]
    nst = info["stages"]
    if nst == 1 and info["tile_bits"] == tile:
        # three pairs: psi with M_end, V^H's last stage with Y_0, the sweep's first stage with the virtual stage
        assert counts == (0, 2, 1, 0), counts
    elif tile == 11:
        # no backward form at all: psi and V^H's last stage over the list, M_end and Y_0 stage by stage, the forward virtual stages
        assert counts == (2, 2 * nst, 1, nst), counts
    else:
        # the real member walks back (no V^H stage), the virtual stages are swept forwards behind it
        assert nst >= 2 and counts == (1, 2 * nst, 1, nst), counts
    for (hs, g), (hs_s, g_s) in zip(out, res["stages"][0]):
        assert maxdiff(hs, hs_s) < ROUTES and maxdiff(g, g_s) < ROUTES
    for b in sorted({0, B // 2, B - 1}):
        x = np.zeros(1 << n, complex)
        x[basis[b]] = 1.0
        for i, th in enumerate(ths):
            vh = orc.v_dagger_mul_vec(circ, th[b], tg[b])
            assert maxdiff(out[i][0][b], vh[gather]) < TOL and maxdiff(out[i][1][b], orc.grad_of_dot_product(circ, th[b], x, vh)) < TOL, (i, b)


def test_alternating_with_surrogate_eval_leaves_no_trace(monkeypatch):
    """objective_launch (virtual stage walked back), surrogate_eval (V^H by its stages, the virtual stage swept FORWARDS from (M_0, Y_0)
    into the same partial-R rows), objective_launch with new thetas: the last results are a fresh workspace's, bit for bit."""
    from aqc_research_amd.engine import BUF_X, BUF_Y

    circ, tile, B = _spin(14, "cx", 40), 12, 5
    n = circ.num_qubits
    tg, _, ths = _inputs(circ, tile, B)
    flips = np.array([0] + [1 << q for q in range(n)], dtype=np.int64)

    def prepared():
        ws = _ws(circ, B, tile, "route", monkeypatch)
        assert ws.virtual_backwalk() == 1
        ws.upload(BUF_Y, tg)
        ws.set_basis(BUF_X, 0)
        ws.gather_setup(flips)
        return ws

    def launch(ws, th):
        ws.set_thetas(th)
        ws.objective_launch(BUF_X)
        return ws.gather_fetch().copy(), ws.get_grads().copy()

    ws = prepared()
    first = launch(ws, ths[0])
    ws.surrogate_eval(np.ascontiguousarray(ths[1]), np.ones(B), np.zeros(B, dtype=np.int64), update_state=False)
    ws.set_basis(BUF_X, 0)
    last = launch(ws, ths[1])
    ws.close()
    fresh = prepared()
    first_fresh = launch(fresh, ths[0])
    fresh.close()
    fresh = prepared()
    last_fresh = launch(fresh, ths[1])
    fresh.close()
    assert np.array_equal(first[0], first_fresh[0]) and np.array_equal(first[1], first_fresh[1])
    assert np.array_equal(last[0], last_fresh[0]) and np.array_equal(last[1], last_fresh[1])
    x = np.zeros(1 << n, complex)
    x[0] = 1.0
    for b in (0, B - 1):
        vh = orc.v_dagger_mul_vec(circ, ths[1][b], tg[b])
        assert maxdiff(last[0][b], vh[flips]) < TOL and maxdiff(last[1][b], orc.grad_of_dot_product(circ, ths[1][b], x, vh)) < TOL, b
