"""GPU: objective by projection with the sweep's first stage walked BACK from (psi, C) (sweep_mfma_body<..., BACK>, csrc/aqc_backwalk.h).

The route applies where the evaluation goes by projection (AQC_PROJECTED_VDAG), the V^H plan mirrors the sweep plan and the tile size has
the backward form; V^H's last stage on the lhs tiles is then not launched, the sweep writes the Z tile, and the gather follows it.
Reference: V^H by its stages (AQC_PROJECTED_VDAG=0) to 1e-13 -- the bound the route tests hold every pair of routes to: the same sums
in another order, fp64 -- and the C oracle at the suite's TOL.  Shapes: the smallest at which each code path exists (persistent 2^12 form
with a pair, one and two items per persistent workgroup; one-wave 2^8 tiles with two virtual stages and no pair; four waves without the
persistent walk; the other entanglers; a 2nd-order Trotter ansatz)."""
import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests.helpers import TOL, maxdiff

pytestmark = pytest.mark.gpu

ROUTES = 1e-13


def _spin(n, ent, depth):
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    return ParametricCircuit(n, ent, create_ansatz_structure(n, "spin", "full", depth))


def _trotter(n, layers):
    from aqc_research_amd import TrotterAnsatz
    from aqc_research_amd.circuit_structures import make_trotter_like_circuit

    return TrotterAnsatz(n, make_trotter_like_circuit(n, layers), second_order=True)


# name: (circuit, tile, lanes, the route's tile launches run in pairs)
SHAPES = {
    "k12_pair": (lambda: _spin(14, "cx", 40), 12, 5, True),
    "k12_pair_two_items_per_workgroup": (lambda: _spin(14, "cx", 40), 12, 260, True),
    "k8_two_virtual_stages": (lambda: _spin(14, "cx", 24), 8, 5, False),
    "k10_four_waves": (lambda: _spin(13, "cx", 30), 10, 5, True),
    "k12_cz": (lambda: _spin(14, "cz", 40), 12, 5, True),
    "k12_cp": (lambda: _spin(14, "cp", 40), 12, 5, True),
    "trotter2_n12": (lambda: _trotter(12, 2), 10, 5, True),
}
MODES = {   # environment of a workspace
    "route": {},
    "stages": {"AQC_PROJECTED_VDAG": "0"},
    "singles": {"AQC_PROJECTED_PAIRS": "0"},   # the single launches of old: V^H's last stage writes the Z tile, the same walk stores nothing
    "own_vdag_plan": {"AQC_MIRROR_PLAN": "0"},
}
_KEYS = ("AQC_PROJECTED_VDAG", "AQC_PROJECTED_PAIRS", "AQC_MIRROR_PLAN")


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
    from aqc_research_amd._lib import K_APPLY, K_APPLY_LIST, K_APPLY_VIRTUAL, K_SWEEP_LIST

    return {name: ws.profile_get(k)[0] for name, k in (("apply", K_APPLY), ("apply_list", K_APPLY_LIST), ("apply_virtual", K_APPLY_VIRTUAL),
                                                        ("sweep_list", K_SWEEP_LIST))}


def _cases(n, tile, B):
    """(basis index per lane, gather set): index 0 with the flip states; one index on the tile's bits, different ones above it."""
    hi = n - tile
    zero = (np.zeros(B, dtype=np.int64), np.array([0] + [1 << q for q in range(n)], dtype=np.int64))
    shifted = (np.array([5 | ((b * 3) % (1 << hi)) << tile for b in range(B)], dtype=np.int64),
               np.array([5 | (f << tile) for f in sorted({0, 1, (1 << hi) - 1, 1 << (hi - 1)})], dtype=np.int64))
    return {"zero": zero, "shifted": shifted}


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
        for i, th in enumerate(ths):   # (with few lanes a gather rides in the gradient walk and the evaluation keeps V^H's stages: without it)
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


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_backward_walk_equals_the_stages_of_vdag_and_the_oracle(shape, monkeypatch):
    make, tile, B, pairs = SHAPES[shape]
    circ = make()
    n = circ.num_qubits
    rng = np.random.default_rng(4200 + n + tile + B)
    tg = np.stack([orc.rand_state(n, rng) for _ in range(min(B, 8))])
    tg = tg[np.arange(B) % len(tg)] * np.exp(1j * np.arange(B))[:, None]   # (many lanes: a few states, a phase per lane)
    tg2 = tg[::-1].copy()
    th8 = [np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(min(B, 8))]) for _ in range(2)]
    ths = [t[(np.arange(B) + 3 * i) % len(t)] + 1e-3 * np.arange(B)[:, None] for i, t in enumerate(th8)]
    cases = _cases(n, tile, B)
    res = {}
    for mode in MODES:
        if mode == "singles" and not pairs:
            continue
        ws = _ws(circ, B, tile, mode, monkeypatch)
        if mode == "route":
            info = ws.projected_info()
            assert info, "the shape was chosen for its route"
        res[mode] = _walk(ws, circ, tg, tg2, ths, cases)
        ws.close()

    # which route ran
    c = res["route"]["counts"]
    assert c["apply_list"] == (0 if pairs else 1) and c["apply_virtual"] >= 2 and c["sweep_list"] >= 1 and c["apply"] == 0, c
    if pairs:
        s = res["singles"]["counts"]
        assert s["apply_list"] == 2 and s["apply_virtual"] >= 2 and s["sweep_list"] == 1 and s["apply"] == 0, s
    o = res["own_vdag_plan"]["counts"]   # a V^H plan of its own: no tile lists at all, V^H by its stages over the whole register
    assert o["apply_list"] == 0 and o["apply_virtual"] == 0 and o["sweep_list"] == 0 and o["apply"] >= 1, o

    route = res["route"]
    lanes = sorted({0, B // 2, B - 1})
    for key, val in route.items():
        if key in ("counts", "z", "seq"):
            continue
        assert maxdiff(val[0], res["stages"][key][0]) < ROUTES and maxdiff(val[1], res["stages"][key][1]) < ROUTES, key
        assert maxdiff(val[0], res["own_vdag_plan"][key][0]) < TOL and maxdiff(val[1], res["own_vdag_plan"][key][1]) < TOL, key
        if pairs:   # pairs and single launches run the same body: not one bit apart
            assert np.array_equal(val[0], res["singles"][key][0]) and np.array_equal(val[1], res["singles"][key][1]), key
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
