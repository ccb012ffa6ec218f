"""GPU: every result-changing value of the run-time switches that select another kernel, launch geometry or plan for the same
mathematical result (include/aqc_switches.def) against the oracle, plus a host part (the planner under AQC_LOW_BITS, the guard that
every switch has a test or a reason).

One harness (``_evaluate``: V^H, both gradient ranges, the overlap, V back) and one helper for the one-call route (``_one_call``:
``eval(th, gather=True)`` twice, the second time with new thetas so that it replays the captured graph).  Every workspace is created
inside ``_env`` and asserts that ``ws.switch(NAME)`` reads back what was set, so no case can silently run the default.

Tolerances are the project's own: ``TOL`` against the oracle; ``np.array_equal`` against the default route where the switch is documented
not to change the kernels that run; routes that sum in another order (AQC_GRADS_DIRECT=0, AQC_MIRROR_PLAN=0, the persistent grids)
are held to the oracle only and print their difference to the default route (recorded in DESIGN.md, not asserted).

With three or more lanes the last lane's target is a normalised state times 2^40 and its results are scaled back (everything here is
linear in the target): a value that leaks between lanes or through a mask is 2^40 times too large to pass.
"""
import ast
import functools
import glob
import os
import re

import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests.helpers import FAMILIES, FAMILY_ENV, TOL, maxdiff
from tests.test_hip_fused_loads import _BIG, _CASES, _env, _run

gpu = pytest.mark.gpu

# every switch this module sets: unset unless a case says otherwise, whatever the caller's environment holds
_UNSET = {name: None for name in (
    "AQC_KERNEL_FAMILY", "AQC_KERNEL_V2", "AQC_LOW_BITS", "AQC_THREADS", "AQC_SWEEP_REG_BITS", "AQC_MIRROR_PLAN", "AQC_GRADS_DIRECT",
    "AQC_UBUILD_MIRROR", "AQC_APPLY_PERSIST", "AQC_SWEEP_GRID", "AQC_SPARSE_SWEEP", "AQC_SPARSE_MIN_ITEMS", "AQC_LAZY_Z", "AQC_PROJECTED",
    "AQC_PROJECTED_VDAG", "AQC_PROJECTED_VDAG_MIN_ELEMS", "AQC_PROJECTED_BEAM", "AQC_PROJECTED_FUSED", "AQC_PROJECTED_FUSED_WGS",
    "AQC_PROJECTED_FUSED_MAX_SHARES", "AQC_PROJECTED_PAIRS", "AQC_GRAPH", "AQC_TILE_BITS_APPLY", "AQC_TILE_BITS_SWEEP")}
_SMALL_ROUTES = {"AQC_SPARSE_MIN_ITEMS": "1", "AQC_PROJECTED_VDAG_MIN_ELEMS": "1"}   # the sparse / projected route at test sizes

# name -> (qubits, entangler or kind, blocks / layers): random pairs as in test_hip_parity_sv.CASES unless the kind names a structure
_CIRCUITS = {
    "n7cx": (7, "cx", 12), "n8cx": (8, "cx", 12), "n8cz": (8, "cz", 15), "n9cp": (9, "cp", 14), "n10cx": (10, "cx", 30),
    "n10cp": (10, "cp", 20), "n12cz": (12, "cz", 25), "n13cx": (13, "cx", 40), "n13cp": (13, "cp", 30), "n14cz": (14, "cz", 33),
    "trotter9": (9, "trotter2", 2), "spin12": (12, "spin", 20), "spin14": (14, "spin", 40),
}


@functools.lru_cache(maxsize=None)
def _circuit(name):
    from aqc_research_amd import ParametricCircuit, TrotterAnsatz
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    n, kind, depth = _CIRCUITS[name]
    if kind == "trotter2":
        return TrotterAnsatz(n, orc.trotter_blocks(n, depth), second_order=True)
    if kind == "spin":
        return ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", depth))
    rng = np.random.default_rng(100 * n + depth)
    blocks = np.stack([rng.permutation(n)[:2] for _ in range(depth)], axis=1).astype(np.int64)
    return ParametricCircuit(n, kind, blocks)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _scale(batch):
    """Per lane: what the lane's target is multiplied by on the device (the last of three or more lanes: 2^40)."""
    s = np.ones(batch)
    if batch >= 3:
        s[-1] = _BIG
    return s


def _partial_range(circ):
    return (1, max(2, circ.num_blocks // 2))


@functools.lru_cache(maxsize=None)
def _dense_data(name, batch, seed):
    """Thetas, lhs states, targets (unscaled) and the oracle's results of the harness: computed once per shape, never modified."""
    circ = _circuit(name)
    n = circ.num_qubits
    rng = np.random.default_rng(seed)
    th = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(batch)])
    x = np.stack([orc.rand_state(n, rng) for _ in range(batch)])
    y = np.stack([orc.rand_state(n, rng) for _ in range(batch)])
    z = np.stack([orc.v_dagger_mul_vec(circ, th[b], y[b]) for b in range(batch)])
    g_full = np.stack([orc.grad_of_dot_product(circ, th[b], x[b], z[b]) for b in range(batch)])
    g_part = np.stack([orc.grad_of_dot_product(circ, th[b], x[b], z[b], _partial_range(circ), False) for b in range(batch)])
    hs = np.array([np.vdot(x[b], z[b]) for b in range(batch)])
    return _frozen(th, x, y, z, g_full, g_part, hs)


def _assert_switches(ws, env):
    """Every create switch the case set reads back from the workspace as set (AQC_KERNEL_FAMILY: after AQC_KERNEL_V2 is folded in)."""
    for name, val in env.items():
        if val is not None:
            assert ws.switch(name) == int(val), (name, val, ws.switch(name))


def _evaluate(circ, batch, ka, ks, env, rng):
    """The harness.  ``circ``: a name of _CIRCUITS; ``rng``: the seed of the inputs (the same seed gives the same inputs, which is what
    a bit-for-bit comparison of two routes needs).  Creates the workspace inside ``_env(env)``, asserts the switches read back, runs
    V^H from Y into Z, the gradients for the full range and for one partial ``block_range`` with ``front_layer=False``, the overlap
    <X|Z> and V back from Z, and returns everything scaled back to the unscaled targets, with what the workspace says about itself."""
    from aqc_research_amd.engine import BUF_X, BUF_Y, BUF_Z, HipContext, Workspace

    c = _circuit(circ)
    th, x, y, *_ = _dense_data(circ, batch, rng)
    s = _scale(batch)
    full = dict(_UNSET)
    full.update(env)
    with _env(**full):
        ws = Workspace(HipContext(c), batch=batch, tile_bits_apply=ka, tile_bits_sweep=ks)
        try:
            _assert_switches(ws, env)
            out = {"family": ws.kernel_family(1), "family_name": ws.family_name(), "kernel": ws.sweep_kernel_name(),
                   "plans": {w: ws.plan_info(w) for w in (0, 1, 2)}, "projected": ws.projected_info()}
            ws.set_thetas(th)
            ws.upload(BUF_Y, y * s[:, None])
            ws.upload(BUF_X, x)
            ws.apply(True, BUF_Y, BUF_Z)
            out["z"] = ws.download(BUF_Z) / s[:, None]
            ws.grad(None, True)
            out["g_full"] = ws.get_grads() / s[:, None]
            ws.grad(_partial_range(c), False)
            out["g_part"] = ws.get_grads() / s[:, None]
            out["hs"] = ws.vdot(BUF_X, BUF_Z) / s
            ws.apply(False, BUF_Z, BUF_Y)
            out["y_back"] = ws.download(BUF_Y) / s[:, None]
            out["sparse"] = ws.sparse_counts()
        finally:
            ws.close()
    return out


_DENSE_KEYS = ("z", "g_full", "g_part", "hs", "y_back")


def _assert_dense_oracle(out, circ, batch, seed, what):
    _, _, y, z, g_full, g_part, hs = _dense_data(circ, batch, seed)
    errs = {k: maxdiff(out[k], ref) for k, ref in (("z", z), ("g_full", g_full), ("g_part", g_part), ("hs", hs), ("y_back", y))}
    print(f"{what} vs oracle: " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < TOL, (what, k, v)


def _assert_bit_equal(a, b, keys, what):
    for k in keys:
        assert np.array_equal(a[k], b[k]), (what, k, maxdiff(a[k], b[k]))


def _print_diff(a, b, keys, what):
    print(f"{what}: " + " ".join(f"{k} {maxdiff(a[k], b[k]):.3e}" for k in keys))


@functools.lru_cache(maxsize=None)
def _call_data(name, batch, seed):
    """One-call route: two theta sets, targets, a basis state per lane, the gather set, and per theta set the oracle's amplitudes and
    gradients (full range and the partial one), and V^H y of the second set."""
    circ = _circuit(name)
    n = circ.num_qubits
    rng = np.random.default_rng(seed)
    ths = np.stack([np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(batch)]) for _ in range(2)])
    y = np.stack([orc.rand_state(n, rng) for _ in range(batch)])
    basis = np.array([(5 + 37 * b) % (1 << n) if b else 0 for b in range(batch)], dtype=np.int64)
    flips = np.array([0] + [1 << q for q in range(n)], dtype=np.int64)
    amps, g_full, g_part, z = [], [], [], []
    for th in ths:
        for b in range(batch):
            vh = orc.v_dagger_mul_vec(circ, th[b], y[b])
            z.append(vh)
            x = np.zeros(1 << n, complex)
            x[basis[b]] = 1.0
            amps.append(vh[flips])
            g_full.append(orc.grad_of_dot_product(circ, th[b], x, vh))
            g_part.append(orc.grad_of_dot_product(circ, th[b], x, vh, _partial_range(circ), False))
    shape = (2, batch, -1)
    return _frozen(ths, y, basis, flips, np.array(amps).reshape(shape), np.array(g_full).reshape(shape), np.array(g_part).reshape(shape),
                   np.array(z[batch:]))


def _one_call(circ, batch, tile, env, rng, partial=False):
    """The one-call route: ``set_basis``, ``gather_setup``, then ``eval(th, gather=True)`` for two theta sets, so that the second call
    replays the graph the first one captured, then a download of all of Z (which the restricted and projected V^H complete on demand).
    Returns the amplitudes and gradients of both calls and Z (scaled back), ``sparse_counts()`` and ``projected_info()``: every case
    asserts from them which route it ran."""
    from aqc_research_amd.engine import BUF_X, BUF_Y, BUF_Z, HipContext, Workspace

    c = _circuit(circ)
    ths, y, basis, flips, *_ = _call_data(circ, batch, rng)
    s = _scale(batch)
    full = dict(_UNSET)
    full.update(env)
    with _env(**full):
        ws = Workspace(HipContext(c), batch=batch, tile_bits_apply=tile, tile_bits_sweep=tile)
        try:
            _assert_switches(ws, env)
            out = {"projected": ws.projected_info(), "plans": {w: ws.plan_info(w) for w in (0, 1, 2)}, "family": ws.kernel_family(1)}
            ws.upload(BUF_Y, y * s[:, None])
            ws.set_basis(BUF_X, basis)
            ws.gather_setup(flips)
            amps, grads = [], []
            for th in ths:
                hs, g = ws.eval(th, gather=True, block_range=_partial_range(c) if partial else None, front_layer=not partial)
                amps.append(hs / s[:, None])
                grads.append(g / s[:, None])
            out["amps"], out["grads"] = np.array(amps), np.array(grads)
            out["sparse"] = ws.sparse_counts()
            out["z"] = ws.download(BUF_Z) / s[:, None]
        finally:
            ws.close()
    return out


def _assert_call_oracle(out, circ, batch, seed, what, partial=False):
    _, _, _, _, amps, g_full, g_part, z = _call_data(circ, batch, seed)
    da, dg, dz = maxdiff(out["amps"], amps), maxdiff(out["grads"], g_part if partial else g_full), maxdiff(out["z"], z)
    print(f"{what} one call vs oracle: amplitudes {da:.3e} gradients {dg:.3e} Z {dz:.3e} sparse {out['sparse']} projected {bool(out['projected'])}")
    assert da < TOL and dg < TOL and dz < TOL, (what, da, dg, dz)


_DENSE_ROUTE = (-1, -1, -1)   # sparse_counts() of a workspace that never built a tile list


# ---- 1. AQC_THREADS -------------------------------------------------------------------------------------------------------------------
# (circuit, tiles, lanes): fewer pair groups than threads (idle waves must contribute exact zeros); five inner products per block;
# the largest dynamic LDS of the per-group sweep (2^11 tiles, 512 threads); thetas with two slots
_THREAD_SHAPES = [("n7cx", 4, 4, 1), ("n9cp", 6, 5, 2), ("n12cz", 11, 11, 1), ("trotter9", 6, 5, 1)]


@gpu
@pytest.mark.parametrize("threads", [64, 192, 320, 512])
@pytest.mark.parametrize("circ,ka,ks,batch", _THREAD_SHAPES)
def test_threads_of_the_per_group_kernels(circ, ka, ks, batch, threads):
    """AQC_THREADS on family 1: 1, 3, 5 and 8 waves in sweep_stage_kernel's row reduction (the default only ever gives 1, 2 or 4)."""
    out = _evaluate(circ, batch, ka, ks, {"AQC_KERNEL_FAMILY": "1", "AQC_THREADS": str(threads)}, 1100 + ka)
    assert out["family"] == 1 and out["kernel"] == "sweep_stage_kernel"
    assert out["plans"][1][1] == ks and out["plans"][0][1] == ka
    _assert_dense_oracle(out, circ, batch, 1100 + ka, f"{circ} AQC_THREADS={threads}")


@gpu
@pytest.mark.parametrize("family", ["register-blocked", "mfma"])
def test_threads_do_not_reach_the_other_families(family):
    """Families 2 and 3 size their workgroups from the tile: AQC_THREADS=192 changes no bit."""
    fam = {"AQC_KERNEL_FAMILY": FAMILY_ENV[family]}
    base = _evaluate("n9cp", 2, 6, 5, fam, 1200)
    out = _evaluate("n9cp", 2, 6, 5, dict(fam, AQC_THREADS="192"), 1200)
    assert out["family"] == int(FAMILY_ENV[family]) == base["family"]
    _assert_dense_oracle(out, "n9cp", 2, 1200, f"{family} AQC_THREADS=192")
    _assert_bit_equal(out, base, _DENSE_KEYS, family)


@gpu
@pytest.mark.parametrize("threads", [32, 100, 576])
def test_threads_out_of_range_are_refused_at_creation(threads):
    from aqc_research_amd.engine import HipContext, Workspace

    with _env(**dict(_UNSET, AQC_KERNEL_FAMILY="1", AQC_THREADS=str(threads))):
        with pytest.raises(RuntimeError, match="AQC_THREADS"):
            Workspace(HipContext(_circuit("n7cx")), batch=1, tile_bits_apply=4, tile_bits_sweep=4)


# ---- 2. AQC_SWEEP_REG_BITS ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("circ,ka,ks,batch", [("n10cx", 7, 7, 2), ("n13cx", 13, 12, 2), ("trotter9", 0, 0, 1)])
def test_register_blocked_sweep_with_three_register_bits(circ, ka, ks, batch):
    out = _evaluate(circ, batch, ka, ks, {"AQC_KERNEL_FAMILY": "2", "AQC_SWEEP_REG_BITS": "3"}, 2100 + ks)
    assert out["family"] == 2 and out["kernel"] == "sweep_stage_kernel2"
    _assert_dense_oracle(out, circ, batch, 2100 + ks, f"{circ} AQC_SWEEP_REG_BITS=3")
    base = _evaluate(circ, batch, ka, ks, {"AQC_KERNEL_FAMILY": "2"}, 2100 + ks)
    _assert_bit_equal(out, base, ("z", "y_back"), "V and V^H do not take the value")   # (they always run four register bits)
    _print_diff(out, base, ("g_full", "g_part"), f"{circ} AQC_SWEEP_REG_BITS=3 vs 4")


@gpu
def test_register_bits_other_than_three_mean_four():
    base = _evaluate("n10cx", 2, 7, 7, {"AQC_KERNEL_FAMILY": "2"}, 2200)
    out = _evaluate("n10cx", 2, 7, 7, {"AQC_KERNEL_FAMILY": "2", "AQC_SWEEP_REG_BITS": "5"}, 2200)
    _assert_dense_oracle(out, "n10cx", 2, 2200, "AQC_SWEEP_REG_BITS=5")
    _assert_bit_equal(out, base, _DENSE_KEYS, "AQC_SWEEP_REG_BITS=5")


# ---- 3. AQC_KERNEL_V2 -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("v2,family_env,want", [("0", None, 1), ("1", None, 2), ("0", "3", 3), ("1", "3", 3)])
def test_older_spelling_of_the_kernel_family(v2, family_env, want):
    """AQC_KERNEL_V2 = 0 / 1 is family 1 / 2 unless AQC_KERNEL_FAMILY is set, which wins; the same bits as the family's own spelling."""
    from aqc_research_amd.engine import Workspace

    env = {"AQC_KERNEL_V2": v2}
    if family_env:
        env["AQC_KERNEL_FAMILY"] = family_env
    out = _evaluate("n8cz", 3, 5, 6, env, 3100)
    assert out["family"] == want and (out["family_name"], out["kernel"]) == Workspace._FAMILIES[want]
    _assert_dense_oracle(out, "n8cz", 3, 3100, f"AQC_KERNEL_V2={v2} AQC_KERNEL_FAMILY={family_env}")
    same = _evaluate("n8cz", 3, 5, 6, {"AQC_KERNEL_FAMILY": str(want)}, 3100)
    assert same["family"] == want
    _assert_bit_equal(out, same, _DENSE_KEYS, f"family {want}")


@gpu
def test_older_spelling_reads_back_folded_into_the_family():
    from aqc_research_amd.engine import HipContext, Workspace

    with _env(**dict(_UNSET, AQC_KERNEL_V2="1")):
        ws = Workspace(HipContext(_circuit("n8cz")), batch=1)
        assert (ws.switch("AQC_KERNEL_V2"), ws.switch("AQC_KERNEL_FAMILY"), ws.kernel_family(1)) == (1, 2, 2)
        ws.close()


# ---- 4. AQC_LOW_BITS ------------------------------------------------------------------------------------------------------------------
_LOW_BITS = [0, 1, 2, 4, 9]


def _best_plan_stages(ctx, which, tile_bits, low_bits):
    """ws_decide's best_plan restated on the host planner: make_plan at ``low_bits``, then every fewer down to 2, a candidate winning
    only with strictly fewer stages."""
    best = len(ctx.plan(which, 1, tile_bits, low_bits))
    for lb in range(low_bits - 1, 1, -1):
        best = min(best, len(ctx.plan(which, 1, tile_bits, lb)))
    return best


@pytest.mark.parametrize("circ", ["n10cx", "n13cx", "trotter9"])
def test_planner_under_every_low_bits_value(circ):
    """Host only.  What make_plan guarantees for every value of ``low_bits`` (-1: the default 3; clamped to [0, k - 2]): a plan whose
    stages hold exactly min(k, n) address bits each, the forced low bits among them whenever the register is larger than the tile, and
    every gate group exactly once (aqc_plan_query also runs check_plan on it).  What it does NOT guarantee is monotony: fewer forced
    bits may give MORE stages (n10cx, sweep, 2^7 tiles: 6 stages at 2 forced bits, 5 at 3), and values below 2, which best_plan never
    tries, may give more stages than the default (n13cx, sweep, 2^10 tiles: 5 at 0 against 4).  What best_plan guarantees, and only for
    the values it searches (low_bits >= 3 includes the default's candidates 3 and 2): never more stages than the default's plan."""
    from aqc_research_amd.engine import HipContext

    c = _circuit(circ)
    ctx = HipContext(c)
    n = c.num_qubits
    for which in (0, 1, 2):
        for tile in (4, 7, 8, 10, 12):
            k = min(tile, n)
            stages = {}
            for lb in range(-1, 10):
                plan = ctx.plan(which, 1, tile, lb)
                assert plan, (which, tile, lb)
                forced = max(0, min(3 if lb < 0 else lb, k - 2))
                for bits, _ in plan:
                    assert len(bits) == k and sorted(set(bits)) == bits and bits[-1] < n, (which, tile, lb, bits)
                    assert n <= k or bits[:forced] == list(range(forced)), (which, tile, lb, bits)
                ops = [op for _, stage_ops in plan for op in stage_ops]
                assert sorted(ops) == list(range(ctx.num_gate_groups)), (which, tile, lb)
                stages[lb] = plan
            assert stages[-1] == stages[3]
            for lb in range(max(k - 2, 0), 10):
                assert stages[lb] == stages[max(k - 2, 0)], "values above k - 2 are clamped to it"
            default = _best_plan_stages(ctx, which, tile, 3)
            for lb in range(3, 10):
                assert _best_plan_stages(ctx, which, tile, lb) <= default, (which, tile, lb)


@gpu
@pytest.mark.parametrize("low_bits", _LOW_BITS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("circ,tile,batch", [("n10cx", 7, 2), ("n13cx", 10, 1)])
def test_low_bits_on_every_family(circ, tile, batch, family, low_bits):
    """Fewer forced low bits than best_plan's own search tries (0, 1), the default's neighbours and a value that clamps (9)."""
    from aqc_research_amd.engine import HipContext

    out = _evaluate(circ, batch, tile, tile, {"AQC_KERNEL_FAMILY": FAMILY_ENV[family], "AQC_LOW_BITS": str(low_bits)}, 4100 + tile)
    assert out["family"] == int(FAMILY_ENV[family])
    ctx = HipContext(_circuit(circ))
    for which in (1, 2):   # the workspace runs the plan best_plan picks for the value (sweep, V)
        nstages, k, _ = out["plans"][which]
        assert k == (max(tile, 8) if family == "mfma" else tile)
        assert nstages == _best_plan_stages(ctx, which, k, low_bits), (which, out["plans"])
    _assert_dense_oracle(out, circ, batch, 4100 + tile, f"{circ} {family} AQC_LOW_BITS={low_bits}")


@gpu
@pytest.mark.parametrize("low_bits", _LOW_BITS)
@pytest.mark.parametrize("circ", ["n10cx", "spin12"])
def test_low_bits_on_the_one_call_route(circ, low_bits):
    """Family 3, 2^8 tiles, the sparse route forced; spin12 is a shape whose later stages also run on the virtual register."""
    out = _one_call(circ, 3, 8, dict(_SMALL_ROUTES, AQC_KERNEL_FAMILY="3", AQC_LOW_BITS=str(low_bits)), 4300)
    assert out["family"] == 3
    if out["plans"][1][0] >= 2:
        assert out["sparse"][0] > 0, "the sparse route did not run"
    else:
        assert out["sparse"] == _DENSE_ROUTE and not out["projected"]
    if circ == "spin12":
        assert out["projected"], "the shape was chosen for the route by projection"
    _assert_call_oracle(out, circ, 3, 4300, f"{circ} AQC_LOW_BITS={low_bits}")


# ---- 5. AQC_MIRROR_PLAN=0 -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("circ,tile,batch", [("n10cx", 8, 2), ("n13cp", 12, 2), ("trotter9", 8, 1)])
def test_vdag_with_a_plan_of_its_own(circ, tile, batch):
    """Family 3, equal tiles, two stages or more: V^H by its own plan instead of the sweep's walked backwards.  AQC_UBUILD_MIRROR stays
    at its default: without the mirrored plan the sweep's U-builder jobs cannot write V^H's operands, so V^H must get jobs of its own
    (a V^H from stale or missing operands misses the oracle).  The sparse and projected routes are off, as the table promises."""
    env = dict(_SMALL_ROUTES, AQC_KERNEL_FAMILY="3", AQC_MIRROR_PLAN="0")
    out = _evaluate(circ, batch, tile, tile, env, 5100 + tile)
    assert out["family"] == 3 and out["plans"][1][0] >= 2 and out["plans"][0][1] == out["plans"][1][1] == tile
    assert not out["projected"] and out["sparse"] == _DENSE_ROUTE
    _assert_dense_oracle(out, circ, batch, 5100 + tile, f"{circ} AQC_MIRROR_PLAN=0")
    base = _evaluate(circ, batch, tile, tile, dict(_SMALL_ROUTES, AQC_KERNEL_FAMILY="3"), 5100 + tile)
    _print_diff(out, base, _DENSE_KEYS, f"{circ} tile {tile} AQC_MIRROR_PLAN=0 vs default")
    call = _one_call(circ, batch, tile, env, 5200 + tile)
    assert not call["projected"] and call["sparse"] == _DENSE_ROUTE
    _assert_call_oracle(call, circ, batch, 5200 + tile, f"{circ} AQC_MIRROR_PLAN=0")
    base = _one_call(circ, batch, tile, dict(_SMALL_ROUTES, AQC_KERNEL_FAMILY="3"), 5200 + tile)
    assert base["sparse"][0] > 0, "the default takes the sparse route here: the case compares two routes"
    _print_diff(call, base, ("amps", "grads"), f"{circ} tile {tile} one call AQC_MIRROR_PLAN=0 vs default")


# ---- 6. AQC_GRADS_DIRECT=0 ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("circ,tile,batch", [("n8cx", 8, 1), ("n10cp", 8, 3), ("n12cz", 10, 2)])
def test_gradients_through_the_partial_sums(circ, tile, batch):
    """Family 3, every theta with one slot: the gradient walk's partial sums and finalize_kernel instead of its direct write, for the
    full range, a partial range without the front layer (``from`` / ``to`` / ``front`` live in both), and the one-call route."""
    env = {"AQC_KERNEL_FAMILY": "3", "AQC_GRADS_DIRECT": "0"}
    out = _evaluate(circ, batch, tile, tile, env, 6100 + tile)
    assert out["family"] == 3
    _assert_dense_oracle(out, circ, batch, 6100 + tile, f"{circ} AQC_GRADS_DIRECT=0")
    base = _evaluate(circ, batch, tile, tile, {"AQC_KERNEL_FAMILY": "3"}, 6100 + tile)
    _assert_bit_equal(out, base, ("z", "hs", "y_back"), "only the gradients take the value")
    _print_diff(out, base, ("g_full", "g_part"), f"{circ} tile {tile} AQC_GRADS_DIRECT=0 vs default")
    for partial in (False, True):
        call = _one_call(circ, batch, tile, dict(_SMALL_ROUTES, **env), 6200 + tile, partial=partial)
        _assert_call_oracle(call, circ, batch, 6200 + tile, f"{circ} AQC_GRADS_DIRECT=0 partial={partial}", partial=partial)
        base = _one_call(circ, batch, tile, dict(_SMALL_ROUTES, AQC_KERNEL_FAMILY="3"), 6200 + tile, partial=partial)
        assert np.array_equal(call["amps"], base["amps"]) and call["sparse"] == base["sparse"]
        _print_diff(call, base, ("grads",), f"{circ} tile {tile} one call partial={partial} AQC_GRADS_DIRECT=0 vs default")


# ---- 7. AQC_APPLY_PERSIST -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("persist", ["1", "3", "0"])
def test_persistent_apply_grids(persist):
    """2^12 tiles, 10 (tile, lane) items, AQC_SWEEP_GRID=2 for a device of two compute units: 2 workgroups of five items, 6 of two or
    one, and -- AQC_APPLY_PERSIST=0 -- one item per workgroup, against the default's 4 workgroups of three or two."""
    env = {"AQC_KERNEL_FAMILY": "3", "AQC_SWEEP_GRID": "2", "AQC_APPLY_PERSIST": persist}
    out = _evaluate("n13cx", 5, 12, 12, env, 7100)
    assert out["family"] == 3 and out["plans"][0][1:] == (12, 2) and out["plans"][2][1:] == (12, 2)
    _assert_dense_oracle(out, "n13cx", 5, 7100, f"AQC_APPLY_PERSIST={persist}")
    base = _evaluate("n13cx", 5, 12, 12, {"AQC_KERNEL_FAMILY": "3", "AQC_SWEEP_GRID": "2"}, 7100)
    _print_diff(out, base, _DENSE_KEYS, f"n13cx AQC_APPLY_PERSIST={persist} vs 2")


@gpu
@pytest.mark.parametrize("persist", ["1", "3", "0"])
@pytest.mark.parametrize("circ", ["n14cz", "spin14"])
def test_persistent_list_launches_and_the_dense_route_without_them(circ, persist):
    """One-call evaluations on 2^12 tiles with the sparse route forced: list launches on persistent grids of 2 and 6 workgroups (spin14:
    the projected route's pair launches as well).  AQC_APPLY_PERSIST=0 has no list launches on 2^12 tiles, so the workspace takes the
    dense route (and plans no projected one) instead of failing inside the evaluation."""
    env = dict(_SMALL_ROUTES, AQC_KERNEL_FAMILY="3", AQC_SWEEP_GRID="2", AQC_APPLY_PERSIST=persist)
    out = _one_call(circ, 3, 12, env, 7200)
    assert out["plans"][1][1] == 12 and out["plans"][1][0] >= 2
    if persist == "0":
        assert out["sparse"] == _DENSE_ROUTE and not out["projected"]
    else:
        assert out["sparse"][0] > 0, "the sparse route did not run"
        assert bool(out["projected"]) == (circ == "spin14")
    _assert_call_oracle(out, circ, 3, 7200, f"{circ} AQC_APPLY_PERSIST={persist}")


def test_no_projected_route_is_planned_without_list_launches():
    """Host only: the planner's answer for 2^12 tiles follows AQC_APPLY_PERSIST, smaller tiles do not depend on it."""
    from aqc_research_amd.engine import HipContext

    ctx = HipContext(_circuit("spin14"))
    with _env(**dict(_UNSET, AQC_APPLY_PERSIST="0")):
        assert ctx.plan_projected(12) == {}
        small = ctx.plan_projected(10)
    with _env(**_UNSET):
        assert ctx.plan_projected(12)["tile_bits"] == 12
        assert ctx.plan_projected(10) == small


@gpu
@pytest.mark.parametrize("circ,tile", [("n10cx", 8), ("spin12", 8), ("spin14", 12)])
def test_vdag_writes_all_of_z_without_lazy_z(circ, tile):
    """AQC_LAZY_Z=0 (no test set it before this one): the sparse route keeps its sweep, V^H runs every stage over every tile -- no
    restricted last stage, so no V^H item list -- and the results, Z included, are the oracle's."""
    env = dict(_SMALL_ROUTES, AQC_KERNEL_FAMILY="3", AQC_LAZY_Z="0")
    out = _one_call(circ, 3, tile, env, 7300 + tile)
    assert out["sparse"][0] > 0 and out["sparse"][2] == -1, out["sparse"]
    _assert_call_oracle(out, circ, 3, 7300 + tile, f"{circ} AQC_LAZY_Z=0")
    base = _one_call(circ, 3, tile, dict(_SMALL_ROUTES, AQC_KERNEL_FAMILY="3"), 7300 + tile)
    assert base["sparse"][0] > 0
    _print_diff(out, base, ("amps", "grads", "z"), f"{circ} tile {tile} AQC_LAZY_Z=0 vs default")


# ---- 8. AQC_PROJECTED_BEAM, AQC_PROJECTED_FUSED_WGS -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fused_case(case):
    """The inputs of tests.test_hip_fused_loads._check for a shape of its _CASES (lane 2's target times 2^40) and the oracle's
    amplitudes and gradients of lanes 1 and 2."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    n, blocks, tile, _, _ = _CASES[case]
    rng = np.random.default_rng(4200 + 100 * n + blocks)
    circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", blocks))
    th = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(3)])
    tg = np.stack([orc.rand_state(n, rng) for _ in range(3)])
    tg[2] *= _BIG
    scale = np.array([1.0, 1.0, 1.0 / _BIG])[:, None]
    flips = np.array([0] + [1 << q for q in range(n)], dtype=np.int64)
    x = np.zeros(1 << n, complex)
    x[0] = 1.0
    ref = {}
    for b in (1, 2):
        vh = orc.v_dagger_mul_vec(circ, th[b], tg[b] * scale[b, 0])
        ref[b] = _frozen(vh[flips], orc.grad_of_dot_product(circ, th[b], x, vh))
    _frozen(th, tg, scale, flips)
    return circ, tile, th, tg, scale, flips, ref


def _fused_run(case, what, **route):
    """``_run`` of test_hip_fused_loads under ``route``; the switches are read back from a workspace of the same environment (``_run``
    closes its own).  Returns projected_info and (amplitudes, gradients) scaled back, after holding lanes 1 and 2 to the oracle."""
    from aqc_research_amd.engine import HipContext, Workspace

    circ, tile, th, tg, scale, flips, ref = _fused_case(case)
    info, (amps, grads) = _run(circ, tile, th, tg, flips, **route)
    with _env(**dict({"AQC_PROJECTED_FUSED": None, "AQC_PROJECTED_VDAG": None, "AQC_PROJECTED_FUSED_MAX_SHARES": None}, **route)):
        ws = Workspace(HipContext.of(circ), batch=1, tile_bits_apply=tile, tile_bits_sweep=tile)
        _assert_switches(ws, route)
        ws.close()
        assert info == HipContext.of(circ).plan_projected(tile), "the workspace took or declined the route as the planner says"
    amps, grads = amps * scale, grads * scale
    for b in (1, 2):
        da, dg = maxdiff(amps[b], ref[b][0]), maxdiff(grads[b], ref[b][1])
        print(f"{case} {what} lane {b} vs oracle: amplitudes {da:.3e} gradients {dg:.3e}")
        assert da < TOL and dg < TOL, (case, what, b)
    return info, (amps, grads)


@gpu
@pytest.mark.parametrize("beam", ["1", "2", "64"])
@pytest.mark.parametrize("case", ["uvalid_mask", "split_walk"])
def test_beam_width_of_the_virtual_plan(case, beam):
    """A narrower or wider sub-stage search may change the virtual plan (or make the route decline): either way the results are the
    oracle's, and the workspace's answer is the host planner's under the same value."""
    info, _ = _fused_run(case, f"AQC_PROJECTED_BEAM={beam}", AQC_PROJECTED_BEAM=beam)
    base = _fused_run(case, "default", AQC_PROJECTED_BEAM=None)[0]
    print(f"{case} AQC_PROJECTED_BEAM={beam}: sub-stages {info.get('substages_per_stage')} (default {base.get('substages_per_stage')})")
    assert base, "the shape was chosen for the route by projection"


@gpu
@pytest.mark.parametrize("wgs", ["1", "4", "100000"])
@pytest.mark.parametrize("case", ["uvalid_mask", "split_walk"])
def test_workgroup_target_of_the_fused_pass(case, wgs):
    """AQC_PROJECTED_FUSED_WGS sizes the split of the fused pass's walk: 1 never splits (the bits of AQC_PROJECTED_FUSED_MAX_SHARES=1),
    4 splits once (3 lanes), 100000 up to the cap."""
    info, got = _fused_run(case, f"AQC_PROJECTED_FUSED_WGS={wgs}", AQC_PROJECTED_FUSED_WGS=wgs)
    assert info, "the shape was chosen for the route by projection"
    whole = _fused_run(case, "AQC_PROJECTED_FUSED_MAX_SHARES=1", AQC_PROJECTED_FUSED_MAX_SHARES="1")[1]
    if wgs == "1":
        assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    else:
        print(f"{case} AQC_PROJECTED_FUSED_WGS={wgs} vs unsplit: amplitudes {maxdiff(got[0], whole[0]):.3e} gradients {maxdiff(got[1], whole[1]):.3e}")


# ---- 9. AQC_LOCKSTEP_SURROGATE_EVAL -----------------------------------------------------------------------------------------------------
def _lockstep_scenario():
    """The scenario of test_hip_lockstep.test_lockstep_objects_with_leading_flip_states: per lane the largest error of values, gradients,
    weights and leading states against orc.SurMaxOracle, and the batch's native calls."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.engine import BUF_X2
    from aqc_research_amd.lockstep import LockstepBatch
    from aqc_research_amd.model_sp_lhs.objective_lhs_sur_max import SpSurrogateObjectiveMax

    n, lanes = 9, 4
    rng = np.random.default_rng(99)
    a = orc.Ansatz(n, "cx", orc.spin_blocks(n, 11))
    circ = ParametricCircuit(n, "cx", a.blocks)
    batch = LockstepBatch(circ, nlanes=lanes)
    idx = orc.flip_state_indices(n, 1)
    data = [(orc.rand_state(n, rng), orc.rand_thetas(a.num_thetas, rng)) for _ in range(lanes)]

    def job(view, lane):
        y, th = data[lane]
        user = dict(num_qubits=n, max_flips=1, state_prep_func=lambda _n: 0, enable_optim_stats=False, verbose=0, workspace=view)
        obj = SpSurrogateObjectiveMax(user_parameters=user, circ=circ, front_layer=True)
        obj.set_target(y)
        o = orc.SurMaxOracle(a, y, 1, None, True)
        errs = []
        for _ in range(2 + lane):
            f, fo = obj.objective(th), o.objective(th)
            g, go = obj.gradient(th), o.gradient(th)
            errs += [abs(f - fo), maxdiff(g, go), abs(obj._weight - o.weight), float(obj._max_no != o.max_no)]
            if lane == 1:   # somebody else's request on the lhs buffer between two pairs
                view.set_basis(BUF_X2, int(idx[2]))
                _, g2 = view.eval(None, vdag=False, gather=False, grad=True, x_buf=BUF_X2, block_range=None, front_layer=True)
                x2 = np.zeros(1 << n, complex)
                x2[idx[2]] = 1
                errs.append(maxdiff(g2[0], orc.grad_of_dot_product(a, th, x2, orc.v_dagger_mul_vec(a, th, y))))
            th = th - 0.05 * g
        return max(errs)

    out = batch.run([(lambda view, lane=lane: job(view, lane)) for lane in range(lanes)])
    batch.close()
    return out, batch.native_calls


@gpu
def test_lockstep_per_call_requests_in_the_same_process():
    """AQC_LOCKSTEP_SURROGATE_EVAL is read by the lane that asks, not when the module is imported: =0 and unset in one process both meet
    the oracle, and the per-call requests really ran (more native calls for the same rounds of work)."""
    calls = {}
    for value in ("0", None):
        with _env(**dict(_UNSET, AQC_LOCKSTEP_SURROGATE_EVAL=value)):
            errs, calls[value] = _lockstep_scenario()
        for e in errs:
            assert not isinstance(e, BaseException), e
            assert e < TOL, (value, e)
    print(f"native calls: per-call requests {calls['0']}, one call per round {calls[None]}")
    assert calls["0"] > calls[None]


def test_lockstep_switch_is_read_per_call():
    """Host only: a lane's preference follows the environment at the time it is asked."""
    from aqc_research_amd.lockstep import LaneView

    view = LaneView.__new__(LaneView)
    with _env(AQC_LOCKSTEP_SURROGATE_EVAL="0"):
        assert view.prefers_surrogate_eval is False
    with _env(AQC_LOCKSTEP_SURROGATE_EVAL=None):
        assert view.prefers_surrogate_eval is True
    with _env(AQC_LOCKSTEP_SURROGATE_EVAL="1"):
        assert view.prefers_surrogate_eval is True


# ---- the guard: every switch has a test that sets it, or a reason why it has no result to check -------------------------------------------
_HERE = "test_hip_switch_routes.py"
# switch -> "module::test function" (the function, or a helper or fixture of its module that it uses, names the switch and sets it to
# something other than its default) or a sentence that is no such reference: why there is no result to hold to the oracle
SWITCH_COVERAGE = {
    "AQC_KERNEL_FAMILY": "test_hip_parity_sv.py::test_oracle_multistage_batched",
    "AQC_KERNEL_V2": _HERE + "::test_older_spelling_of_the_kernel_family",
    "AQC_LOW_BITS": _HERE + "::test_low_bits_on_every_family",
    "AQC_TILE_BITS_APPLY": "test_hip_round5.py::test_device_lbfgs_on_the_sparse_route",
    "AQC_TILE_BITS_SWEEP": "test_hip_round5.py::test_device_lbfgs_on_the_sparse_route",
    "AQC_THREADS": _HERE + "::test_threads_of_the_per_group_kernels",
    "AQC_SWEEP_REG_BITS": _HERE + "::test_register_blocked_sweep_with_three_register_bits",
    "AQC_MIRROR_PLAN": _HERE + "::test_vdag_with_a_plan_of_its_own",
    "AQC_VERBOSE": "diagnostics on stderr only; no result depends on it",
    "AQC_SPARSE_SWEEP": "test_hip_round5.py::test_sparse_route_equals_dense_route_and_oracle",
    "AQC_SPARSE_MIN_ITEMS": "test_hip_round5.py::test_device_lbfgs_on_the_sparse_route",
    "AQC_LAZY_Z": _HERE + "::test_vdag_writes_all_of_z_without_lazy_z",
    "AQC_R_ONLY_LAST": "test_hip_round5.py::test_r_only_last_substage_equals_full_sweep_and_oracle",
    "AQC_R_ONLY_MAX_SUBS": "test_hip_round5.py::test_r_only_last_substage_equals_full_sweep_and_oracle",
    "AQC_SKIP_ZERO_W": "test_hip_round5.py::test_zero_groups_of_w_are_skipped_without_changing_a_bit",
    "AQC_GRADS_DIRECT": _HERE + "::test_gradients_through_the_partial_sums",
    "AQC_UBUILD_MIRROR": "test_hip_ubuild_subset.py::test_subset_equals_everything_and_the_oracle",
    "AQC_UBUILD_SUBSET": "test_hip_ubuild_subset.py::test_subset_equals_everything_and_the_oracle",
    "AQC_PROJECTED": "test_hip_round5.py::test_projected_route_equals_full_size_sweep_and_oracle",
    "AQC_PROJECTED_BEAM": _HERE + "::test_beam_width_of_the_virtual_plan",
    "AQC_PROJECTED_VDAG": "test_hip_round5.py::test_objective_launch_leaves_partial_z_that_readers_complete",
    "AQC_PROJECTED_VDAG_MIN_ELEMS": "test_hip_round5.py::test_objective_by_projection_equals_the_stages_of_vdag",
    "AQC_PROJECTED_FUSED": "test_hip_round5.py::test_fused_pass_equals_the_two_launches",
    "AQC_PROJECTED_FUSED_WGS": _HERE + "::test_workgroup_target_of_the_fused_pass",
    "AQC_PROJECTED_FUSED_MAX_SHARES": "test_hip_round5.py::test_fused_pass_equals_the_two_launches",
    "AQC_PROJECTED_FUSED_QB": "test_hip_fused_loads.py::test_fused_pass_with_four_blocks_per_wave",
    "AQC_PROJECTED_PAIRS": "test_hip_pairs.py::test_pairs_equal_the_single_launches",
    "AQC_GRAPH": "test_hip_switches.py::test_switches_belong_to_the_workspace",
    "AQC_SWEEP_GRID": _HERE + "::test_persistent_apply_grids",
    "AQC_APPLY_PERSIST": _HERE + "::test_persistent_apply_grids",
    "AQC_STAMPS": "tuning builds only (-DAQC_TUNING): timing stamps on stderr, the library the suite builds ignores it",
    "AQC_DEBUG_SKIP": "tuning builds only (-DAQC_TUNING): skips work on purpose, its results are wrong by design",
    "AQC_CD_CHAIN": "test_hip_round4.py::test_coordinate_descent_one_launch_lanes_and_sweeps",
    "AQC_SVD_BLOCKED": "test_hip_mps_engine.py::test_blocked_jacobi_agrees_with_round_per_launch",
    "AQC_SVD_DEBUG": "tuning builds only (-DAQC_TUNING): a debug word for timing experiments, its results are wrong by design",
    "AQC_DEVICE": "names the device, not a route: every device computes the same, and the suite runs on one",
    "AQC_COMM_TIMEOUT_S": "a time limit of the collectives: it bounds a wait, no result depends on it",
    "AQC_COMM_INIT_TIMEOUT_S": "a time limit of the communicator's creation: it bounds a wait, no result depends on it",
    "AQC_HIP_LIB": "names the library file to load (tuning and experiment builds), not a route inside it",
    "AQC_MPS_APPLY": "test_hip_mps_engine.py::test_reference_signature_functions_route_to_the_engine",
    "AQC_MPS_METHOD": "test_hip_mps_state_prep.py::test_objective_mps_route_matches_dense_route",
    "AQC_LOCKSTEP_SURROGATE_EVAL": _HERE + "::test_lockstep_per_call_requests_in_the_same_process",
    "AQC_COMM_FILE": "names the rendezvous file of the ranks: where the id travels, no result depends on it",
    "AQC_COMM_TAG": "names the launch inside the rendezvous file: it tells launches apart, no result depends on it",
}
_REASON_ONLY = {"AQC_VERBOSE", "AQC_STAMPS", "AQC_DEBUG_SKIP", "AQC_SVD_DEBUG", "AQC_HIP_LIB", "AQC_DEVICE", "AQC_COMM_TIMEOUT_S",
                "AQC_COMM_INIT_TIMEOUT_S", "AQC_COMM_FILE", "AQC_COMM_TAG"}


def _mentions(module_path, function, switch):
    """Whether ``function`` of the module, or a module-level function (helper, fixture) it uses by name -- autouse fixtures always --
    names ``switch``."""
    src = open(module_path).read()
    tree = ast.parse(src)
    defs = {node.name: node for node in tree.body if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef))}
    if function not in defs:
        return None
    autouse = [name for name, node in defs.items() if any("autouse=True" in ast.get_source_segment(src, d) for d in node.decorator_list)]
    seen, todo = set(), [function] + autouse
    while todo:
        name = todo.pop()
        if name in seen:
            continue
        seen.add(name)
        node = defs[name]
        text = ast.get_source_segment(src, node)
        if re.search(r"\b" + switch + r"\b", text):
            return True
        used = {n.id for n in ast.walk(node) if isinstance(n, ast.Name)} | {a.arg for a in node.args.args}
        todo += [u for u in used if u in defs]
    return False


def test_every_switch_has_a_test_or_a_reason():
    from aqc_research_amd.switches import table

    names = [row["name"] for row in table()]
    assert len(names) == len(set(names)) >= 44
    missing = sorted(set(names) - set(SWITCH_COVERAGE))
    assert not missing, f"switches without a test or a reason: {missing}"
    assert not sorted(set(SWITCH_COVERAGE) - set(names)), "entries for switches the table no longer has"
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    modules = {os.path.basename(p) for p in glob.glob(os.path.join(tests_dir, "test_*.py"))}
    for name, entry in SWITCH_COVERAGE.items():
        if "::" in entry:
            assert name not in _REASON_ONLY
            module, function = entry.split("::")
            assert module in modules and function.startswith("test_"), (name, entry)
            found = _mentions(os.path.join(tests_dir, module), function, name)
            assert found is not None, f"{name}: {entry} does not exist"
            assert found, f"{name}: {entry} does not mention the switch"
        else:
            assert name in _REASON_ONLY and len(entry.split()) >= 5 and "\n" not in entry, (name, entry)
