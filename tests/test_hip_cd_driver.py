"""Coordinate-descent AQC driver on the device (aqc_ws_cd_minimize, model_sketching.aqc_coord_descent): the wide walk for operands that
do not fit LDS against the oracle's sweep, the two routes against each other, lanes against solo runs bit for bit, and the stop rules
of aqc_coord_descent.py:70-101 against that loop written out over the oracle's sweep."""
import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests.helpers import TOL, maxdiff

pytestmark = pytest.mark.gpu
R10 = float(np.sqrt(10.0))


def _spin_problem(n, ent, seed):
    """The problem of test_hip_round4's single-step test: spin layout, 12 blocks, a random unitary target."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    rng = np.random.default_rng(seed)
    circ = ParametricCircuit(n, ent, create_ansatz_structure(n, "spin", "full", 12))
    d = 1 << n
    u = np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0]
    return circ, orc.rand_thetas(circ.num_thetas, rng), np.ascontiguousarray(u)


def _pairs_circuit(n, depth, seed, ent="cx"):
    """`depth` blocks on random qubit pairs: control above and below the target, neighbours and not."""
    from aqc_research_amd import ParametricCircuit

    rng = np.random.default_rng(seed)
    pairs = []
    while len(pairs) < depth:
        c, t = (int(v) for v in rng.integers(0, n, 2))
        if c != t:
            pairs.append((c, t))
    return ParametricCircuit(n, ent, np.array(pairs, dtype=np.int64).T)


def _minimize(circ, thetas, targets, maxiter, **kw):
    """Workspace.cd_minimize on a workspace of its own: thetas (lanes, T), targets (lanes, d, d)."""
    from aqc_research_amd.engine import BUF_Y, HipContext, Workspace

    th = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
    d = circ.dimension
    ws = Workspace(HipContext.of(circ), batch=th.shape[0], ncols=d)
    try:
        ws.upload(BUF_Y, np.ascontiguousarray(np.broadcast_to(targets, (th.shape[0], d, d))))
        kw.setdefault("fobj_thr", 0.0)
        kw.setdefault("dtheta_thr", 0.0)
        return ws.cd_minimize(th, maxiter, **kw)
    finally:
        ws.close()


@pytest.mark.parametrize("n,ent,steps", [(7, "cx", 1), (7, "cx", 2), (7, "cx", 5), (7, "cx", 17), (7, "cz", 19), (8, "cx", 3), (3, "cx", 12), (2, "cz", 7)])
def test_wide_walk_single_steps_at_the_north_star_tolerance(n, ent, steps):
    """The wide walk stopped after a few parameter updates (openers, steps, the partial sums handed from launch to launch) agrees with
    the oracle to 1e-10 on every theta and on the objective.  3 and 2 qubits are forced onto the wide route: fewer 4-element groups
    than one wave has lanes, and the front segment's second address bit wraps round to qubit 0."""
    circ, th, u = _spin_problem(n, ent, 500 + 10 * n + steps)
    ref, f_ref = orc.coord_descent_single_sweep(circ, th, u, max_steps=steps)
    assert int((np.abs(ref - th) > 0).sum()) == steps
    res = _minimize(circ, th, u, 1, route="wide", max_steps=steps)
    assert res["nit"][0] == 1 and res["status"][0] == 1                 # one sweep = maxiter: normal
    print("max |dtheta|", maxdiff(res["thetas"][0], ref), "|df|", abs(res["cost"][0] - f_ref))
    assert maxdiff(res["thetas"][0], ref) < TOL and abs(res["cost"][0] - f_ref) < TOL and res["profile"][0, 0] == res["cost"][0]


@pytest.fixture(scope="module")
def lanes7():
    """7 qubits, 3 lanes with their own thetas and targets, 10 blocks on random pairs; the oracle's two consecutive sweeps."""
    n, lanes = 7, 3
    circ = _pairs_circuit(n, 10, 91)
    b = circ.blocks
    assert (b[0] > b[1]).any() and (b[0] < b[1]).any() and (np.abs(b[0] - b[1]) > 1).any()
    rng = np.random.default_rng(92)
    d = 1 << n
    ths = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(lanes)])
    us = np.stack([np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0] for _ in range(lanes)])
    ref = []
    for k in range(lanes):
        t1, f1 = orc.coord_descent_single_sweep(circ, ths[k], us[k])
        t2, f2 = orc.coord_descent_single_sweep(circ, t1, us[k])
        ref.append((t1, f1, t2, f2))
    return circ, ths, us, ref


def test_wide_walk_whole_sweeps_with_lanes(lanes7):
    """Two sweeps of every lane follow the oracle's consecutive sweeps within the bounds of
    test_coordinate_descent_one_launch_lanes_and_sweeps (rounding is amplified along ~T sequential steps): 1e-8 / 1e-7."""
    circ, ths, us, ref = lanes7
    res = _minimize(circ, ths, us, 2, route="wide", chunk=2)
    for k, (t1, f1, t2, f2) in enumerate(ref):
        assert f2 < f1 < 1.0
        print(k, abs(res["profile"][k, 0] - f1), abs(res["profile"][k, 1] - f2), maxdiff(res["thetas"][k], t2))
        assert abs(res["profile"][k, 0] - f1) < 1e-8 and abs(res["profile"][k, 1] - f2) < 1e-7 and maxdiff(res["thetas"][k], t2) < 1e-7
        assert res["cost"][k] == res["profile"][k, 1] and res["nit"][k] == 2 and res["status"][k] == 1


def test_wide_lane_of_a_batch_equals_the_solo_run_and_a_repeat_bit_for_bit(lanes7):
    circ, ths, us, _ = lanes7
    a = _minimize(circ, ths, us, 2, route="wide")
    b = _minimize(circ, ths, us, 2, route="wide")
    solo = _minimize(circ, ths[1], us[1], 2, route="wide")
    for key in ("thetas", "cost", "nit", "status", "profile"):
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a[key][1], solo[key][0]), key


def test_single_sweep_beyond_lds_is_one_sweep_of_the_wide_walk(lanes7):
    """coord_descent_single_sweep at 7 qubits (no persistent launch) twice in a row follows the oracle's consecutive sweeps within the
    whole-sweep bounds above, and its first call is cd_minimize(maxiter=1, route="wide", thresholds off) on a one-lane workspace bit
    for bit: the call is that one by construction."""
    from aqc_research_amd.core_op_matrix import coord_descent_single_sweep

    circ, ths, us, ref = lanes7
    t1, f1, t2, f2 = ref[0]
    th = ths[0].copy()
    g1 = coord_descent_single_sweep(circ, th, us[0], None)
    first = th.copy()
    g2 = coord_descent_single_sweep(circ, th, us[0], None)
    print(abs(g1 - f1), abs(g2 - f2), maxdiff(th, t2))
    assert abs(g1 - f1) < 1e-8 and abs(g2 - f2) < 1e-7 and maxdiff(th, t2) < 1e-7
    assert f2 < f1 < 1.0
    res = _minimize(circ, ths[0], us[0], 1, route="wide", fobj_thr=0, dtheta_thr=0)
    assert np.array_equal(first, res["thetas"][0]) and g1 == res["profile"][0, 0]


def test_workspace_follows_the_thetas_a_wide_sweep_left(lanes7):
    """The close kernel writes the sweep's thetas over the workspace's own on the device, and the driver announces them when it returns:
    a V^H asked of the workspace afterwards, with no set_thetas in between, is V(thetas after the sweep)^H, with nothing in it that was
    built for the thetas at the sweep's start."""
    from aqc_research_amd.engine import BUF_Y, BUF_Z, HipContext, Workspace

    circ, ths, us, _ = lanes7
    ws = Workspace(HipContext.of(circ), batch=1, ncols=circ.dimension)
    try:
        ws.upload(BUF_Y, us[:1])
        res = ws.cd_minimize(ths[:1], 1, route="wide", fobj_thr=0.0, dtheta_thr=0.0)
        ws.apply(True, BUF_Y, BUF_Z)
        z = ws.download(BUF_Z)[0]
    finally:
        ws.close()
    assert maxdiff(z, orc.v_dagger_mul_mat(circ, res["thetas"][0], us[0])) < TOL


def test_single_sweep_refusals(lanes7):
    """aqc_ws_cd_sweep keeps its contract beyond LDS: one lane, cx / cz, a square workspace."""
    from aqc_research_amd import ParametricCircuit, _lib
    from aqc_research_amd.core_op_matrix import coord_descent_single_sweep
    from aqc_research_amd.engine import BUF_Y, HipContext, Workspace, live_buffers

    circ, ths, us, _ = lanes7
    d = circ.dimension
    before = live_buffers()
    fobj = np.zeros(1)
    for batch, ncols, msg in ((2, d, "single-lane workspace"), (1, d // 2, "square workspace")):
        ws = Workspace(HipContext.of(circ), batch=batch, ncols=ncols)
        try:
            ws.upload(BUF_Y, np.ascontiguousarray(np.broadcast_to(us[0][:, :ncols], (batch, d, ncols))))
            th = ths[0].copy()
            with pytest.raises(RuntimeError, match=msg):
                _lib.check(ws._L.aqc_ws_cd_sweep(ws.handle, _lib.dptr(th), _lib.dptr(fobj)))
            assert np.array_equal(th, ths[0])
        finally:
            ws.close()
    assert live_buffers() == before
    cp = ParametricCircuit(7, "cp", circ.blocks)
    with pytest.raises(NotImplementedError, match="CPhase"):
        coord_descent_single_sweep(cp, ths[0].copy(), us[0], None)
    ws = Workspace(HipContext.of(cp), batch=1, ncols=d)
    try:
        ws.upload(BUF_Y, us[:1])
        with pytest.raises(RuntimeError, match="CPhase"):
            _lib.check(ws._L.aqc_ws_cd_sweep(ws.handle, _lib.dptr(ths[0].copy()), _lib.dptr(fobj)))
    finally:
        ws.close()
    assert live_buffers() == before


@pytest.fixture(scope="module")
def lanes5():
    n, lanes = 5, 3
    circ = _pairs_circuit(n, 10, 93)
    rng = np.random.default_rng(94)
    d = 1 << n
    ths = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(lanes)])
    us = np.stack([np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0] for _ in range(lanes)])
    return circ, ths, us


def test_routes_agree_on_five_qubits(lanes5):
    """One sweep, the wide walk forced where the persistent launch would do: 1e-8, the bound of a whole sweep against the oracle."""
    circ, ths, us = lanes5
    p = _minimize(circ, ths, us, 1, route="persistent")
    w = _minimize(circ, ths, us, 1, route="wide")
    auto = _minimize(circ, ths, us, 1)
    print(maxdiff(p["thetas"], w["thetas"]), maxdiff(p["cost"], w["cost"]))
    assert maxdiff(p["thetas"], w["thetas"]) < 1e-8 and maxdiff(p["cost"], w["cost"]) < 1e-8
    assert all(np.array_equal(auto[k], p[k]) for k in p)                 # auto = persistent where it fits
    t1, f1 = orc.coord_descent_single_sweep(circ, ths[0], us[0])
    assert abs(p["cost"][0] - f1) < 1e-8 and maxdiff(p["thetas"][0], t1) < 1e-8


def test_persistent_lane_of_a_batch_equals_the_solo_run_and_a_repeat_bit_for_bit(lanes5):
    from aqc_research_amd.core_op_matrix import coord_descent_sweeps

    circ, ths, us = lanes5
    a = _minimize(circ, ths, us, 3, route="persistent", chunk=2)
    b = _minimize(circ, ths, us, 3, route="persistent", chunk=2)
    solo = _minimize(circ, ths[2], us[2], 3, route="persistent", chunk=2)
    for key in ("thetas", "cost", "nit", "status", "profile"):
        assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a[key][2], solo[key][0]), key
    plain = ths.copy()                                                   # the kernel without the rule: the same sweeps
    f = coord_descent_sweeps(circ, plain, us, 3)
    assert np.array_equal(f, a["profile"])


# ---- stop rules ---------------------------------------------------------------------------------------------------------------
# Lanes: targets V(theta*) and starts theta* + noise, drawn from default_rng([base, index]).  The indices below were chosen on the CPU,
# with the oracle alone, among draws at noise 1e-5: lane "B" loses a factor >= 10 of its objective between sweeps 1 and 2, lane "C" a
# factor >= 10 of its largest step.  (No pair of draws was found that puts both crossings into ONE call: a small step with an objective
# that is still above the threshold needs f2_C >= f1_B and d1_B >= d1_C at once.)  So each size runs two calls: one whose objective
# threshold sits at the geometric mean of B's two values, one whose step threshold sits at that of C's.
RULE_CASES = {5: dict(base=11, depth=4, B=7, C=109, route="persistent"), 7: dict(base=12, depth=4, B=22, C=3, route="wide")}
MAXITER = 4


def _rule_lane(circ, base, index, noise):
    rng = np.random.default_rng([base, index])
    ts = orc.rand_thetas(circ.num_thetas, rng)
    u = orc.v_mul_mat(circ, ts, np.eye(circ.dimension, dtype=np.complex128))
    return u, ts + noise * rng.standard_normal(circ.num_thetas)


@pytest.fixture(scope="module", params=sorted(RULE_CASES))
def rule_case(request):
    """The lanes of a size (each call takes four of them) and the oracle's MAXITER sweeps of each: profile, max |dtheta|, thetas."""
    n = request.param
    case = RULE_CASES[n]
    circ = _pairs_circuit(n, case["depth"], case["base"])
    # 0: next to the solution; 1, 2: B and C, see above; 3, 4: far enough to run all sweeps whatever the thresholds of the two calls
    lanes = [_rule_lane(circ, case["base"], 100000, 2e-9), _rule_lane(circ, case["base"], case["B"], 1e-5),
             _rule_lane(circ, case["base"], case["C"], 1e-5), _rule_lane(circ, case["base"], 100001, 1e-3),
             _rule_lane(circ, case["base"], 100002, 3e-2)]
    orac = []
    for u, th0 in lanes:
        th, fs, ds, ths = th0, [], [], []
        for _ in range(MAXITER):
            t1, f = orc.coord_descent_single_sweep(circ, th, u)
            fs.append(f); ds.append(float(np.max(np.abs(t1 - th)))); ths.append(t1)
            th = t1
        orac.append((np.array(fs), np.array(ds), ths))
    return n, case, circ, lanes, orac


def _reference_loop(fs, ds, fobj_thr, dtheta_thr):
    """aqc_coord_descent.py:70-101 over recorded sweeps -> (nit, exit_status, index of the best sweep)."""
    best, best_k, nit, status = np.inf, -1, 0, "normal"
    while nit < MAXITER:
        nit += 1
        f = fs[nit - 1]
        if f < best:
            best, best_k = f, nit - 1
        if f < fobj_thr:
            status = "early"
            break
        if ds[nit - 1] < dtheta_thr:
            break
    return nit, status, best_k


def _check_rule_run(n, case, circ, lanes, orac, sel, fobj_thr, dtheta_thr, want):
    from aqc_research_amd.model_sketching.aqc_coord_descent import coordinate_descent_aqc

    lanes, orac = [lanes[i] for i in sel], [orac[i] for i in sel]
    # the condition on the inputs, from the oracle alone: every value a threshold is compared with before a lane ends is a factor
    # sqrt(10) away from it (the pair a geometric-mean threshold separates: a factor >= 10 apart); rounding cannot cross that
    expect = []
    for (fs, ds, _), w in zip(orac, want):
        nit, status, best_k = _reference_loop(fs, ds, fobj_thr, dtheta_thr)
        assert (nit, status) == w
        for k in range(nit):
            assert fobj_thr <= 0 or not (fobj_thr / R10 < fs[k] < fobj_thr * R10), (k, fs[k], fobj_thr)
            early = fs[k] < fobj_thr
            assert early or dtheta_thr == 0 or not (dtheta_thr / R10 < ds[k] < dtheta_thr * R10), (k, ds[k], dtheta_thr)
        expect.append((nit, status, best_k))
    targets = np.stack([u for u, _ in lanes])
    starts = np.stack([t for _, t in lanes])
    runs = [coordinate_descent_aqc(circ, targets, starts, maxiter=MAXITER, fobj_thr=fobj_thr, thetas_change_thr=dtheta_thr, chunk=c,
                                   route=case["route"]) for c in (1, 3)]
    d = circ.dimension
    for b, ((fs, ds, ths), (nit, status, best_k)) in enumerate(zip(orac, expect)):
        r = runs[0][b]
        prof = r["stats"]["convergence_profile"]
        print(n, b, r["nit"], r["exit_status"], r["cost"], fs[:nit], maxdiff(r["thetas"], ths[best_k]))
        assert (r["nit"], r["exit_status"]) == (nit, status) and r["num_iters"] == r["num_fun_ev"] == r["stats"]["nit"] == nit
        assert prof.dtype == np.float32 and prof.shape == (nit,) and np.allclose(prof, fs[:nit].astype(np.float32), rtol=1e-3, atol=1e-14)
        assert np.float32(r["cost"]) == prof.min() and abs(r["cost"] - fs[best_k]) < 1e-7
        assert maxdiff(r["thetas"], ths[best_k]) < 1e-7 and np.array_equal(r["ini_thetas"], starts[b])
        v = orc.v_mul_mat(circ, ths[best_k], np.eye(d, dtype=np.complex128))
        assert abs(r["fidelity"] - (1.0 + abs(np.vdot(v, targets[b])) ** 2 / d) / (d + 1)) < 1e-10
        assert r["entangler"] == circ.entangler and np.array_equal(r["blocks"], circ.blocks)
        # a finished lane does not move in later chunks: one host visit per sweep or per three sweeps, the same results
        other = runs[1][b]
        for key in ("cost", "nit", "exit_status", "fidelity"):
            assert r[key] == other[key], key
        assert np.array_equal(r["thetas"], other["thetas"]) and np.array_equal(prof, other["stats"]["convergence_profile"])


def test_stop_rule_small_objective(rule_case):
    """fobj_thr at the geometric mean of lane B's objective after sweeps 1 and 2: lane 0 ends early after one sweep (its step is below
    the step threshold as well: the small objective is tested first), B early after two, the others run to maxiter."""
    n, case, circ, lanes, orac = rule_case
    fb = orac[1][0]
    assert fb[0] / fb[1] >= 10
    _check_rule_run(n, case, circ, lanes, orac, (0, 1, 3, 4), float(np.sqrt(fb[0] * fb[1])), 1e-7,
                    [(1, "early"), (2, "early"), (MAXITER, "normal"), (MAXITER, "normal")])
    assert orac[0][1][0] < 1e-7 / R10                                    # lane 0's step alone would have ended it as "normal"


def test_stop_rule_small_step(rule_case):
    """dtheta_thr at the geometric mean of lane C's largest step in sweeps 1 and 2, an objective threshold that nothing is below
    (next to the solution the objective is rounding noise of either sign): lane 0 ends after one sweep, C after two, both "normal";
    the two far lanes run to maxiter."""
    n, case, circ, lanes, orac = rule_case
    dc = orac[2][1]
    assert dc[0] / dc[1] >= 10
    _check_rule_run(n, case, circ, lanes, orac, (0, 3, 2, 4), -1.0, float(np.sqrt(dc[0] * dc[1])),
                    [(1, "normal"), (MAXITER, "normal"), (2, "normal"), (MAXITER, "normal")])


def test_maxiter_and_timeout_exits(lanes5, lanes7):
    from aqc_research_amd.model_sketching.aqc_coord_descent import coordinate_descent_aqc

    for circ, ths, us in (lanes5, lanes7[:3]):
        res = coordinate_descent_aqc(circ, us, ths, maxiter=2, fobj_thr=0.0, thetas_change_thr=0.0)
        assert [(r["exit_status"], r["nit"], len(r["stats"]["convergence_profile"])) for r in res] == [("normal", 2, 2)] * 3
        # the limit has passed when the first chunk of two sweeps returns: every lane still running is timed out there
        res = coordinate_descent_aqc(circ, us, ths, maxiter=5, time_limit=1e-9, chunk=2)
        assert [(r["exit_status"], r["nit"]) for r in res] == [("timeout", 2)] * 3
        one = coordinate_descent_aqc(circ, us[0], ths[0], maxiter=1)     # (T,) start and a (d, d) target: one dictionary
        assert one["nit"] == 1 and 0.0 < one["cost"] < 1.0 and 0.0 < one["fidelity"] < 1.0


def test_refusals_leave_no_buffers_behind():
    from aqc_research_amd import ParametricCircuit, TrotterAnsatz
    from aqc_research_amd.engine import BUF_Y, HipContext, Workspace, live_buffers

    blocks = np.array([[0, 1, 2], [1, 2, 0]], dtype=np.int64)
    before = live_buffers()
    for circ, d in ((ParametricCircuit(3, "cp", blocks), 8), (TrotterAnsatz(4, orc.trotter_blocks(4, 1), second_order=False), 16)):
        ws = Workspace(HipContext.of(circ), batch=2, ncols=d)
        try:
            ws.upload(BUF_Y, np.stack([np.eye(d, dtype=np.complex128)] * 2))
            with pytest.raises(RuntimeError, match="CPhase|Trotter"):
                ws.cd_minimize(np.zeros((2, circ.num_thetas)), 3)
        finally:
            ws.close()
    sq = ParametricCircuit(7, "cx", np.array([[0, 3], [1, 5]], dtype=np.int64))
    ws = Workspace(HipContext.of(sq), batch=1, ncols=128)
    try:
        with pytest.raises(RuntimeError, match="do not fit"):
            ws.cd_minimize(np.zeros((1, sq.num_thetas)), 3, route="persistent")
    finally:
        ws.close()
    assert live_buffers() == before
