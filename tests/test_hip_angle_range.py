"""GPU: every theta-consuming kernel at angles outside [-pi, pi] (patterns and expected lane signs: tests/angle_cases.py).

Every other GPU test draws pi (2u - 1), on which no half-angle cosine is negative: the c < 0 branch of put_pair, the parity count of
sign_kernel with its Trotter-tail exclusion, the per-lane sign applied on the last stage of V x / V^H y and its cancellation inside
the sweeps never run there.  References: the compiled CPU restatement (oracle/aqc_ref.c), the NumPy oracle where that has no entry;
unit-norm inputs, so the absolute tolerance IS 1e-10 (tests/test_hip_parity_random.py)."""
import numpy as np
import pytest

from oracle import aqc_oracle as orc
from oracle import aqc_ref as cref
from tests import angle_cases as ac
from tests.helpers import FAMILIES, FAMILY_ENV, TOL, maxdiff

pytestmark = pytest.mark.gpu

SWITCHES = ("AQC_SPARSE_MIN_ITEMS", "AQC_PROJECTED_VDAG_MIN_ELEMS", "AQC_PROJECTED", "AQC_LAZY_Z", "AQC_SPARSE_SWEEP",
            "AQC_KERNEL_FAMILY", "AQC_PROJECTED_VDAG")
FORCED = {"AQC_SPARSE_MIN_ITEMS": "1", "AQC_PROJECTED_VDAG_MIN_ELEMS": "1"}     # as tests/test_hip_call_sequences.py


def _circuit(a):
    from aqc_research_amd import ParametricCircuit, TrotterAnsatz

    return TrotterAnsatz(a.n, a.blocks, second_order=a.second_order) if a.trotter else ParametricCircuit(a.n, a.entangler, a.blocks)


def _unit(shape, rng):
    v = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return v / np.sqrt((np.abs(v.reshape(shape[0], -1)) ** 2).sum(axis=1)).reshape((shape[0],) + (1,) * (len(shape) - 1))


def _family_shape(family, kind):
    """Circuit name and tile bits of part a: two stages on every family for the spin layouts, so that `final_stage` matters."""
    if kind.startswith("trot"):
        return f"{kind}_8", (8 if family == "mfma" else 6)
    return (f"{kind}10", 8) if family == "mfma" else (f"{kind}9", 6)


def _partial_range(a):
    """A partial block range: inside a second-order Trotter ansatz it takes in tail records and others."""
    return (2, a.num_blocks // 2 + 1)


# ---- a. state vectors, three families ------------------------------------------------------------------------------------------

def _sv_run(a, tile, th, x, y, br):
    """V x, V^H y, the full and the partial gradient of every lane on one workspace."""
    from aqc_research_amd.engine import BUF_X, BUF_Y, BUF_Z, HipContext, Workspace

    ws = Workspace(HipContext.of(_circuit(a)), batch=th.shape[0], tile_bits_apply=tile, tile_bits_sweep=tile)
    try:
        ws.set_thetas(th)
        ws.upload(BUF_X, x)
        ws.upload(BUF_Y, y)
        ws.apply(True, BUF_Y, BUF_Z)
        z = ws.download(BUF_Z)
        ws.grad()
        g = ws.get_grads()
        ws.grad(br, False)
        gp = ws.get_grads()
        ws.apply(False, BUF_X, BUF_Y)
        vx = ws.download(BUF_Y)
        stages = ws.plan_info(2)[0]
    finally:
        ws.close()
    return vx, z, g, gp, stages


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", ["cx", "cz", "cp", "trot1", "trot2"])
@pytest.mark.parametrize("pattern", ["wide", "flip_all", "exact", "far", "lanes_mixed"])
def test_state_vector_patterns(pattern, kind, family, monkeypatch):
    """V x, V^H y, the gradient (full; partial block_range with front_layer=False), lane by lane against the compiled oracle."""
    monkeypatch.setenv("AQC_KERNEL_FAMILY", FAMILY_ENV[family])
    name, tile = _family_shape(family, kind)
    a, th, par = ac.case(name, pattern)                     # asserts, from the angles alone, that the sign path is taken
    rng = np.random.default_rng(ac.seed_for(name, pattern) + 1000)
    x, y = _unit((4, a.dim), rng), _unit((4, a.dim), rng)
    br = _partial_range(a)
    vx, z, g, gp, stages = _sv_run(a, tile, th, x, y, br)
    assert stages >= 2 or a.n <= tile
    bad = []
    for b in range(4):
        zr = cref.v_dagger_mul_vec(a, th[b], y[b])
        errs = (maxdiff(vx[b], cref.v_mul_vec(a, th[b], x[b])), maxdiff(z[b], zr), maxdiff(g[b], cref.grad_of_dot_product(a, th[b], x[b], zr)),
                maxdiff(gp[b], cref.grad_of_dot_product(a, th[b], x[b], zr, br, False)))
        print(f"{family} {name} {pattern} lane {b} parity {par[b]}: |Vx| {errs[0]:.3g} |VHy| {errs[1]:.3g} |g| {errs[2]:.3g} |g part| {errs[3]:.3g}")
        if not max(errs) < TOL:
            bad.append((b, errs))
    assert not bad, f"lanes off: {bad}; parities {par.tolist()}"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind,role", [("cx", "front"), ("cz", "block"), ("cp", "front"), ("cp", "block"), ("cp", "cp"), ("trot1", "block"),
                                       ("trot2", "front"), ("trot2", "block"), ("trot2", "tail")])
def test_two_pi_on_one_parameter_negates_or_keeps_v(kind, role, family, monkeypatch):
    """2 pi on one half-angle parameter negates all of V x and V^H y -- unless the parameter belongs to a tail record of a second-order
    Trotter ansatz, applied twice, or is the CPhase angle: then nothing changes.  Lane 0 holds the base thetas, lane 1 the flipped ones,
    the same x and y in both; both lanes against the oracle as well."""
    monkeypatch.setenv("AQC_KERNEL_FAMILY", FAMILY_ENV[family])
    name, tile = _family_shape(family, kind)
    a = ac.ansatz(name)
    base, flipped, t = ac.one_flip_pair(a, role, 5)
    th = np.stack([base, flipped])
    par = ac.parity(a, th)
    ac.check_reaches_sign_path(a, "one_flip", flipped, par[1], role)
    assert par[0] == 0 and par[1] == (0 if role in ("tail", "cp") else 1)
    s = 1.0 - 2.0 * par[1]
    rng = np.random.default_rng(77)
    x, y = _unit((1, a.dim), rng).repeat(2, axis=0), _unit((1, a.dim), rng).repeat(2, axis=0)
    br = _partial_range(a)
    vx, z, g, gp, _ = _sv_run(a, tile, th, x, y, br)
    print(f"{family} {name} {role} theta {t}: |Vx' - s Vx| {maxdiff(vx[1], s * vx[0]):.3g} |z' - s z| {maxdiff(z[1], s * z[0]):.3g} "
          f"|g' - s g| {maxdiff(g[1], s * g[0]):.3g}")
    assert np.abs(vx[0]).max() > 1e-3
    assert maxdiff(vx[1], s * vx[0]) < TOL and maxdiff(z[1], s * z[0]) < TOL
    assert maxdiff(g[1], s * g[0]) < TOL and maxdiff(gp[1], s * gp[0]) < TOL       # z = V^H y carries the sign into <V x|y>
    for b in range(2):
        zr = cref.v_dagger_mul_vec(a, th[b], y[b])
        assert maxdiff(vx[b], cref.v_mul_vec(a, th[b], x[b])) < TOL and maxdiff(z[b], zr) < TOL
        assert maxdiff(g[b], cref.grad_of_dot_product(a, th[b], x[b], zr)) < TOL
        assert maxdiff(gp[b], cref.grad_of_dot_product(a, th[b], x[b], zr, br, False)) < TOL


# ---- b. matrix route -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("ent", ["cx", "cz", "cp"])
@pytest.mark.parametrize("ncols", [3, 8])
@pytest.mark.parametrize("pattern", ["wide", "lanes_mixed"])
def test_matrix_route(pattern, ncols, ent, family, monkeypatch):
    from aqc_research_amd.engine import BUF_X, BUF_Y, BUF_Z, HipContext, Workspace

    monkeypatch.setenv("AQC_KERNEL_FAMILY", FAMILY_ENV[family])
    a, th, par = ac.case(f"{ent}5", pattern)
    rng = np.random.default_rng(2000 + ncols)
    x, y = _unit((4, a.dim, ncols), rng), _unit((4, a.dim, ncols), rng)
    ws = Workspace(HipContext.of(_circuit(a)), batch=4, ncols=ncols)
    try:
        ws.set_thetas(th)
        ws.upload(BUF_X, x)
        ws.upload(BUF_Y, y)
        ws.apply(True, BUF_Y, BUF_Z)
        z = ws.download(BUF_Z)
        ws.grad()
        g = ws.get_grads()
        ws.apply(False, BUF_X, BUF_Y)
        vx = ws.download(BUF_Y)
    finally:
        ws.close()
    for b in range(4):
        zr = cref.v_dagger_mul_mat(a, th[b], y[b])
        errs = (maxdiff(vx[b], cref.v_mul_mat(a, th[b], x[b])), maxdiff(z[b], zr), maxdiff(g[b], cref.grad_of_matrix_dot_product(a, th[b], x[b], zr)))
        print(f"{family} {ent} k={ncols} {pattern} lane {b} parity {par[b]}: {errs}")
        assert max(errs) < TOL, (b, int(par[b]), errs)


# ---- c. one-call evaluations, sparse and projected routes -------------------------------------------------------------------------

ONE_CALL = {"cx13": 8, "cp14": 9, "trot2_13": 10}          # circuit -> tile bits
_ONE_CALL_CACHE = {}


def _one_call_reference(name, pattern):
    """Thetas, targets, lhs / gather indices and the oracle's V^H y and gradients: computed once, shared by the route settings."""
    key = (name, pattern)
    if key not in _ONE_CALL_CACHE:
        a, th, par = ac.case(name, pattern)
        tile = ONE_CALL[name]
        rng = np.random.default_rng(3000 + tile)
        y = _unit((4, a.dim), rng)
        x_idx = [(3 << tile) | (5 + b) for b in range(4)]                  # a tile that the gather set does not touch
        gather = np.array([0, 1, 1 << tile, x_idx[0], a.dim - 1], np.int64)
        zr = np.stack([cref.v_dagger_mul_vec(a, th[b], y[b]) for b in range(4)])
        br = _partial_range(a)
        e = np.eye(1, a.dim, 0, dtype=complex).ravel()
        gr = np.stack([cref.grad_of_dot_product(a, th[b], np.roll(e, x_idx[b]), zr[b]) for b in range(4)])
        gpr = np.stack([cref.grad_of_dot_product(a, th[b], np.roll(e, x_idx[b]), zr[b], br, False) for b in range(4)])
        _ONE_CALL_CACHE[key] = (a, th, par, y, x_idx, gather, zr, br, gr, gpr)
    return _ONE_CALL_CACHE[key]


def _one_call_run(monkeypatch, env, name, pattern, routes):
    from aqc_research_amd.engine import BUF_X, BUF_Y, BUF_Z, HipContext, Workspace

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a, th, par, y, x_idx, gather, zr, br, gr, gpr = _one_call_reference(name, pattern)
    tile = ONE_CALL[name]
    ws = Workspace(HipContext(_circuit(a)), batch=4, tile_bits_apply=tile, tile_bits_sweep=tile)
    try:
        ws.upload(BUF_Y, y)
        ws.set_basis(BUF_X, x_idx)
        ws.gather_setup(gather)
        hs, g = ws.eval(th, vdag=True, gather=True, grad=True)
        if routes is not None:
            assert ws.sparse_counts()[0] > 0, "the sparse route did not run"
            assert bool(ws.projected_info()) == routes
        hs_p, gp = ws.eval(th, vdag=True, gather=True, grad=True, block_range=br, front_layer=False)
        ws.set_thetas(th[::-1].copy())                       # something else in between: the launch below recomputes everything
        ws.objective_launch(BUF_X)
        ws.set_thetas(th)
        ws.objective_launch(BUF_X)
        hs_l, g_l = ws.gather_fetch(), ws.get_grads()
        z = ws.download(BUF_Z)
    finally:
        ws.close()
    bad = []
    for b in range(4):
        errs = (maxdiff(hs[b], zr[b][gather]), maxdiff(g[b], gr[b]), maxdiff(hs_p[b], zr[b][gather]), maxdiff(gp[b], gpr[b]),
                maxdiff(hs_l[b], zr[b][gather]), maxdiff(g_l[b], gr[b]), maxdiff(z[b], zr[b]))
        print(f"{name} {env} {pattern} lane {b} parity {par[b]}: {errs}")
        if not max(errs) < TOL:
            bad.append((b, errs))
    assert not bad, f"lanes off: {bad}; parities {par.tolist()}"


@pytest.mark.parametrize("name", sorted(ONE_CALL))
@pytest.mark.parametrize("projected", ["1", "0"])
@pytest.mark.parametrize("pattern", ["wide", "lanes_mixed"])
def test_one_call_evaluations_on_the_sparse_and_projected_routes(pattern, projected, name, monkeypatch):
    """ws.eval(vdag, gather, grad) and objective_launch from one basis state per lane with the sparse / projected routes forced on
    problems this small: the gathered amplitudes h_i = (V^H y)[i] carry the lane sign, the gradient carries it through z."""
    _one_call_run(monkeypatch, dict(FORCED, AQC_PROJECTED=projected), name, pattern, projected == "1")


@pytest.mark.parametrize("name", ["cx13", "trot2_13"])
@pytest.mark.parametrize("pattern", ["wide", "lanes_mixed"])
def test_one_call_evaluations_on_the_register_blocked_family(pattern, name, monkeypatch):
    """The same calls on the family whose last stage applies the lane sign (the routes above belong to the matrix cores)."""
    _one_call_run(monkeypatch, dict(FORCED, AQC_KERNEL_FAMILY=FAMILY_ENV["register-blocked"]), name, pattern, None)


# ---- d. coordinate descent from starts outside the range --------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[("cd5", "persistent"), ("cd7", "wide")])
def cd_case(request):
    name, route = request.param
    a, th, par = ac.case(name, "wide")
    rng = np.random.default_rng(4000 + a.n)
    d = a.dim
    us = np.stack([np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0] for _ in range(3)])
    return a, route, th, us


def _cd(a, th, us, route, **kw):
    from aqc_research_amd.engine import BUF_Y, HipContext, Workspace

    ws = Workspace(HipContext.of(_circuit(a)), batch=th.shape[0], ncols=a.dim)
    try:
        ws.upload(BUF_Y, np.ascontiguousarray(us))
        return ws.cd_minimize(th, 1, route=route, fobj_thr=0.0, dtheta_thr=0.0, **kw)
    finally:
        ws.close()


@pytest.mark.parametrize("steps", [1, 5])
def test_coordinate_descent_single_steps(cd_case, steps):
    """The `cs` table at the start of a sweep and t_new = t_old + dt composed on it (aqc_cd.hip), from angles up to 3 pi."""
    a, route, th, us = cd_case
    res = _cd(a, th, us, route, max_steps=steps)
    for b in range(3):
        ref, f_ref = orc.coord_descent_single_sweep(a, th[b], us[b], max_steps=steps)
        assert int((np.abs(ref - th[b]) > 0).sum()) == steps
        print(f"n={a.n} {route} steps={steps} lane {b}: |dtheta| {maxdiff(res['thetas'][b], ref):.3g} |df| {abs(res['cost'][b] - f_ref):.3g}")
        assert maxdiff(res["thetas"][b], ref) < TOL and abs(res["cost"][b] - f_ref) < TOL


def test_coordinate_descent_whole_sweep(cd_case):
    """One whole sweep at the bounds of tests/test_hip_cd_driver.py (rounding amplified along ~T sequential steps): 1e-8 / 1e-7."""
    a, route, th, us = cd_case
    res = _cd(a, th, us, route)
    for b in range(3):
        ref, f_ref = orc.coord_descent_single_sweep(a, th[b], us[b])
        assert np.abs(ref).max() > np.pi                                 # the sweep does not wrap its angles either
        print(f"n={a.n} {route} lane {b}: |dtheta| {maxdiff(res['thetas'][b], ref):.3g} |df| {abs(res['cost'][b] - f_ref):.3g}")
        assert abs(res["cost"][b] - f_ref) < 1e-8 and maxdiff(res["thetas"][b], ref) < 1e-7 and res["nit"][b] == 1


# ---- e. MPS routes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mps_cx6", "mps_trot2_6"])
def test_mps_routes(name):
    """fast_dot_gradient_mps on the single-lane engine (trunc_thr = 1e-16) and evaluate_lanes in lockstep against the dense oracle."""
    from aqc_research_amd import mps_engine as me

    a, th, par = ac.case(name, "wide")
    circ = _circuit(a)
    rng = np.random.default_rng(5000 + a.num_blocks)
    tmps = [orc.random_mps(a.n, 3, rng) for _ in range(3)]
    lmps = [orc.random_mps(a.n, 2, rng) for _ in range(3)]
    targets, lhs = [me.DeviceMPS.from_qiskit(m) for m in tmps], [me.DeviceMPS.from_qiskit(m) for m in lmps]
    br = _partial_range(a)
    try:
        h, g = me.evaluate_lanes(circ, th, targets, lhs, method="lockstep")
        hp, gp = me.evaluate_lanes(circ, th, targets, lhs, block_range=br, front_layer=False, method="lockstep")
        for b in range(3):
            x, dense = orc.mps_to_vector(lmps[b]), orc.v_dagger_mul_vec(a, th[b], orc.mps_to_vector(tmps[b]))
            gr, gpr = orc.grad_of_dot_product(a, th[b], x, dense), orc.grad_of_dot_product(a, th[b], x, dense, br, False)
            vh = me.v_dagger_mul_mps(circ, th[b], targets[b], trunc_thr=1e-16, method="single")
            try:
                h1 = lhs[b].dot(vh)
                g1 = me.fast_dot_gradient_mps(circ, th[b], lhs[b], vh, trunc_thr=1e-16, method="single")
                gp1 = me.fast_dot_gradient_mps(circ, th[b], lhs[b], vh, trunc_thr=1e-16, block_range=br, front_layer=False, method="single")
            finally:
                vh.close()
            errs = (abs(h[b] - np.vdot(x, dense)), maxdiff(g[b], gr), abs(hp[b] - np.vdot(x, dense)), maxdiff(gp[b], gpr),
                    abs(h1 - np.vdot(x, dense)), maxdiff(g1, gr), maxdiff(gp1, gpr))
            print(f"{name} lane {b} parity {par[b]}: {errs}")
            assert max(errs) < TOL, (b, errs)
    finally:
        for m in targets + lhs:
            m.close()


# ---- f. gate-level primitives ----------------------------------------------------------------------------------------------------

PRIM_ANGLES = np.concatenate([ac.EXACT, [7.3, -7.3, 50.1, -50.1]])


def _rot2(name, angle):
    """The closed forms of core_operations.py:164-264."""
    c, s = np.cos(0.5 * angle), np.sin(0.5 * angle)
    return {"rx": np.array([[c, -1j * s], [-1j * s, c]]), "ry": np.array([[c, -s], [s, c]], dtype=complex),
            "rz": np.array([[np.exp(-0.5j * angle), 0], [0, np.exp(0.5j * angle)]])}[name]


def _on_qubit(g, q, arr, n):
    """g on qubit q (bit q of the row index) of an array whose first axis has 2^n entries."""
    t = arr.reshape((1 << (n - 1 - q), 2, 1 << q) + arr.shape[1:])
    return np.einsum("ij,ajb...->aib...", g, t).reshape(arr.shape)


def test_gate_primitives_at_wide_angles():
    from aqc_research_amd import core_op_matrix as com
    from aqc_research_amd import core_operations as cop

    n, k = 5, 3
    rng = np.random.default_rng(6000)
    vec = _unit((1, 1 << n), rng)[0]
    mat = _unit((1, 1 << n, k), rng)[0]
    tmp = np.zeros_like(vec)
    worst = 0.0
    for angle in PRIM_ANGLES:
        for name, fv, fm in (("rx", cop.rx_mul_vec, com.rx_mul_mat), ("ry", cop.ry_mul_vec, com.ry_mul_mat), ("rz", cop.rz_mul_vec, com.rz_mul_mat)):
            g = _rot2(name, float(angle))
            for pos in range(n):
                worst = max(worst, maxdiff(fv(n, pos, float(angle), vec.copy(), tmp), _on_qubit(g, n - 1 - pos, vec, n)),   # big-endian positions
                            maxdiff(fm(float(angle), pos, mat.copy(), np.zeros_like(mat)), _on_qubit(g, pos, mat, n)))
        for c in range(n):
            for t in range(n):
                if c == t:
                    continue
                both = ((np.arange(1 << n) >> (n - 1 - c)) & (np.arange(1 << n) >> (n - 1 - t)) & 1).astype(bool)
                ref = np.where(both, np.exp(1j * angle) * vec, vec)
                dref = np.where(both, 1j * np.exp(1j * angle) * vec, 0.0)
                out = np.full_like(vec, 7.0)
                worst = max(worst, maxdiff(cop.cp_mul_vec(n, c, t, float(angle), vec.copy(), tmp), ref),
                            maxdiff(cop.derv_cphase_mul_vec(n, c, t, float(angle), vec.copy(), out), dref))
    print("gate primitives, worst deviation:", worst)
    assert worst < TOL


# ---- g. the objective object the device L-BFGS starts on --------------------------------------------------------------------------

@pytest.mark.parametrize("family", FAMILIES)
def test_batched_surrogate_objective_from_mixed_starts(family, monkeypatch):
    """BatchedSurrogateObjective.value_and_grad on a second-order Trotter ansatz from lanes_mixed starts against orc.SurMaxOracle.  The
    first call with update_state=True applies hysteresis and weight smoothing, then evaluates under the new state: that is the oracle's
    SECOND objective() / gradient() pair at the same thetas (its first pair evaluates under weight 1 and smooths afterwards)."""
    from aqc_research_amd.batched_optimizer import BatchedSurrogateObjective

    monkeypatch.setenv("AQC_KERNEL_FAMILY", FAMILY_ENV[family])
    a, th, par = ac.case("trot2_12", "lanes_mixed")
    circ = _circuit(a)
    neel = sum(1 << q for q in range(0, a.n, 2))
    rng = np.random.default_rng(7000)
    targets = _unit((4, a.dim), rng)
    bo = BatchedSurrogateObjective(circ, targets, base_index=neel)
    try:
        f, g = bo.value_and_grad(th)
        for b in range(4):
            o = orc.SurMaxOracle(a, targets[b], 1, None, True, base_index=neel)
            o.objective(th[b])
            o.gradient(th[b])
            fr, gr = o.objective(th[b]), o.gradient(th[b])
            print(f"lane {b} parity {par[b]} leading {o.max_no}: |df| {abs(f[b] - fr):.3g} |dg| {maxdiff(g[b], gr):.3g}")
            assert abs(f[b] - fr) < TOL and maxdiff(g[b], gr) < TOL and bo.max_no[b] == o.max_no
            assert abs(bo.fidelity[b] - o.fidelity) < TOL
    finally:
        bo.close()
