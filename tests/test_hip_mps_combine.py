"""GPU: linear combinations of MPS states on the device (mps_engine.linear_combinations, aqc_mps_combine; kernel
csrc/aqc_mps_combine.hip, the sweep of compression) on both routes, against sum_k c_k dense(psi_k) and the NumPy statement
(tests/mps_combine_ref.py).

Cases of tests/mps_combine_ref.py.  Bounds: TOL x scale at trunc_thr = 0, scale = sum_k |c_k| |psi_k|; with truncation
TOL x scale / gap against the statement, the relative gap read from the reference's decisions and held to >= 1e-3 there
(tests/test_mps_combine_ref.py), as tests/test_hip_mps_compress.py bounds it.  Ranks must be equal, weights agree within TOL x scale^2.
The tests print what they observe; DESIGN.md records it."""
import functools

import numpy as np
import pytest

from tests import mps_combine_ref, mps_obs_ref
from tests.helpers import TOL
from tests.lane_contract import check_lanes
from tests.test_hip_mps_entanglement import _flat
from tests.test_mps_compress_ref import MIN_GAP, normalised

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _dense(name):
    states, coeffs, _ = mps_combine_ref.case(name)
    vec, scale = mps_combine_ref.dense_sum(states, coeffs)
    vec.setflags(write=False)
    return vec, scale


@functools.lru_cache(maxsize=None)
def _statement(name):
    states, coeffs, _ = mps_combine_ref.case(name)
    return mps_combine_ref.combine(states, coeffs)


def _upload(states):
    """DeviceMPS states of the tuples, one per distinct tuple object (a tuple listed twice is one state listed twice)."""
    from aqc_research_amd.mps_engine import DeviceMPS

    made = {}
    for s in states:
        if id(s) not in made:
            made[id(s)] = DeviceMPS.from_qiskit(s, assume_canonical=True)
    return [made[id(s)] for s in states], list(made.values())


def _vec(state):
    return mps_obs_ref.dense(state.to_qiskit())


def _close(items):
    for x in items:
        if x is not None:
            x.close()


@pytest.mark.parametrize("name", mps_combine_ref.CASES)
def test_exact_sums_on_both_routes(name):
    from aqc_research_amd.mps_engine import is_canonical, linear_combinations

    states, coeffs, want_bonds = mps_combine_ref.case(name)
    n = len(states[0][0])
    want, scale = _dense(name)
    ref = _statement(name)
    dev, owned = _upload(states)
    made = {}
    try:
        before = [_flat(m.to_qiskit()) for m in owned]
        for method in (None, "fused", "canonical"):
            out, info = linear_combinations(dev, coeffs, method=method, details=True)
            made[method] = out
            assert info["route"] == (method or "fused") and info["status"] == 0
            assert info["ranks"].shape == info["dropped"].shape == info["sweeps"].shape == (n - 1,)
            err = float(np.linalg.norm(_vec(out) - want))
            lam = out.to_qiskit()[1]
            lam_err = max([0.0] + [float(np.max(np.abs(a - b))) if a.shape == b.shape else np.inf for a, b in zip(lam, ref.lam)])
            print(f"case {name}, method {method}: |sum - dense sum| = {err:.3g}, max |bond vector - statement| = {lam_err:.3g} (scale {scale:.3g}), "
                  f"bonds -> {out.bond_dims.tolist()}, sweeps {info['sweeps'].tolist()}")
            assert out.bond_dims.tolist() == ref.bond_dims.tolist() == want_bonds and out.bond_dims[1:n].tolist() == info["ranks"].tolist()
            assert err <= TOL * scale and lam_err <= TOL * scale
            if n > 1:
                assert is_canonical(normalised(out.to_qiskit(), float(np.linalg.norm(want))))
            assert abs(out.discarded_weight) <= TOL * scale ** 2 and np.all(np.abs(info["dropped"]) <= TOL * scale ** 2)
            assert [np.array_equal(_flat(m.to_qiskit()), b) for m, b in zip(owned, before)] == [True] * len(owned)   # the inputs, bit for bit
        routes = float(np.linalg.norm(_vec(made["fused"]) - _vec(made["canonical"])))
        print(f"case {name}: |fused - canonical| = {routes:.3g}")
        assert routes <= TOL * scale
        assert np.array_equal(_flat(made[None].to_qiskit()), _flat(made["fused"].to_qiskit()))
        made["tuples"] = linear_combinations(states, coeffs)                              # tuples: uploaded for the call
        assert np.array_equal(_flat(made["tuples"].to_qiskit()), _flat(made["fused"].to_qiskit()))
        assert made["tuples"].discarded_weight == made["fused"].discarded_weight
    finally:
        _close(list(made.values()) + owned)


@pytest.mark.parametrize("as_cap", (False, True), ids=("trunc_thr", "max_bond"))
@pytest.mark.parametrize("name", mps_combine_ref.TRUNCATED)
def test_truncation_matches_the_statement(name, as_cap):
    from aqc_research_amd.mps_engine import linear_combinations

    states, coeffs, _ = mps_combine_ref.case(name)
    n = len(states[0][0])
    _, scale = _dense(name)
    thr, cap, ref, gap = mps_combine_ref.truncation(name, as_cap)
    assert gap is not None and gap >= MIN_GAP
    bound = TOL * scale / gap
    want = ref.to_vector()
    dev, owned = _upload(states)
    made = []
    try:
        for method in ("fused", "canonical"):
            out, info = linear_combinations(dev, coeffs, thr, cap, method=method, details=True)
            made.append(out)
            err = float(np.linalg.norm(_vec(out) - want))
            weight = out.discarded_weight
            got = np.array([d.total - d.kept for d in ref.decisions])
            print(f"case {name}, trunc_thr {thr:g}, max_bond {cap}, {method}: bonds -> {out.bond_dims.tolist()}, |sum - statement| = {err:.3g} "
                  f"(bound {bound:.3g}), discarded {weight:.6g} (statement {ref.discarded:.6g})")
            assert info["status"] == 0
            assert out.bond_dims.tolist() == ref.bond_dims.tolist() and info["ranks"].tolist() == ref.bond_dims[1:n].tolist()
            assert abs(weight - ref.discarded) <= TOL * scale ** 2 and abs(float(info["dropped"].sum()) - weight) <= TOL * scale ** 2
            assert np.max(np.abs(info["dropped"] - got), initial=0.0) <= TOL * scale ** 2
            assert err <= bound
            lam = out.to_qiskit()[1]
            assert max(float(np.max(np.abs(a - b))) for a, b in zip(lam, ref.lam)) <= bound
    finally:
        _close(made + owned)


def test_the_cap_between_the_routes():
    """Four states of bond 16 sum to exactly 64 and go fused; a product state more makes 65 and goes canonical."""
    from aqc_research_amd.mps_engine import combine_route, linear_combinations

    states, coeffs, bonds = mps_combine_ref.case("cap64")
    more, c5 = states + [mps_obs_ref.hand_made([1] * 9, 720)], list(coeffs) + [0.8j]
    want, scale = mps_combine_ref.dense_sum(more, c5)
    dev, owned = _upload(more)
    made = []
    try:
        assert combine_route([m.bond_dims for m in dev[:4]]) == "fused" and combine_route([m.bond_dims for m in dev]) == "canonical"
        out, info = linear_combinations(dev[:4], coeffs, details=True)
        made.append(out)
        assert info["route"] == "fused"
        with pytest.raises(ValueError):
            linear_combinations(dev, c5, method="fused")
        out, info = linear_combinations(dev, c5, details=True)
        made.append(out)
        err = float(np.linalg.norm(_vec(out) - want))
        print(f"summed bond 65, canonical: |sum - dense sum| = {err:.3g} (scale {scale:.3g}), bonds -> {out.bond_dims.tolist()}")
        assert info["route"] == "canonical" and info["status"] == 0
        assert err <= TOL * scale and out.bond_dims.tolist() == mps_combine_ref.combine(more, c5).bond_dims.tolist()
        both, info = linear_combinations(dev, [list(coeffs) + [0.0], c5], details=True)   # the two routes in one call
        made += both
        assert info["route"] == ["fused", "canonical"] and info["status"].tolist() == [0, 0]
        assert np.array_equal(_flat(both[0].to_qiskit()), _flat(made[0].to_qiskit())) and np.array_equal(_flat(both[1].to_qiskit()), _flat(made[1].to_qiskit()))
    finally:
        _close(made + owned)


_MATRIX = np.array([[0.0, 0.0, 1.3 - 0.2j, 0.0],
                    [0.7, 0.0, 0.0, -0.4j],
                    [0.5j, -0.9, 0.0, 0.3],
                    [0.6, 0.2 + 0.7j, -1.1, 0.8j],
                    [0.7, 0.0, 0.0, -0.4j]])


def _matrix_states():
    hm = mps_obs_ref.hand_made
    return [hm(mps_combine_ref.P5, 731), hm(mps_combine_ref.P7, 732), hm([1] * 7, 733), hm(mps_combine_ref.P5, 734)]


def test_many_outputs_in_one_call():
    """A 5 x 4 coefficient matrix with zeros (outputs of 1, 2, 3 and 4 terms) and a repeated row: every output has the bits of its
    one-output call, also when the sweep runs in chunks of 3 and of 1 outputs."""
    from aqc_research_amd import _lib
    from aqc_research_amd.mps_engine import linear_combinations

    L = _lib.lib()
    tuples = _matrix_states()
    dev, owned = _upload(tuples)
    made = []
    per_output = 8 * 16 * 18 * 18   # mps_compress_chunk at K = 5 + 7 + 1 + 5, the largest summed bond of the call
    try:
        whole, info = linear_combinations(dev, _MATRIX, 1e-3, details=True)
        made += whole
        assert len(whole) == 5 and info["status"].tolist() == [0] * 5 and info["route"] == ["fused"] * 5
        assert np.array_equal(_flat(whole[4].to_qiskit()), _flat(whole[1].to_qiskit())) and whole[4].handle.value != whole[1].handle.value
        for j in range(5):
            one, one_info = linear_combinations(dev, _MATRIX[j], 1e-3, details=True)
            made.append(one)
            want, scale = mps_combine_ref.dense_sum(tuples, _MATRIX[j])
            exact = linear_combinations(dev, _MATRIX[j])
            made.append(exact)
            assert float(np.linalg.norm(_vec(exact) - want)) <= TOL * scale
            assert np.array_equal(_flat(one.to_qiskit()), _flat(whole[j].to_qiskit())), j
            assert one.discarded_weight == whole[j].discarded_weight and np.array_equal(one_info["ranks"], info["ranks"][j])
            assert np.array_equal(one_info["dropped"], info["dropped"][j])
        default = L.aqc_mps_combine_svd_budget(3 * per_output + 7)
        assert default == 256 << 20
        for chunk in (3, 1):
            assert L.aqc_mps_combine_svd_budget(chunk * per_output + 7) > 0
            got, again = linear_combinations(dev, _MATRIX, 1e-3, details=True)
            made += got
            for key in ("ranks", "dropped", "sweeps", "status"):
                assert np.array_equal(info[key], again[key]), (chunk, key)
            for j in range(5):
                assert np.array_equal(_flat(got[j].to_qiskit()), _flat(whole[j].to_qiskit())), (chunk, j)
                assert got[j].discarded_weight == whole[j].discarded_weight
    finally:
        L.aqc_mps_combine_svd_budget(0)
        _close(made + owned)
    assert L.aqc_mps_combine_svd_budget(0) == 256 << 20


_WIDE = [1, 2, 4, 33, 40, 8, 2, 1]   # two of these sum to 66 and 80: beyond the fused cap
_LANE_SIZE = 7 * 2 * 80 * 80


@pytest.mark.parametrize("method", ("fused", "canonical"))
def test_outputs_hold_the_lane_contract(method):
    """Four coefficient rows as lanes, probes (0, 3), at a threshold that cuts.  F: the other rows get other finite coefficients; N: they
    get NaN, their outputs get status 2 and no state, and the probes' bits do not move."""
    from aqc_research_amd.mps_engine import linear_combinations

    hm = mps_obs_ref.hand_made
    tuples = [hm(mps_combine_ref.P5, 741), hm(mps_combine_ref.P7, 742), hm([1] * 7, 743)] if method == "fused" else [hm(_WIDE, 744), hm(_WIDE, 745)]
    dev, owned = _upload(tuples)
    rng = np.random.default_rng(746)
    rows = rng.standard_normal((4, len(tuples))) + 1j * rng.standard_normal((4, len(tuples)))
    other = rng.standard_normal((4, len(tuples))) + 1j * rng.standard_normal((4, len(tuples)))

    def run(coeffs):
        results, info = linear_combinations(dev, coeffs, 1e-4, details=True)
        assert info["route"] == [method] * 4
        sites = np.zeros((4, _LANE_SIZE), dtype=np.complex128)
        for l, out in enumerate(results):
            if out is None:
                sites[l] = np.nan
                continue
            flat = _flat(out.to_qiskit())
            sites[l, :flat.size] = flat
            out.close()
        return {"state": sites, "ranks": info["ranks"], "dropped": info["dropped"], "status": info["status"]}

    try:
        base = check_lanes(run, rows, probes=(0, 3), other=other, distinct=("state",))
        assert np.all(base["status"] == 0) and np.all(base["ranks"] >= 1)
        poisoned = rows.copy()
        poisoned[1:3] = np.nan
        results, info = linear_combinations(dev, poisoned, 1e-4, details=True)
        assert results[1] is None and results[2] is None and info["status"].tolist() == [0, 2, 2, 0]
        assert np.all(info["ranks"][1:3] == 0)
        for l in (0, 3):
            flat = _flat(results[l].to_qiskit())
            assert np.array_equal(flat, base["state"][l, :flat.size])
            results[l].close()
        with pytest.raises(RuntimeError, match="output 1, cut 1"):
            linear_combinations(dev, poisoned[:2], 1e-4)
    finally:
        _close(owned)


def test_forty_qubits():
    """Beyond dense reach: n = 40, two hand-made states of bond 16.  With G_jk = <psi_j|psi_k>: <psi_j|out> = sum_k c_k G_jk and
    <out|out> = c^H G c."""
    from aqc_research_amd.mps_engine import DeviceMPS, linear_combinations
    from aqc_research_amd.mps_observables import overlaps

    n = 40
    dims = [min(2 ** q, 2 ** (n - q), 16) for q in range(n + 1)]
    terms = [DeviceMPS.from_qiskit(mps_obs_ref.hand_made(dims, 751 + k), assume_canonical=True) for k in range(2)]
    c = np.array([0.8 - 0.3j, -0.5 + 0.6j])
    out = None
    try:
        out, info = linear_combinations(terms, c, details=True)
        gram = overlaps(terms, terms)
        scale = float(sum(abs(ck) * np.sqrt(gram[k, k].real) for k, ck in enumerate(c)))
        got = overlaps(terms + [out], [out])[:, 0]
        err = float(np.max(np.abs(got[:2] - gram @ c)))
        err_norm = abs(got[2] - c.conj() @ gram @ c)
        print(f"n = {n}, two states of bond 16, route {info['route']}: bonds up to {int(out.bond_dims.max())}, max |<psi_j|out> - sum_k c_k G_jk| = {err:.3g}, "
              f"|<out|out> - c^H G c| = {err_norm:.3g} (scale {scale:.3g})")
        assert info["route"] == "fused" and info["status"] == 0 and int(out.bond_dims.max()) == 32
        assert err <= TOL * scale ** 2 and err_norm <= TOL * scale ** 2
    finally:
        _close(terms + [out])


def test_w_state_of_twelve_qubits():
    from aqc_research_amd.mps_engine import DeviceMPS, linear_combinations

    n = 12
    terms = [DeviceMPS.basis_state(n, 1 << q) for q in range(n)]
    out = None
    try:
        out = linear_combinations(terms, np.full(n, 1.0 / np.sqrt(n)))
        vec = out.to_vector()
        want = np.zeros(1 << n)
        want[[1 << q for q in range(n)]] = 1.0 / np.sqrt(n)
        err = float(np.max(np.abs(vec - want)))
        print(f"W state of {n} qubits: bonds {out.bond_dims.tolist()}, max |amplitude - W| = {err:.3g}")
        assert out.bond_dims.tolist() == [1] + [2] * (n - 1) + [1]
        assert err <= TOL
    finally:
        _close(terms + [out])


def test_plus_and_scaled():
    from aqc_research_amd.mps_engine import linear_combinations

    states, coeffs, _ = mps_combine_ref.case("three")
    dev, owned = _upload(states)
    made = []
    try:
        a, b = dev[0], dev[1]
        thr = mps_combine_ref.truncation("three", False)[0]
        for got, want in ((a.plus(b), linear_combinations([a, b], [1.0, 1.0])),
                          (a.plus(b, -0.5j, thr, 4, method="canonical"), linear_combinations([a, b], [1.0, -0.5j], thr, 4, method="canonical")),
                          (a.plus(a), linear_combinations([a, a], [1.0, 1.0])),
                          (a.scaled(0.3 - 2.0j), linear_combinations([a], [0.3 - 2.0j]))):
            made += [got, want]
            assert np.array_equal(_flat(got.to_qiskit()), _flat(want.to_qiskit())) and got.discarded_weight == want.discarded_weight
        out, info = a.plus(b, 2.0, details=True)
        made.append(out)
        assert info["status"] == 0 and info["route"] == "fused"
        scaled = made[-3]
        err = float(np.linalg.norm(_vec(scaled) - (0.3 - 2.0j) * mps_obs_ref.dense(states[0])))
        assert err <= TOL * abs(0.3 - 2.0j) and scaled.bond_dims.tolist() == mps_combine_ref.P5
    finally:
        _close(made + owned)


def test_refusals_leave_no_buffers_and_a_correct_call_follows():
    from ctypes import c_void_p

    from aqc_research_amd import _lib
    from aqc_research_amd.engine import live_buffers
    from aqc_research_amd.mps_engine import DeviceMPS, linear_combinations

    L = _lib.lib()
    states, coeffs, bonds = mps_combine_ref.case("n3")
    dev, owned = _upload(states)
    wide = DeviceMPS.from_qiskit(mps_obs_ref.hand_made([1, 2, 33, 1], 761), assume_canonical=True)
    five = DeviceMPS.basis_state(5)
    owned += [wide, five]
    made = []
    try:
        hs, out = (c_void_p * 2)(dev[0].handle, dev[1].handle), (c_void_p * 2)()
        off, st = np.array([0, 2, 3], np.int32), np.array([0, 1, 1], np.int32)
        cf = np.array([1.0, 0.0, 0.5, 0.5, -1.0, 0.0])
        ranks, sweeps, status, dropped = np.zeros((2, 2), np.int32), np.zeros((2, 2), np.int32), np.zeros(2, np.int32), np.zeros((2, 2))

        def call(states=hs, nstates=2, nout=2, term_off=off, term_state=st, coeffs=cf, thr=0.0, cap=0, method=0, dst=out):
            ip = lambda a: None if a is None else _lib.iptr(a)   # noqa: E731
            return L.aqc_mps_combine(states, nstates, nout, ip(term_off), ip(term_state), None if coeffs is None else _lib.dptr(coeffs), thr, cap, method,
                                     dst, _lib.iptr(ranks), _lib.dptr(dropped), _lib.iptr(sweeps), _lib.iptr(status))

        live = live_buffers()
        assert call(states=None) == 1 and call(dst=None) == 1 and call(term_off=None) == 1 and call(term_state=None) == 1 and call(coeffs=None) == 1
        assert call(nout=0) == 1 and call(nstates=0) == 1 and call(method=3) == 1
        assert call(states=(c_void_p * 2)(dev[0].handle, None)) == 1
        assert call(states=(c_void_p * 2)(dev[0].handle, five.handle)) == 1 and b"differ" in L.aqc_last_error()            # mixed n
        assert call(term_off=np.array([1, 2, 3], np.int32)) == 1 and b"term_off" in L.aqc_last_error()
        assert call(term_off=np.array([0, 0, 3], np.int32)) == 1 and b"at least one term" in L.aqc_last_error()
        assert call(term_off=np.array([0, 3, 2], np.int32)) == 1 and b"at least one term" in L.aqc_last_error()
        assert call(term_state=np.array([0, 2, 1], np.int32)) == 1 and b"outside" in L.aqc_last_error()
        assert call(term_state=np.array([0, -1, 1], np.int32)) == 1 and b"outside" in L.aqc_last_error()
        assert call(states=(c_void_p * 2)(wide.handle, wide.handle), method=1) == 1 and b"fused" in L.aqc_last_error()    # 66: beyond the cap
        assert call(cap=-1) == 1 and b"max_bond" in L.aqc_last_error()
        assert call(thr=-1e-3) == 1 and b"trunc_thr" in L.aqc_last_error()
        assert call(thr=float("nan")) == 1 and b"trunc_thr" in L.aqc_last_error()
        assert out[0] is None and out[1] is None and live_buffers() == live
        closed = DeviceMPS.basis_state(3)
        closed.close()
        for bad in (lambda: linear_combinations([dev[0], five], [1.0, 1.0]), lambda: linear_combinations([dev[0], closed], [1.0, 1.0]),
                    lambda: linear_combinations([wide, wide], [1.0, 1.0], method="fused"), lambda: linear_combinations(dev, coeffs, 0.0, -1),
                    lambda: linear_combinations(dev, coeffs, -1e-3), lambda: linear_combinations(dev, [0.0, 0.0]),
                    lambda: linear_combinations(dev, coeffs, method="gemm"), lambda: linear_combinations(dev, [1.0])):
            with pytest.raises(ValueError):
                bad()
        assert live_buffers() == live
        with pytest.raises(RuntimeError, match="output 0"):
            linear_combinations(dev, [1.0, float("nan")])
        assert live_buffers() == live
        ok = linear_combinations(dev, coeffs)
        made.append(ok)
        want, scale = mps_combine_ref.dense_sum(states, coeffs)
        assert float(np.linalg.norm(_vec(ok) - want)) <= TOL * scale and ok.bond_dims.tolist() == bonds
        ok.close()
        assert call() == 0 and out[0] and out[1] and out[0] != out[1] and status.tolist() == [0, 0]
        assert ranks[0].tolist() == mps_combine_ref.combine(states, [1.0, 0.5 + 0.5j]).bond_dims[1:3].tolist()
        assert ranks[1].tolist() == [1, 2]                                                      # - psi_1 alone: its own bonds
        for h in out:
            assert L.aqc_mps_destroy(c_void_p(h)) == 0
        assert live_buffers() == live
    finally:
        _close(owned)
