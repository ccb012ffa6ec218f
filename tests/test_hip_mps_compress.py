"""GPU: MPS compression on the device (mps_engine.compress, aqc_mps_compress; kernels csrc/aqc_mps_compress.hip) on both routes, against
the dense vector, the NumPy statement (tests/mps_compress_ref.py), and the loop it replaces: clone().canonicalize() followed by a
sweep of truncating identity gates.

Profiles of tests/test_hip_mps_entanglement.py (A, B13, B2, C, F, pad, Q1 = one qubit, D beyond the fused cap).  Bounds: TOL x |psi| at
trunc_thr = 0; with truncation TOL x |psi| x s_max / gap against the statement (Wedin's bound on the kept subspace: two SVDs of the
same matrix that differ by rounding agree on it to rounding / gap), the gap read from the reference's decisions and held to >= 1e-3
there (tests/test_mps_compress_ref.py), where the thresholds and caps are chosen too.  Ranks must be equal, weights agree within TOL.
The tests print what they observe; DESIGN.md 6v records it."""
import functools

import numpy as np
import pytest

from tests import mps_compress_ref, mps_obs_ref, mps_trunc_ref
from tests.helpers import TOL
from tests.lane_contract import check_lanes
from tests.test_hip_mps_entanglement import _LANE_BONDS, _case, _flat, _lane_mps
from tests.test_mps_compress_ref import MIN_GAP, normalised, truncation
from tests.test_mps_ent_ref import NAMES as CPU_NAMES

pytestmark = pytest.mark.gpu

NAMES = list(CPU_NAMES) + ["D", "Q1"]
COMPARED_MIN = 40   # every one of the 40 states of profile C clears the margins and the gap at trunc_thr 1e-3 on the reference
EYE4 = np.eye(4, dtype=np.complex128)


@functools.lru_cache(maxsize=None)
def _dense(name):
    psi = mps_obs_ref.dense(_case(name)[0])
    psi.setflags(write=False)
    return psi


@functools.lru_cache(maxsize=None)
def _exact_bonds(name):
    """The bonds trunc_thr = 0 leaves (the ranks of the cuts), by the NumPy statement."""
    return mps_compress_ref.compress(_case(name)[0]).bond_dims.tolist() if name != "Q1" else [1, 1]


def _device(name):
    from aqc_research_amd.mps_engine import DeviceMPS

    return DeviceMPS.from_qiskit(_case(name)[0], assume_canonical=True)


def _vec(state):
    return mps_obs_ref.dense(state.to_qiskit())


def _loop(state, thr, cap):
    """What compress replaces, on the engine: a canonical clone, then a truncating identity gate on every bond, left to right."""
    m = state.clone().canonicalize()
    for q in range(m.num_qubits - 1):
        m.gate2(EYE4, q, q + 1, thr, cap)
    return m


@pytest.mark.parametrize("name", NAMES)
def test_exact_compression_on_both_routes(name):
    from aqc_research_amd.mps_engine import compress, compress_route, is_canonical

    mps, dims, norm, want = _case(name)
    n, psi = len(dims) - 1, _dense(name)
    m = _device(name)
    made = {}
    try:
        assert compress_route(m.bond_dims) == ("canonical" if name == "D" else "fused")
        before = _flat(m.to_qiskit())
        for method in (None, "fused", "canonical"):
            if name == "D" and method == "fused":
                with pytest.raises(ValueError):
                    compress(m, method="fused")
                continue
            out, info = compress(m, method=method, details=True)
            made[method] = out
            assert info["route"] == (method or ("canonical" if name == "D" else "fused")) and info["status"] == 0
            assert info["ranks"].shape == info["dropped"].shape == info["sweeps"].shape == (n - 1,)
            new = out.bond_dims.tolist()
            err = float(np.linalg.norm(_vec(out) - psi))
            lam = out.to_qiskit()[1]
            lam_err = max([0.0] + [float(np.max(np.abs(lam[q - 1] - want[q - 1, :new[q]]))) for q in range(1, n)])
            print(f"profile {name}, method {method}: |compressed - psi| = {err:.3g}, max |bond vector - dense SVD| = {lam_err:.3g} (|psi| = {norm:.3g}), "
                  f"bonds {dims} -> {new}, sweeps {info['sweeps'].tolist()}")
            assert err <= TOL * norm and lam_err <= TOL * norm
            assert all(np.all(want[q - 1, new[q]:] <= TOL * norm) for q in range(1, n))
            assert is_canonical(normalised(out.to_qiskit(), norm))
            assert new == _exact_bonds(name) and new[1:n] == info["ranks"].tolist()     # the ranks of the cuts
            assert abs(out.discarded_weight) <= TOL * norm ** 2 and np.all(np.abs(info["dropped"]) <= TOL * norm ** 2)
            assert out.num_qubits == n and out.handle.value != m.handle.value
            assert np.array_equal(_flat(m.to_qiskit()), before)                         # the input, bit for bit
        if "fused" in made:
            routes = float(np.linalg.norm(_vec(made["fused"]) - _vec(made["canonical"])))
            print(f"profile {name}: |fused - canonical| = {routes:.3g}")
            assert routes <= TOL * norm
            assert np.array_equal(_flat(made[None].to_qiskit()), _flat(made["fused"].to_qiskit()))
            again = m.compressed()
            made["again"] = again
            assert np.array_equal(_flat(again.to_qiskit()), _flat(made["fused"].to_qiskit()))
            from_tuple = compress(mps)                                                    # a tuple: uploaded for the call
            made["tuple"] = from_tuple
            assert np.array_equal(_flat(from_tuple.to_qiskit()), _flat(made["fused"].to_qiskit()))
        if name == "pad":
            assert dims[4] == 8 and made["fused"].bond_dims[4] == 4
    finally:
        for x in list(made.values()) + [m]:
            x.close()


@pytest.mark.parametrize("as_cap", (False, True), ids=("trunc_thr", "max_bond"))
@pytest.mark.parametrize("name", CPU_NAMES)
def test_truncation_matches_the_statement_and_the_loop(name, as_cap):
    from aqc_research_amd.mps_engine import compress

    _, dims, norm, _ = _case(name)
    n = len(dims) - 1
    thr, cap, ref, gap = truncation(name, as_cap)
    assert gap is None or gap >= MIN_GAP
    bound = TOL * norm / (gap if gap else 1.0)
    want = ref.to_vector()
    m = _device(name)
    made = []
    try:
        loop = _loop(m, thr, cap)
        made.append(loop)
        loop_vec = _vec(loop)
        for method in ("fused", "canonical"):
            out, info = compress(m, thr, cap, method=method, details=True)
            made.append(out)
            vec = _vec(out)
            err, err_loop = float(np.linalg.norm(vec - want)), float(np.linalg.norm(vec - loop_vec))
            weight = out.discarded_weight
            print(f"profile {name}, trunc_thr {thr:g}, max_bond {cap}, {method}: bonds -> {out.bond_dims.tolist()}, |compressed - statement| = {err:.3g}, "
                  f"|compressed - loop| = {err_loop:.3g} (bound {bound:.3g}), discarded {weight:.6g} (statement {ref.discarded:.6g}, loop {loop.discarded_weight:.6g})")
            assert info["status"] == 0
            assert out.bond_dims.tolist() == ref.bond_dims.tolist() == loop.bond_dims.tolist()
            assert info["ranks"].tolist() == ref.bond_dims[1:n].tolist()
            assert abs(weight - ref.discarded) <= TOL and abs(weight - loop.discarded_weight) <= TOL
            assert abs(float(info["dropped"].sum()) - ref.discarded) <= TOL
            got = np.array([d.total - d.kept for d in ref.decisions])
            assert np.max(np.abs(info["dropped"] - got), initial=0.0) <= TOL
            assert err <= bound and err_loop <= bound
            lam = out.to_qiskit()[1]
            assert max([0.0] + [float(np.max(np.abs(a - b))) for a, b in zip(lam, ref.lam)]) <= bound
    finally:
        for x in made + [m]:
            x.close()


@pytest.mark.parametrize("name", ("A", "F", "pad", "D"))
def test_max_bond_three_alone(name):
    from aqc_research_amd.mps_engine import compress

    m = _device(name)
    try:
        out = compress(m, 0.0, 3)
        try:
            assert out.bond_dims.tolist() == np.minimum(_exact_bonds(name), 3).tolist()
        finally:
            out.close()
    finally:
        m.close()


def test_three_psi():
    """3 psi gives 3 x the bond vectors and the same ranks at a threshold scaled by 9."""
    from aqc_research_amd.mps_engine import DeviceMPS, compress

    gam, lam = _case("F")[0]
    thr, _, ref, gap = truncation("F", False)
    tripled = ([(3.0 * g0, 3.0 * g1) if q == 0 else (g0, g1) for q, (g0, g1) in enumerate(gam)], lam)
    one, three = DeviceMPS.from_qiskit((gam, lam), assume_canonical=True), DeviceMPS.from_qiskit(tripled, assume_canonical=True)
    made = [one, three]
    try:
        a, b = compress(one, thr), compress(three, 9.0 * thr)
        made += [a, b]
        assert a.bond_dims.tolist() == b.bond_dims.tolist() == ref.bond_dims.tolist()
        err = max(float(np.max(np.abs(3.0 * x - y))) for x, y in zip(a.to_qiskit()[1], b.to_qiskit()[1]))
        print(f"3 psi: max |3 lambda - lambda'| = {err:.3g}")
        assert err <= 3.0 * TOL / gap
        assert abs(b.discarded_weight - 9.0 * a.discarded_weight) <= 9.0 * TOL
    finally:
        for x in made:
            x.close()


def test_engine_made_state():
    """The n = 12 two-layer Trotter state, built exactly: compress(thr) leaves at the first cut the rank bond_dims_needed(thr) predicts
    (later cuts see a state already truncated on their left), at every cut the loop's bond, and the loop's overlap with the exact state."""
    from aqc_research_amd import mps_engine as me
    from aqc_research_amd.mps_observables import bond_dims_needed
    from tests.test_hip_mps_pauli import _trotter

    n = 12
    circ, th, neel = _trotter(n, layers=2)
    basis = me.DeviceMPS.basis_state(n, neel)
    exact = me.v_mul_mps(circ, th, basis, trunc_thr=1e-16, max_bond=0, method="single")
    made = [basis, exact]
    try:
        thr, ref = mps_compress_ref.pick(exact.to_qiskit(), (1e-6, 3e-6, 1e-7, 1e-5, 1e-8), False)
        dims = exact.bond_dims
        predicted, _ = bond_dims_needed(exact, thr)
        loop = _loop(exact, thr, 0)
        made.append(loop)
        want = loop.dot(exact)
        for method in ("fused", "canonical"):
            out = me.compress(exact, thr, method=method)
            made.append(out)
            got = out.dot(exact)
            print(f"Trotter n = {n}, trunc_thr {thr:g}, {method}: bonds {dims.tolist()} -> {out.bond_dims.tolist()} (needed {predicted.tolist()}), "
                  f"<compressed|exact> = {got:.12f}, loop {want:.12f}, |difference| = {abs(got - want):.3g}")
            assert out.bond_dims[1] == predicted[0]
            assert out.bond_dims.tolist() == loop.bond_dims.tolist() == ref.bond_dims.tolist()
            assert np.any(out.bond_dims < dims)
            assert abs(got - want) <= TOL
            assert abs(out.discarded_weight - loop.discarded_weight) <= TOL
    finally:
        for x in made:
            x.close()


def test_forty_qubits():
    """Beyond dense reach: n = 40, hand-made (not canonical) with bonds of 16: at trunc_thr = 0 the overlap with the input is 1 and the
    bond vectors are the input's Schmidt values."""
    from aqc_research_amd.mps_engine import DeviceMPS, compress, is_canonical
    from aqc_research_amd.mps_observables import overlaps, schmidt_values

    n = 40
    dims = [min(2 ** q, 2 ** (n - q), 16) for q in range(n + 1)]
    m = DeviceMPS.from_qiskit(mps_obs_ref.hand_made(dims, 871), assume_canonical=True)
    out = None
    try:
        out = compress(m)
        want = schmidt_values(m)
        ov = overlaps([out], [m])[0, 0]
        gam, lam = out.to_qiskit()
        err = max(float(np.max(np.abs(lam[q - 1] - want[q - 1, :dims[q]]))) for q in range(1, n))
        print(f"n = {n}, bonds of 16: <compressed|input> = {ov:.14f}, max |bond vector - Schmidt value| = {err:.3g}")
        assert out.bond_dims.tolist() == dims
        assert abs(ov - 1.0) <= TOL and err <= TOL
        assert is_canonical((gam, lam))
    finally:
        for x in (out, m):
            if x is not None:
                x.close()


def test_many_states_in_one_call():
    """40 states of profile C and a second listing of one of them: every lane has the bits of its own one-state call."""
    from aqc_research_amd.mps_engine import DeviceMPS, compress

    tuples = [mps_obs_ref.hand_made(mps_obs_ref.PROFILE_C, 900 + l) for l in range(40)]
    states = [DeviceMPS.from_qiskit(t, assume_canonical=True) for t in tuples]
    made = list(states)
    try:
        got = compress(states + [states[3]], 1e-3)
        made += got
        assert len(got) == 41 and len({x.handle.value for x in got}) == 41
        assert np.array_equal(_flat(got[40].to_qiskit()), _flat(got[3].to_qiskit())) and got[40].bond_dims.tolist() == got[3].bond_dims.tolist()
        for l in range(40):
            one = compress(states[l], 1e-3)
            try:
                assert one.bond_dims.tolist() == got[l].bond_dims.tolist() and one.discarded_weight == got[l].discarded_weight, l
                assert np.array_equal(_flat(one.to_qiskit()), _flat(got[l].to_qiskit())), l
            finally:
                one.close()
        worst, compared = 0.0, 0
        for l, t in enumerate(tuples):
            ref = mps_compress_ref.compress(t, 1e-3)
            if min(d.tail_margin for d in ref.decisions) >= mps_trunc_ref.MIN_MARGIN:
                assert got[l].bond_dims.tolist() == ref.bond_dims.tolist(), l
                gaps = mps_compress_ref.gaps(ref.decisions, mps_compress_ref.spectra(t, 1e-3))
                if not gaps or min(gaps) >= MIN_GAP:
                    compared += 1
                    worst = max(worst, float(np.linalg.norm(_vec(got[l]) - ref.to_vector())) * (min(gaps) if gaps else 1.0))
        print(f"40 states of profile C at trunc_thr 1e-3: {compared} compared, max |compressed - statement| x gap = {worst:.3g}")
        assert compared >= COMPARED_MIN and worst <= TOL
    finally:
        for x in made:
            x.close()


def test_chunks_of_states_give_the_same_bits():
    """The sweep runs in chunks of states that fit the SVD budget (512 states or more by default).  With the budget lowered to 3 states
    and to 1 state per chunk the 41 lanes have the bits of the call that takes them in one chunk."""
    from aqc_research_amd import _lib
    from aqc_research_amd.mps_engine import DeviceMPS, compress

    L = _lib.lib()
    states = [DeviceMPS.from_qiskit(mps_obs_ref.hand_made(mps_obs_ref.PROFILE_C, 900 + l), assume_canonical=True) for l in range(40)]
    made = list(states)
    per_state = 8 * 16 * 3 * 3   # mps_compress_chunk at K = 3
    try:
        whole, info = compress(states + [states[3]], 1e-3, details=True)
        made += whole
        default = L.aqc_mps_compress_svd_budget(3 * per_state + 7)
        assert default == 256 << 20
        for chunk in (3, 1):
            assert L.aqc_mps_compress_svd_budget(chunk * per_state + 7) > 0
            got, again = compress(states + [states[3]], 1e-3, details=True)
            made += got
            for key in ("ranks", "dropped", "sweeps", "status"):
                assert np.array_equal(info[key], again[key]), (chunk, key)
            for l in range(41):
                assert np.array_equal(_flat(got[l].to_qiskit()), _flat(whole[l].to_qiskit())), (chunk, l)
                assert got[l].discarded_weight == whole[l].discarded_weight
    finally:
        L.aqc_mps_compress_svd_budget(0)
        for x in made:
            x.close()
    assert L.aqc_mps_compress_svd_budget(0) == 256 << 20


_LANE_SIZE = 7 * 2 * 96 * 96   # room for every site of a lane state at its input bonds


def _lane_outputs(results, info):
    sites = np.zeros((len(results), _LANE_SIZE), dtype=np.complex128)
    for l, out in enumerate(results):
        if out is None:
            sites[l] = np.nan
            continue
        flat = _flat(out.to_qiskit())
        sites[l, :flat.size] = flat
        out.close()
    return {"state": sites, "ranks": info["ranks"], "dropped": info["dropped"], "status": info["status"]}


@pytest.mark.parametrize("method", ("fused", "canonical"))
def test_lanes_hold_the_lane_contract(method):
    """Four states, probes (0, 3), at a threshold that cuts.  F: neighbours with other bonds of the same route; N: every neighbour holds
    NaN tensors, gets status 2 and no state, and the probes' bits do not move."""
    from aqc_research_amd.mps_engine import DeviceMPS, compress, compress_route

    mine, theirs = ("A", "A2") if method == "fused" else ("D", "D2")
    made = []

    def device(profile, seed, nan=False):
        gam, lam = _lane_mps(profile, seed)
        if nan:
            gam = [(g0 * np.nan, g1 * np.nan) for g0, g1 in gam]
        made.append(DeviceMPS.from_qiskit((gam, lam), assume_canonical=True))
        return made[-1]

    def run(states):
        results, info = compress(states, 1e-4, details=True)
        return _lane_outputs(results, info)

    try:
        states = [device(mine, 880 + l) for l in range(4)]
        poison = [device(mine, 880 + l, nan=True) for l in range(4)]
        assert all(compress_route(m.bond_dims) == method for m in states)
        base = check_lanes(run, states, probes=(0, 3), other=[device(theirs, 890 + l) for l in range(4)], poison=poison, distinct=("state",))
        assert np.all(base["status"] == 0) and np.all(base["ranks"] >= 1)
        results, info = compress([states[0], poison[1], poison[2], states[3]], 1e-4, details=True)
        assert results[1] is None and results[2] is None and info["status"].tolist() == [0, 2, 2, 0] and info["route"] == [method] * 4
        assert np.all(info["ranks"][1:3] == 0)
        for l in (0, 3):
            assert np.array_equal(_flat(results[l].to_qiskit()), base["state"][l, :_flat(results[l].to_qiskit()).size])
            results[l].close()
        with pytest.raises(RuntimeError, match="state 1, cut 1"):
            compress([states[0], poison[1]], 1e-4)
    finally:
        for m in made:
            m.close()


def test_in_place():
    from aqc_research_amd.mps_engine import compress

    thr, _, ref, _ = truncation("F", False)
    m, other = _device("F"), None
    try:
        other = compress(m, thr)
        version, serial = m.version, m.serial
        assert m.compress(thr) is m
        assert m.version == version + 1 and m.serial == serial and m.handle
        assert m.bond_dims.tolist() == ref.bond_dims.tolist() == other.bond_dims.tolist()
        assert np.array_equal(_flat(m.to_qiskit()), _flat(other.to_qiskit()))
        vals = m.schmidt_values()
        assert vals.shape == (12, int(max(ref.bond_dims)))
        lam = m.to_qiskit()[1]   # (a bond vector holds the values of its cut when it was made; only the last cut saw no later one)
        assert float(np.max(np.abs(vals[11, :lam[11].size] - lam[11]))) <= TOL and np.all(vals[11, lam[11].size:] == 0.0)
        assert all(np.all(vals[q, lam[q].size:] == 0.0) for q in range(12))
    finally:
        for x in (m, other):
            if x is not None:
                x.close()


def test_refusals_leave_no_buffers_and_a_correct_call_follows():
    from ctypes import c_void_p

    from aqc_research_amd import _lib
    from aqc_research_amd.engine import live_buffers
    from aqc_research_amd.mps_engine import DeviceMPS, compress

    L = _lib.lib()
    a, d, five = _device("C"), _device("D"), DeviceMPS.basis_state(5)
    out_ok = None
    try:
        hs, out = (c_void_p * 2)(a.handle, a.handle), (c_void_p * 2)()
        ranks, sweeps, status, dropped = np.zeros((2, 3), np.int32), np.zeros((2, 3), np.int32), np.zeros(2, np.int32), np.zeros((2, 3))

        def call(states, nstates, thr=0.0, cap=0, method=0, dst=out):
            return L.aqc_mps_compress(states, nstates, thr, cap, method, dst, _lib.iptr(ranks), _lib.dptr(dropped), _lib.iptr(sweeps), _lib.iptr(status))

        live = live_buffers()
        assert call(None, 2) == 1 and call(hs, 2, dst=None) == 1 and call(hs, 0) == 1 and call(hs, 2, method=3) == 1
        assert call((c_void_p * 2)(a.handle, None), 2) == 1
        assert call((c_void_p * 2)(a.handle, five.handle), 2) == 1 and b"differ" in L.aqc_last_error()            # mixed n
        assert call((c_void_p * 1)(d.handle), 1, method=1) == 1 and b"fused" in L.aqc_last_error()                # beyond the cap
        assert call(hs, 2, cap=-1) == 1 and b"max_bond" in L.aqc_last_error()
        assert call(hs, 2, thr=-1e-3) == 1 and b"trunc_thr" in L.aqc_last_error()
        assert call(hs, 2, thr=float("nan")) == 1 and b"trunc_thr" in L.aqc_last_error()
        assert out[0] is None and out[1] is None and live_buffers() == live
        closed = _device("C")
        closed.close()
        for bad in (lambda: compress([a, five]), lambda: compress([a, closed]), lambda: compress(d, method="fused"), lambda: compress(a, 0.0, -1),
                    lambda: compress(a, -1e-3), lambda: compress(_case("D")[0], method="fused"), lambda: compress(a, method="gemm")):
            with pytest.raises(ValueError):
                bad()
        assert live_buffers() == live
        out_ok = compress(a)
        assert float(np.linalg.norm(_vec(out_ok) - _dense("C"))) <= TOL and out_ok.bond_dims.tolist() == _exact_bonds("C")
        out_ok.close()
        out_ok = None
        assert call(hs, 2) == 0 and out[0] and out[1] and out[0] != out[1] and status.tolist() == [0, 0]
        assert ranks.tolist() == [_exact_bonds("C")[1:4]] * 2
        for h in out:
            assert L.aqc_mps_destroy(c_void_p(h)) == 0
        assert live_buffers() == live
    finally:
        for m in (a, d, five, out_ok):
            if m is not None:
                m.close()
