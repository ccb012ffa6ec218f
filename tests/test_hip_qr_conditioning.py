"""The device's CholeskyQR2 (csrc/aqc_sketch.hip: aqc_qr, aqc_ws_sketch_generate) where its answer depends on the input's conditioning:
row counts that end in a short slab, a ladder of condition numbers, a family that straddles the status rule, column scaling,
non-finite entries and the `eigen` generator close to convergence.  The reference for the range is modified Gram-Schmidt in extended
precision (tests/sketch_ref.py: extended_range_basis); the status rule is stated in NumPy there (cholesky_qr2_rule)."""
from ctypes import byref, c_int32

import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests import sketch_ref as sk
from tests.helpers import TOL, maxdiff

pytestmark = pytest.mark.gpu

EPS = 2.2e-16


def _rand_c(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _qr_status(a):
    """(q, status) of aqc_qr through its status word: a flagged matrix is returned, not raised."""
    from aqc_research_amd import _lib
    from aqc_research_amd.engine import default_device

    a = _lib.as_c128(a)
    q, st = np.empty_like(a), c_int32(0)
    _lib.check(_lib.lib().aqc_qr(default_device(), a.shape[0], a.shape[1], _lib.dptr(a), _lib.dptr(q), byref(st)))
    return q, int(st.value)


def _orth(q):
    return maxdiff(np.conj(q.T) @ q, np.eye(q.shape[1]))


def _range_gap(q, a):
    ref = sk.extended_range_basis(a)
    return maxdiff(q @ np.conj(q.T), ref @ np.conj(ref.T))


def _workspace(n, k, lanes, seed):
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.engine import HipContext, Workspace

    rng = np.random.default_rng(seed)
    circ = ParametricCircuit(n, "cz", orc.spin_blocks(n, 2 * n + 2))
    thetas = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(lanes)])
    return circ, thetas, Workspace(HipContext.of(circ), batch=lanes, ncols=k), rng


@pytest.mark.parametrize("m,k", [(5, 4), (17, 16), (65, 16), (100, 32), (130, 64), (1027, 8)])
def test_ragged_row_counts(m, k):
    """Row counts that are no multiple of 4, 16 or 64: the r < d guards of the gram and apply kernels and the short last slab.
    A workspace has d = 2^n rows, so these shapes reach the kernels through the single call only; that a lane of a batch equals
    the single call bit for bit is asserted at d = 32 in test_hip_sketched.py and, with a flagged neighbour, below."""
    from aqc_research_amd.engine import qr

    a = _rand_c(np.random.default_rng(1000 * m + k), m, k)
    q = qr(a)
    e_orth, e_proj = _orth(q), _range_gap(q, a)
    print(f"qr {m}x{k}: |Q^H Q - I| = {e_orth:.2e}, |Q Q^H - Qref Qref^H| = {e_proj:.2e}")
    assert e_orth < 1e-12
    assert e_proj < TOL
    assert np.array_equal(q, qr(a))


@pytest.mark.parametrize("kappa", [1e2, 1e3, 1e4])
@pytest.mark.parametrize("spectrum", ["geometric", "last"])
@pytest.mark.parametrize("d,k", [(64, 16), (100, 16), (256, 64)])
def test_conditioning_ladder(d, k, spectrum, kappa):
    """Prescribed singular values, Haar vectors.  A pivot ratio is at least (s_min / s_max)^2 >= 1e-8 and eps kappa^2 <= 2.2e-8 is far
    below the second pass's 1e-4: no lane here may be flagged.  The range of a matrix of condition kappa is determined to
    O(eps kappa); CholeskyQR2 in NumPy stays below 1e-3 of the bound asserted."""
    from aqc_research_amd.engine import qr

    s = np.geomspace(1.0, 1.0 / kappa, k) if spectrum == "geometric" else np.r_[np.ones(k - 1), 1.0 / kappa]
    a = sk.with_spectrum(d, k, s, np.random.default_rng(int(d + k + np.log10(kappa))))[0]
    q = qr(a)                                   # raises if the lane is flagged
    e_orth, e_proj, bound = _orth(q), _range_gap(q, a), 64 * EPS * kappa
    print(f"qr {d}x{k} {spectrum} kappa={kappa:.0e}: |Q^H Q - I| = {e_orth:.2e}, range gap = {e_proj:.2e} = {e_proj / bound:.2e} of 64 eps kappa")
    assert e_orth < 1e-12
    assert e_proj <= bound


def test_status_contract_on_a_family_that_straddles_the_threshold():
    """Kahan matrices (every pivot ratio benign, condition number up to 1e17) and graded spectra.  Each matrix either comes back
    with status 0, orthonormal to 1e-12 and with the range to 64 eps kappa_eq (kappa_eq: condition number with the columns scaled
    to norm 1; accepted only while that bound is below 1e-6), or flagged and unchanged bit for bit.  kappa_eq <= 1e4 must take the
    first outcome and kappa_eq >= 1e14 the second, and both sets occur.  Before the second pass tested |G2 - I| the NumPy statement
    of the rule returned status 0 with |Q^H Q - I| = 7e-9 for kahan(64, 32, 0.75) and status 0 at kappa_eq = 2.6e9 (theta = 0.95)."""
    from aqc_research_amd.engine import RankDeficientSketch, qr

    wrong, accepted, flagged, must_accept, must_flag = [], 0, 0, 0, 0
    for name, a in sk.straddling_family():
        keq = sk.cond_equilibrated(a)
        q, st = _qr_status(a)
        bound = 64 * EPS * keq
        if st == 0:
            accepted += 1
            e_orth, e_proj = _orth(q), _range_gap(q, a)
            print(f"{name}: kappa_eq = {keq:.2e}, status 0, |Q^H Q - I| = {e_orth:.2e}, range gap = {e_proj:.2e} ({e_proj / bound:.2e} of the bound)")
            if not (bound < 1e-6 and e_orth < 1e-12 and e_proj <= bound):
                wrong.append(f"{name}: status 0 at kappa_eq = {keq:.2e} with |Q^H Q - I| = {e_orth:.2e}, range gap = {e_proj:.2e}")
        else:
            flagged += 1
            print(f"{name}: kappa_eq = {keq:.2e}, flagged")
            if st != sk.QR_RANK_DEFICIENT or not np.array_equal(q, a):
                wrong.append(f"{name}: status {st}, matrix unchanged: {np.array_equal(q, a)}")
            with pytest.raises(RankDeficientSketch):
                qr(a)
        if keq <= 1e4:
            must_accept += 1
            if st != 0:
                wrong.append(f"{name}: flagged at kappa_eq = {keq:.2e}")
        if keq >= 1e14:
            must_flag += 1
            if st == 0:
                wrong.append(f"{name}: status 0 at kappa_eq = {keq:.2e}")
    print(f"accepted {accepted}, flagged {flagged}; kappa_eq <= 1e4: {must_accept}, kappa_eq >= 1e14: {must_flag}")
    assert must_accept > 0 and must_flag > 0
    assert not wrong, "\n".join(wrong)


def test_power_of_two_column_scaling_changes_no_bit():
    """Column j times 2^e_j, e_j over [-100, 100]: Gram matrix, Cholesky, triangular solve and A R^-1 all commute exactly with it
    (squared norms reach 2^+-200, inside the double range), and the tests on pivots and on G2 - I are relative: the same Q."""
    rng = np.random.default_rng(44)
    a = _rand_c(rng, 128, 16)
    e = rng.permutation(np.round(np.linspace(-100, 100, 16)).astype(int))
    q0, st0 = _qr_status(a)
    q1, st1 = _qr_status(a * np.ldexp(1.0, e))
    assert st0 == 0 and st1 == 0
    assert _orth(q0) < 1e-12
    assert np.array_equal(q0, q1)


@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_a_non_finite_entry_flags_its_lane_alone(poison):
    from aqc_research_amd.engine import BUF_X, BUF_Y, qr

    n, k, lanes = 5, 8, 3
    circ, thetas, ws, rng = _workspace(n, k, lanes, 8)
    d = 1 << n
    targets = np.stack([np.linalg.qr(_rand_c(rng, d, d))[0] for _ in range(lanes)])
    ws.sketch_target(targets)
    mats = _rand_c(rng, lanes, d, k)
    mats[1, 11, 3] = poison
    st = ws.sketch_generate("rand", omega=mats)
    x, y = ws.download(BUF_X), ws.download(BUF_Y)
    ws.close()
    assert [int(s) for s in st] == [0, sk.QR_RANK_DEFICIENT, 0]
    assert np.array_equal(x[1], mats[1], equal_nan=True)
    for b in (0, 2):
        assert np.array_equal(x[b], qr(mats[b]))
        assert np.all(np.isfinite(y[b])) and maxdiff(y[b], targets[b] @ x[b]) < TOL


def test_eigen_close_to_convergence():
    """Targets U_b = V(theta_b) exp(i eps_b H), |H|_2 = 1, eps = (1e-3, 1e-7, 1e-13): (V^H - U^H) Omega has scale eps.  The first
    two are ranges to orthonormalise.  In the third a column's squared norm is at most eps^2 * 2 d = 3.2e-25, below the absolute
    floor 2 d * 1e-24 of the eigen assembly: that lane, and it alone, is flagged.  (No comparison of ranges: the difference itself
    carries a cancellation error of eps_machine / eps.)"""
    from aqc_research_amd.engine import BUF_X, BUF_Y

    n, k, lanes = 4, 4, 3
    circ, thetas, ws, rng = _workspace(n, k, lanes, 31)
    d = 1 << n
    h = _rand_c(rng, d, d)
    lam, w = np.linalg.eigh(h + np.conj(h.T))
    lam = lam / np.max(np.abs(lam))
    targets = np.stack([orc.v_mul_mat(circ, thetas[b], np.eye(d, dtype=np.complex128)) @ ((w * np.exp(1j * e * lam)) @ np.conj(w.T))
                        for b, e in enumerate((1e-3, 1e-7, 1e-13))])
    ws.sketch_target(targets)
    ws.set_thetas(thetas)
    st = ws.sketch_generate("eigen", omega=_rand_c(rng, lanes, d, k))
    x, y = ws.download(BUF_X), ws.download(BUF_Y)
    ws.close()
    assert [int(s) for s in st] == [0, 0, sk.QR_RANK_DEFICIENT]
    for b in (0, 1):
        print(f"eigen lane {b}: |X^H X - I| = {_orth(x[b]):.2e}, |Y - U X| = {maxdiff(y[b], targets[b] @ x[b]):.2e}")
        assert _orth(x[b]) < 1e-12
        assert maxdiff(y[b], targets[b] @ x[b]) < TOL
