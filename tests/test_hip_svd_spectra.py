"""The one-sided Jacobi SVD of the MPS engine (csrc/aqc_svd.hip, jacobi_lds_sweeps of csrc/aqc_mps_dev.h, aqc_svd) on the spectra
two-site tensors have -- repeated values, clusters, gradings over many decades, exact rank deficiency, columns that are orthogonal
already -- on each of its three routes.  Inputs are built from prescribed singular values and Haar vectors (tests/sketch_ref.py:
with_spectrum), so values and vectors are compared with what was prescribed, not with another library's rounding; LAPACK's gesvd is
run alongside and its distance to the same bounds printed."""
import functools
import os

import numpy as np
import pytest

from tests import sketch_ref as sk
from tests.helpers import maxdiff

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
# route -> (AQC_SVD_BLOCKED, shapes): one workgroup in LDS (rows, cols <= 64); the persistent two-level kernel (nine column blocks =
# an odd tournament; 66 columns = a ragged last block, also through mode 1); one launch per round (rows > 512, or the switch)
ROUTES = {"lds": (None, [(24, 24), (64, 40)]), "two-level": (None, [(96, 72), (130, 66), (66, 130)]),
          "round-per-launch": (None, [(520, 16)]), "round-per-launch-forced": ("0", [(96, 72)])}
ROUTE_SHAPES = [(r, s) for r, (_, shapes) in ROUTES.items() for s in shapes]
CASES = ["equal", "clusters", "graded", "graded-negligible", "rank-half", "diagonal", "permuted-diagonal"]


def _spectrum(case, k):
    if case == "equal":
        return np.full(k, 0.7)
    if case == "clusters":      # groups of four equal values 1, 0.8, .., 0.2, then 1 again: every gap is 0.2 s0 whatever k
        return np.sort(1.0 - 0.2 * ((np.arange(k) // 4) % 5))[::-1]
    if case == "graded":
        return np.geomspace(1.0, 1e-12, k)
    if case == "graded-negligible":
        return np.geomspace(1.0, 1e-22, k)
    if case == "rank-half":
        return np.r_[np.linspace(1.0, 0.5, k // 2), np.zeros(k - k // 2)]
    raise ValueError(case)


def _input(case, m, n):
    """(a, s_true descending, U, V) -- U, V None where the case prescribes no vectors."""
    k = min(m, n)
    rng = np.random.default_rng(1000 * m + n + 7 * CASES.index(case))
    if case in ("diagonal", "permuted-diagonal"):
        dvals = rng.permutation(np.linspace(0.1, 1.0, k))
        a = np.zeros((m, n), dtype=np.complex128)
        if case == "diagonal":
            a[np.arange(k), np.arange(k)] = dvals * rng.choice([-1.0, 1.0], k)
        else:
            a[np.arange(k), np.arange(k)] = dvals * np.exp(2j * np.pi * rng.random(k))
            a = a[rng.permutation(m)][:, rng.permutation(n)]
        return np.ascontiguousarray(a), np.sort(dvals)[::-1], None, None
    s = _spectrum(case, k)
    a, u, v = sk.with_spectrum(m, n, s, rng)
    if case == "rank-half":
        perm = rng.permutation(n)
        a, v = np.ascontiguousarray(a[:, perm]), v[perm]
    return a, s, u, v


@functools.lru_cache(maxsize=None)
def _run(route, shape, case, scale_exp=0):
    """One device SVD, computed once and read by every test that needs it."""
    from aqc_research_amd.mps_engine import svd

    a, s_true, u_true, v_true = _input(case, *shape)
    keep, want = os.environ.get("AQC_SVD_BLOCKED"), ROUTES[route][0]
    try:
        if want is not None:
            os.environ["AQC_SVD_BLOCKED"] = want
        u, s, vh, sweeps = svd(a * np.ldexp(1.0, scale_exp))
    finally:
        if want is not None:
            if keep is None:
                del os.environ["AQC_SVD_BLOCKED"]
            else:
                os.environ["AQC_SVD_BLOCKED"] = keep
    return {"a": a, "s_true": s_true, "u_true": u_true, "v_true": v_true, "u": u, "s": s, "vh": vh, "sweeps": int(sweeps)}


def _clusters(s_true):
    """index sets of equal prescribed values and each one's distance to the nearest other value (zero included)"""
    out, start = [], 0
    for j in range(1, len(s_true) + 1):
        if j == len(s_true) or s_true[j] != s_true[start]:
            others = np.r_[s_true[:start], s_true[j:], 0.0]
            out.append((np.arange(start, j), float(np.min(np.abs(others - s_true[start])))))
            start = j
    return out


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("route,shape", ROUTE_SHAPES)
def test_prescribed_spectrum(route, shape, case):
    """Convergence (fewer than the 60 sweeps that mean "none"), singular values against the prescribed ones to the normwise bound of
    one-sided Jacobi, 8 k eps s0, reconstruction to the same bound, orthonormal vectors over the values above 1e-12 s0, and, where
    the vectors are determined (equal values, clusters), the projector of every cluster to 8 k eps s0 / gap.  In the graded case
    that runs past kNegligible2 (1e-22 s0) the values below 1e-15 s0 carry no relative information and are held to the absolute
    bound alone, like all others.  Columns that are orthogonal on entry take one sweep and come back as phased permutations."""
    import scipy.linalg

    m, n = shape
    k = min(m, n)
    r = _run(route, shape, case)
    a, s_true, u, s, vh, sweeps = r["a"], r["s_true"], r["u"], r["s"], r["vh"], r["sweeps"]
    s0, bound = s_true[0], 8 * k * EPS * s_true[0]
    e_s = maxdiff(s, s_true)
    e_lapack = maxdiff(scipy.linalg.svd(a, compute_uv=False, lapack_driver="gesvd"), s_true)
    e_rec = maxdiff((u * s) @ vh, a)
    good = s > 1e-12 * s0
    ng = int(good.sum())
    e_u = maxdiff(np.conj(u[:, good].T) @ u[:, good], np.eye(ng))
    e_v = maxdiff(vh[good] @ np.conj(vh[good].T), np.eye(ng))
    print(f"svd {route} {m}x{n} {case}: sweeps {sweeps}, |s - s_true| / bound: device {e_s / bound:.3f}, gesvd {e_lapack / bound:.3f}; "
          f"reconstruction / bound {e_rec / bound:.3f}; orthonormality / (8 k eps): u {e_u / (8 * k * EPS):.3f}, vh {e_v / (8 * k * EPS):.3f}")
    assert 0 < sweeps < 60
    assert np.all(np.diff(s) <= 1e-13 * s0)
    assert e_s <= bound
    assert e_rec <= bound
    assert e_u <= 8 * k * EPS and e_v <= 8 * k * EPS
    if case == "rank-half":
        assert ng == k // 2
    if case in ("diagonal", "permuted-diagonal"):
        assert sweeps == 1
        assert np.all(np.diff(s) <= 0)
        for name, mat in (("u", u), ("vh", vh.T)):          # columns: one entry of modulus 1, in a row of its own
            hot = np.abs(mat) > 0.5
            assert maxdiff(np.abs(mat), hot.astype(float)) <= 1e-15, name
            assert np.all(hot.sum(axis=0) == 1) and np.all(hot.sum(axis=1) <= 1), name
    if case in ("equal", "clusters"):
        for idx, gap in _clusters(s_true):
            tol = bound / gap
            e_pu = maxdiff(u[:, idx] @ np.conj(u[:, idx].T), r["u_true"][:, idx] @ np.conj(r["u_true"][:, idx].T))
            e_pv = maxdiff(np.conj(vh[idx].T) @ vh[idx], r["v_true"][:, idx] @ np.conj(r["v_true"][:, idx].T))
            print(f"    cluster s = {s_true[idx[0]]:.1f} x {len(idx)}: projector error / (8 k eps s0 / gap): left {e_pu / tol:.3f}, right {e_pv / tol:.3f}")
            assert e_pu <= tol and e_pv <= tol


@pytest.mark.parametrize("case", ["clusters", "graded", "rank-half"])
def test_two_level_kernel_agrees_with_round_per_launch(case):
    blocked, plain = _run("two-level", (96, 72), case), _run("round-per-launch-forced", (96, 72), case)
    s0 = blocked["s_true"][0]
    e_s = maxdiff(blocked["s"], plain["s"])
    e_rec = maxdiff((blocked["u"] * blocked["s"]) @ blocked["vh"], (plain["u"] * plain["s"]) @ plain["vh"])
    print(f"96x72 {case}: two-level against round per launch: |s - s'| = {e_s:.2e}, |reconstructions| = {e_rec:.2e}")
    assert e_s <= 1e-12 * s0 and e_rec <= 1e-12 * s0


@pytest.mark.parametrize("exp2", [-100, 100])
@pytest.mark.parametrize("route,shape", [("lds", (24, 24)), ("two-level", (96, 72)), ("round-per-launch", (520, 16))])
def test_power_of_two_scaling(route, shape, exp2):
    """svd(2^e a), e = +-100 (the documented reach of aqc_svd is |e| < 250: beyond, |gamma|^2 leaves the double range)."""
    base, scaled = _run(route, shape, "graded"), _run(route, shape, "graded", exp2)
    k, s0 = min(shape), base["s_true"][0]
    bound = 8 * k * EPS * s0
    s_back = np.ldexp(scaled["s"], -exp2)
    rec, rec_back = (base["u"] * base["s"]) @ base["vh"], (scaled["u"] * s_back) @ scaled["vh"]
    same = np.array_equal(s_back, base["s"]) and np.array_equal(scaled["u"], base["u"]) and np.array_equal(scaled["vh"], base["vh"])
    print(f"svd {route} {shape} x 2^{exp2}: sweeps {scaled['sweeps']} (unscaled {base['sweeps']}), |s 2^-e - s| / bound = "
          f"{maxdiff(s_back, base['s']) / bound:.3f}, reconstruction / bound = {maxdiff(rec_back, rec) / bound:.3f}, bit-identical: {same}")
    assert 0 < scaled["sweeps"] < 60
    assert maxdiff(s_back, base["s"]) <= bound
    assert maxdiff(rec_back, rec) <= bound
