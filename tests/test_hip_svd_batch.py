"""mps_engine.svd_batch / aqc_svd_batch (csrc/aqc_svd_batch.hip: block one-sided Jacobi on the fp64 matrix cores, a workgroup per matrix)
on the spectra, helpers and bounds of tests/test_hip_svd_spectra.py, at the smallest shapes at which each piece of the kernel can go
wrong: one block (16 x 16), one pair (32 x 32), a bye and a ragged last block (48 x 40), ragged in both directions (130 x 66), the
transposed route (66 x 130) and the largest sizes (256 x 128, 256 x 256).  The seven spectra of a shape go through ONE call, computed
once and read by every test.

The Newton-Schulz step on each panel's J is what the two largest shapes need: without it V collects J's rounding at every visit and
the NumPy statement of the rule leaves |V V^H - 1| at 1.3 .. 2.3 times 8 k eps for ``graded``, ``graded-negligible`` and ``clusters``
there; with it 0.02 (tests/test_svd_block_host.py)."""
import ctypes
import functools

import numpy as np
import pytest

from tests.helpers import maxdiff
from tests.test_hip_svd_spectra import CASES, EPS, _clusters, _input

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16), (32, 32), (48, 40), (130, 66), (66, 130), (256, 128), (256, 256)]
MIXED = [(1, 1), (16, 16), (48, 40), (130, 66), (66, 130), (130, 130)]


def _live():
    from aqc_research_amd.engine import live_buffers

    return live_buffers()


@functools.lru_cache(maxsize=None)
def _run(shape, scale_exp=0):
    """the seven spectra of one shape in one call"""
    from aqc_research_amd.mps_engine import svd_batch

    inputs = [_input(case, *shape) for case in CASES]
    u, s, vh, sweeps, status = svd_batch(np.stack([np.ldexp(1.0, scale_exp) * i[0] for i in inputs]))
    return inputs, u, s, vh, sweeps, status


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_prescribed_spectrum(shape, case):
    """The checks and bounds of test_hip_svd_spectra.test_prescribed_spectrum, per matrix of the batch."""
    m, n = shape
    k, i = min(m, n), CASES.index(case)
    inputs, ub, sb, vhb, sweeps, status = _run(shape)
    (a, s_true, u_true, v_true), u, s, vh = inputs[i], ub[i], sb[i], vhb[i]
    s0, bound = s_true[0], 8 * k * EPS * s_true[0]
    e_s, e_rec = maxdiff(s, s_true), maxdiff((u * s) @ vh, a)
    good = s > 1e-12 * s0
    ng = int(good.sum())
    e_u = maxdiff(np.conj(u[:, good].T) @ u[:, good], np.eye(ng))
    e_v = maxdiff(vh[good] @ np.conj(vh[good].T), np.eye(ng))
    print(f"svd_batch {m}x{n} {case}: sweeps {sweeps[i]}, status {status[i]}, |s - s_true| / bound {e_s / bound:.3f}; reconstruction / bound "
          f"{e_rec / bound:.3f}; orthonormality / (8 k eps): u {e_u / (8 * k * EPS):.3f}, vh {e_v / (8 * k * EPS):.3f}")
    assert status[i] == 0 and 0 < sweeps[i] < 60
    assert np.all(np.diff(s) <= 1e-13 * s0)
    assert e_s <= bound
    assert e_rec <= bound
    assert e_u <= 8 * k * EPS and e_v <= 8 * k * EPS
    if case == "rank-half":
        assert ng == k // 2
    if case in ("diagonal", "permuted-diagonal"):
        assert sweeps[i] == 1
        assert np.all(np.diff(s) <= 0)
        for name, mat in (("u", u), ("vh", vh.T)):
            hot = np.abs(mat) > 0.5
            assert maxdiff(np.abs(mat), hot.astype(float)) <= 1e-15, name
            assert np.all(hot.sum(axis=0) == 1) and np.all(hot.sum(axis=1) <= 1), name
    if case in ("equal", "clusters"):
        for idx, gap in _clusters(s_true):
            tol = bound / gap
            e_pu = maxdiff(u[:, idx] @ np.conj(u[:, idx].T), u_true[:, idx] @ np.conj(u_true[:, idx].T))
            e_pv = maxdiff(np.conj(vh[idx].T) @ vh[idx], v_true[:, idx] @ np.conj(v_true[:, idx].T))
            print(f"    cluster s = {s_true[idx[0]]:.1f} x {len(idx)}: projector error / (8 k eps s0 / gap): left {e_pu / tol:.3f}, right {e_pv / tol:.3f}")
            assert e_pu <= tol and e_pv <= tol


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", SHAPES)
def test_agrees_with_the_existing_routes(shape, case):
    from aqc_research_amd.mps_engine import svd

    i = CASES.index(case)
    inputs, _, sb, _, _, _ = _run(shape)
    s_one = svd(inputs[i][0])[1]
    bound = 8 * min(shape) * EPS * inputs[i][1][0]
    print(f"svd_batch against svd {shape} {case}: |s - s'| / bound = {maxdiff(sb[i], s_one) / bound:.3f}")
    assert maxdiff(sb[i], s_one) <= bound


@functools.lru_cache(maxsize=None)
def _mixed():
    """(store, rows, cols): m = n = 130 with the active sizes of MIXED, then an all-zero matrix and a rank-half one"""
    mats = [_input("clusters" if min(r, c) >= 4 else "diagonal", r, c)[0] for r, c in MIXED] + [np.zeros((40, 24), dtype=np.complex128), _input("rank-half", 96, 72)[0]]
    store = np.zeros((len(mats), 130, 130), dtype=np.complex128)
    for i, a in enumerate(mats):
        store[i, :a.shape[0], :a.shape[1]] = a
    return store, np.array([a.shape[0] for a in mats], dtype=np.int32), np.array([a.shape[1] for a in mats], dtype=np.int32)


def _alone(store, rows, cols, i):
    from aqc_research_amd.mps_engine import svd_batch

    return svd_batch(store[i:i + 1], rows[i:i + 1], cols[i:i + 1])


def test_one_call_mixed_sizes_is_bitwise_each_matrix_alone():
    from aqc_research_amd.mps_engine import svd_batch

    store, rows, cols = _mixed()
    u, s, vh, sweeps, status = svd_batch(store, rows, cols)
    assert np.all(status == 0)
    for i in range(len(rows)):
        r, c = int(rows[i]), int(cols[i])
        k = min(r, c)
        one = _alone(store, rows, cols, i)
        for name, got, want in (("u", u[i], one[0][0]), ("s", s[i], one[1][0]), ("vh", vh[i], one[2][0])):
            assert np.array_equal(got, want), (i, name)
        assert sweeps[i] == one[3][0] and status[i] == one[4][0]
        assert not u[i, r:].any() and not u[i, :, k:].any() and not s[i, k:].any() and not vh[i, k:].any() and not vh[i, :, c:].any(), i   # the padding
        a = store[i, :r, :c]
        assert maxdiff((u[i, :r, :k] * s[i, :k]) @ vh[i, :k, :c], a) <= 8 * 130 * EPS * max(float(s[i, 0]), 1.0), i
    z = len(MIXED)                                      # the all-zero matrix: zero singular values, no left vectors, V = 1
    assert not s[z].any() and not u[z].any() and np.array_equal(vh[z, :24, :24], np.eye(24))


def test_non_finite_matrices_are_flagged_and_leave_their_neighbours_alone():
    from aqc_research_amd.mps_engine import svd_batch

    store, rows, cols = _mixed()
    base = svd_batch(store, rows, cols)
    dirty = store.copy()
    dirty[2, 5, 7] = np.nan
    dirty[4, 0, 0] = complex(0.0, np.inf)
    u, s, vh, sweeps, status = svd_batch(dirty, rows, cols)
    assert list(status) == [0, 0, 2, 0, 2, 0, 0, 0]
    for i in (2, 4):
        assert not u[i].any() and not s[i].any() and not vh[i].any()
    for i in (0, 1, 3, 5, 6, 7):
        assert np.array_equal(u[i], base[0][i]) and np.array_equal(s[i], base[1][i]) and np.array_equal(vh[i], base[2][i]) and sweeps[i] == base[3][i], i


def test_argument_errors_raise():
    from aqc_research_amd import _lib
    from aqc_research_amd.mps_engine import svd_batch

    good = np.zeros((2, 4, 3), dtype=np.complex128)
    with pytest.raises(ValueError):
        svd_batch(good, rows=[4, 5])
    with pytest.raises(TypeError):
        svd_batch(good.real)
    L, i32 = _lib.lib(), ctypes.POINTER(ctypes.c_int32)
    u, s, vh, st = np.zeros((2, 4, 3), dtype=np.complex128), np.zeros((2, 3)), np.zeros((2, 3, 3), dtype=np.complex128), np.zeros(2, dtype=np.int32)
    bad_rows = np.array([4, 5], dtype=np.int32)
    args = (_lib.dptr(good), _lib.dptr(u), _lib.dptr(s), _lib.dptr(vh), None, st.ctypes.data_as(i32))
    assert L.aqc_svd_batch(0, 0, 4, 3, None, None, *args) != 0
    assert L.aqc_svd_batch(0, 2, 257, 3, None, None, *args) != 0
    assert L.aqc_svd_batch(0, 2, 4, 3, bad_rows.ctypes.data_as(i32), None, *args) != 0
    assert b"rows[1]" in L.aqc_last_error()
    assert L.aqc_svd_batch(0, 2, 4, 3, None, None, _lib.dptr(good), _lib.dptr(u), _lib.dptr(s), _lib.dptr(vh), None, None) != 0


@pytest.mark.parametrize("exp2", [-100, 100])
def test_power_of_two_scaling(exp2):
    """2^+-100 on ``clusters`` at 48 x 40 (the documented range of aqc_svd): the same relative results."""
    shape, i = (48, 40), CASES.index("clusters")
    (inputs, ub, sb, vhb, _, _), (_, us, ss, vhs, sweeps, status) = _run(shape), _run(shape, exp2)
    bound = 8 * min(shape) * EPS * inputs[i][1][0]
    s_back = np.ldexp(ss[i], -exp2)
    rec, rec_back = (ub[i] * sb[i]) @ vhb[i], (us[i] * s_back) @ vhs[i]
    print(f"svd_batch {shape} x 2^{exp2}: sweeps {sweeps[i]}, |s 2^-e - s| / bound = {maxdiff(s_back, sb[i]) / bound:.3f}, "
          f"reconstruction / bound = {maxdiff(rec_back, rec) / bound:.3f}")
    assert status[i] == 0 and 0 < sweeps[i] < 60
    assert maxdiff(s_back, sb[i]) <= bound
    assert maxdiff(rec_back, rec) <= bound


def test_no_buffer_stays_behind():
    from aqc_research_amd.mps_engine import svd_batch

    before = _live()
    svd_batch(_mixed()[0][:3], _mixed()[1][:3], _mixed()[2][:3])
    with pytest.raises(RuntimeError):
        from aqc_research_amd import _lib
        _lib.check(_lib.lib().aqc_svd_batch(0, 0, 4, 3, None, None, None, None, None, None, None, None))
    assert _live() == before   # the calls' own buffers are gone: the count is what other tests' live objects hold
