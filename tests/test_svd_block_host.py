"""CPU-only checks of the batched block-Jacobi SVD (csrc/aqc_svd_batch.hip): its rule as stated in NumPy (tests/svd_block_ref.py) on
the spectra of tests/test_hip_svd_spectra.py, held to the bounds that file applies to the device routes, and csrc/aqc_svd_blocks.h
(tournament, ragged blocks, transposition, LDS bytes) built by g++ under ASan + UBSan as a stand-alone program.

Does the Gram step alone survive ``graded`` and ``graded-negligible``?  Yes: the panel's Gram matrix is formed afresh from W at every
visit, so what G loses on graded columns costs sweeps (18 at 130 x 66 against 10 for ``clusters``), not accuracy, and every bound holds
without closing scalar sweeps.  What does not survive on its own is V: the 32 x 32 J of a visit carries the rounding of up to 62
rotations per column, V collects that defect at every visit, and at the kernel's largest shapes (18 .. 40 sweeps) |V V^H - 1| ended at
1.3 (256 x 128 ``clusters``), 1.4 (``graded``), 1.5 (``graded-negligible``), 1.9, 2.0 and 2.3 (the same at 256 x 256) times 8 k eps.
One Newton-Schulz step J <- J + J (1 - J^H J) / 2 per visit takes that to 0.014 .. 0.020 at those six, and singular values and
reconstruction from 0.36 .. 0.90 and 0.02 .. 0.22 of their bound to below 0.011 and 0.002; two or four inner sweeps make no difference
then.  (16 .. 80 s per matrix in NumPy at those shapes, so no test runs them here: ``python -m tests.svd_block_ref 256 128`` prints the
figures without and with the step, and tests/test_hip_svd_batch.py runs the shapes on the device.)"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import sketch_ref as sk
from tests import svd_block_ref as ref
from tests.helpers import maxdiff
from tests.test_hip_svd_spectra import CASES, EPS, _clusters, _input, _spectrum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
# one block; a pair and a ragged third block; five blocks (a bye) with a ragged last one, also transposed
SHAPE_CASES = [(s, c) for s in ((24, 24), (64, 40), (130, 66)) for c in CASES] + [((66, 130), c) for c in ("clusters", "graded", "permuted-diagonal")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    path = str(tmp_path_factory.mktemp("svd_blocks") / "svd_blocks_selftest")
    out = subprocess.run(["g++", "-std=c++17", *SAN, os.path.join(ROOT, "tests", "native", "svd_blocks_selftest.cpp"), "-o", path],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    return path


def _run(exe, *args):
    out = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_blocks_header_selftest(exe):
    """every block pair once per sweep for 1..17 blocks, a bye per round when the count is odd, ragged last blocks, LDS <= 160 KiB"""
    assert _run(exe).strip().endswith("ok")


@pytest.mark.parametrize("nb", [1, 2, 3, 5, 8, 16])
def test_numpy_statement_uses_the_headers_schedule(exe, nb):
    lines = [ln.split() for ln in _run(exe, "schedule", nb).split("\n") if ln.strip()]
    got = [[tuple(int(v) for v in pair.split(",")) for pair in ln] for ln in lines]
    assert got == ref.schedule(nb)
    assert ref.blocks(16 * nb - 3) == nb and ref.block_width(nb - 1, 16 * nb - 3) == 13


@pytest.mark.parametrize("shape,case", SHAPE_CASES)
def test_block_rule_on_prescribed_spectra(shape, case):
    """The bounds of test_hip_svd_spectra.test_prescribed_spectrum on the NumPy statement of the block rule."""
    m, n = shape
    k = min(m, n)
    a, s_true, u_true, v_true = _input(case, m, n)
    u, s, vh, sweeps, status = ref.svd_block(a)
    s0, bound = s_true[0], 8 * k * EPS * s_true[0]
    e_s, e_rec = maxdiff(s, s_true), maxdiff((u * s) @ vh, a)
    good = s > 1e-12 * s0
    ng = int(good.sum())
    e_u = maxdiff(np.conj(u[:, good].T) @ u[:, good], np.eye(ng))
    e_v = maxdiff(vh[good] @ np.conj(vh[good].T), np.eye(ng))
    print(f"block rule {m}x{n} {case}: sweeps {sweeps}, |s - s_true| / bound {e_s / bound:.3f}; reconstruction / bound {e_rec / bound:.3f}; "
          f"orthonormality / (8 k eps): u {e_u / (8 * k * EPS):.3f}, vh {e_v / (8 * k * EPS):.3f}")
    assert status == ref.CONVERGED and 0 < sweeps < 60
    assert np.all(np.diff(s) <= 1e-13 * s0)
    assert e_s <= bound
    assert e_rec <= bound
    assert e_u <= 8 * k * EPS and e_v <= 8 * k * EPS
    if case == "rank-half":
        assert ng == k // 2
    if case in ("diagonal", "permuted-diagonal"):
        assert sweeps == 1
        for name, mat in (("u", u), ("vh", vh.T)):
            hot = np.abs(mat) > 0.5
            assert maxdiff(np.abs(mat), hot.astype(float)) <= 1e-15, name
            assert np.all(hot.sum(axis=0) == 1) and np.all(hot.sum(axis=1) <= 1), name
    if case in ("equal", "clusters"):
        for idx, gap in _clusters(s_true):
            tol = bound / gap
            assert maxdiff(u[:, idx] @ np.conj(u[:, idx].T), u_true[:, idx] @ np.conj(u_true[:, idx].T)) <= tol
            assert maxdiff(np.conj(vh[idx].T) @ vh[idx], v_true[:, idx] @ np.conj(v_true[:, idx].T)) <= tol


def test_newton_schulz_step_takes_the_rotations_rounding_out_of_j():
    """J^H J - 1 after the step is the rounding of ONE 32-term product, whatever the rotations left: never more than before the step"""
    a = _input("graded", 256, 32)[0]
    g = np.conj(a.T) @ a
    g = np.triu(g, 1) + np.conj(np.triu(g, 1).T) + np.diag(np.diag(g).real)
    defect = []
    for step in (False, True):
        j, did = ref.diagonalise(g, np.ones(32, dtype=bool), 0.0, newton_schulz=step)
        assert did
        defect.append(maxdiff(np.conj(j.T) @ j, np.eye(32)))
    print(f"|J^H J - 1| / eps: {defect[0] / EPS:.1f} as rotated, {defect[1] / EPS:.1f} after the step")
    assert defect[1] < defect[0]


def test_block_rule_status_and_zero_matrix():
    a = sk.with_spectrum(20, 12, _spectrum("clusters", 12), np.random.default_rng(3))[0]
    a[3, 4] = np.nan
    u, s, vh, sweeps, status = ref.svd_block(a)
    assert status == ref.NON_FINITE and not u.any() and not s.any() and not vh.any()
    u, s, vh, sweeps, status = ref.svd_block(np.zeros((5, 3), dtype=np.complex128))
    assert status == ref.CONVERGED and sweeps == 1 and not s.any() and not u.any() and np.array_equal(vh, np.eye(3))


def test_svd_batch_argument_errors_come_before_any_device_call(monkeypatch):
    from aqc_research_amd import _lib, mps_engine

    def no_device(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(_lib, "lib", no_device)
    good = np.zeros((2, 4, 3), dtype=np.complex128)
    with pytest.raises(TypeError):
        mps_engine.svd_batch([[1.0]])
    with pytest.raises(TypeError):
        mps_engine.svd_batch(np.zeros((2, 4, 3)))
    with pytest.raises(ValueError, match="count, m, n"):
        mps_engine.svd_batch(good[0])
    with pytest.raises(ValueError, match="256"):
        mps_engine.svd_batch(np.zeros((1, 257, 3), dtype=np.complex128))
    with pytest.raises(ValueError, match="count"):
        mps_engine.svd_batch(np.zeros((0, 4, 3), dtype=np.complex128))
    with pytest.raises(ValueError, match="rows"):
        mps_engine.svd_batch(good, rows=[4])
    with pytest.raises(ValueError, match="rows"):
        mps_engine.svd_batch(good, rows=[4, 5])
    with pytest.raises(ValueError, match="cols"):
        mps_engine.svd_batch(good, cols=[0, 3])
    with pytest.raises(ValueError, match="cols"):
        mps_engine.svd_batch(good, cols=[1.0, 2.0])
