"""CPU-only checks of the device-resident sketching path's host-visible pieces: csrc/aqc_philox.h built by g++ under ASan + UBSan
against np.random.Philox bit for bit, the counter rule of tests/sketch_ref.py, its CholeskyQR2, and the driver's host policy."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import sketch_ref as sk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
M64 = (1 << 64) - 1
# (key, counter): an ordinary pair, the draw rule's own shape, and a counter whose low word wraps inside the run (carry into word 1)
PAIRS = [((1234567, 2), (0, 0, 0, 0)), ((42, 0), (0, 7, 3, 1)), ((M64, 0x9E3779B97F4A7C15), (M64 - 1, M64, 5, 6))]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    path = str(tmp_path_factory.mktemp("philox") / "philox_selftest")
    out = subprocess.run(["g++", "-std=c++17", *SAN, os.path.join(ROOT, "tests", "native", "philox_selftest.cpp"), "-o", path],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    return path


def _run(exe, *args):
    out = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr
    return out.stdout.split()


@pytest.mark.parametrize("key,counter", PAIRS)
def test_philox_header_equals_numpy_bit_for_bit(exe, key, counter):
    nblocks = 5
    words = _run(exe, "raw", *key, *counter, nblocks)
    raw = np.array([int(w, 16) for w in words[0::2]], dtype=np.uint64)
    dbl = np.array([int(w, 16) for w in words[1::2]], dtype=np.uint64).view(np.float64)
    mk = lambda: np.random.Philox(key=np.array(key, dtype=np.uint64), counter=np.array(counter, dtype=np.uint64))
    assert np.array_equal(raw, mk().random_raw(4 * nblocks))          # NumPy advances the counter before its first block
    assert np.array_equal(dbl, np.random.Generator(mk()).random(4 * nblocks))
    if counter[0] == M64 - 1:   # the low word wrapped: the second block's counter is (0, 0, 6, 6) after two carries
        st = mk()
        st.random_raw(8)
        assert [int(c) for c in st.state["state"]["counter"]] == [0, 0, 6, 6]


def test_plane_rule_is_the_documented_numpy_call(exe):
    seed, stream, it, lane, plane, count = 99, sk.SKETCH_EIGEN, 5, 1, 3, 37    # (count not a multiple of the block)
    got = np.array([int(w, 16) for w in _run(exe, "plane", seed, stream, it, lane, plane, count)], dtype=np.uint64).view(np.float64)
    assert np.array_equal(got, sk.plane_uniforms(seed, stream, it, lane, plane, count))
    assert got.min() >= 0.0 and got.max() < 1.0
    other = sk.plane_uniforms(seed, stream, it, lane + 1, plane, count)
    assert not np.array_equal(got, other)


def test_box_muller_moments():
    z = sk.box_muller(sk.plane_uniforms(3, 2, 1, 0, 0, 200000), sk.plane_uniforms(3, 2, 1, 0, 1, 200000))
    assert np.all(np.isfinite(z)) and abs(z.mean()) < 0.01 and abs(z.var() - 1) < 0.02 and abs(np.mean(z**4) - 3) < 0.1


@pytest.mark.parametrize("d,k", [(4, 1), (16, 4), (256, 64), (1024, 16)])
def test_cholesky_qr2_reference(d, k):
    a = sk.omega(sk.SKETCH_RAND, 11, 1, 0, d, k)
    q, qh = sk.cholesky_qr2(a), np.linalg.qr(a)[0]
    assert np.max(np.abs(np.conj(q.T) @ q - np.eye(k))) < 1e-14
    assert np.max(np.abs(q @ np.conj(q.T) - qh @ np.conj(qh.T))) < 1e-13


EPS = 2.2e-16


def _orth_and_range(q, a):
    ref = sk.extended_range_basis(a)
    return (float(np.max(np.abs(np.conj(q.T) @ q - np.eye(a.shape[1])))), float(np.max(np.abs(q @ np.conj(q.T) - ref @ np.conj(ref.T)))))


@pytest.mark.parametrize("kappa", [1e2, 1e3, 1e4])
@pytest.mark.parametrize("spectrum", ["geometric", "last"])
@pytest.mark.parametrize("d,k", [(64, 16), (100, 16), (256, 64)])
def test_qr_rule_on_the_conditioning_ladder(d, k, spectrum, kappa):
    """The device's rule in NumPy accepts condition numbers up to 1e4 and returns the range to 64 eps kappa against the
    extended-precision reference (the ladder of tests/test_hip_qr_conditioning.py)."""
    s = np.geomspace(1.0, 1.0 / kappa, k) if spectrum == "geometric" else np.r_[np.ones(k - 1), 1.0 / kappa]
    a = sk.with_spectrum(d, k, s, np.random.default_rng(int(d + k + np.log10(kappa))))[0]
    q, st = sk.cholesky_qr2_rule(a)
    assert st == 0
    e_orth, e_proj = _orth_and_range(q, a)
    assert e_orth < 1e-12 and e_proj <= 64 * EPS * kappa


def test_qr_rule_status_contract_and_why_the_second_pass_is_tested():
    """Over the straddling family, status 0 means an orthonormal Q of a range that double precision determines (64 eps kappa_eq
    < 1e-6), and a flagged matrix comes back as it was.  With the test on G2 - I switched off -- pivots alone, as the kernel was --
    the same family holds matrices that pass every pivot test of both passes and break that contract."""
    silent, sides = [], {0: 0, sk.QR_RANK_DEFICIENT: 0}
    must_accept = must_flag = 0
    for name, a in sk.straddling_family():
        keq = sk.cond_equilibrated(a)
        q, st = sk.cholesky_qr2_rule(a)
        sides[st] += 1
        if st == 0:
            e_orth, e_proj = _orth_and_range(q, a)
            assert 64 * EPS * keq < 1e-6 and e_orth < 1e-12 and e_proj <= 64 * EPS * keq, (name, keq, e_orth, e_proj)
        else:
            assert np.array_equal(q, a), name
        must_accept += keq <= 1e4
        must_flag += keq >= 1e14
        assert not (keq <= 1e4 and st != 0) and not (keq >= 1e14 and st == 0), (name, keq, st)
        q_old, st_old = sk.cholesky_qr2_rule(a, orth_tol=np.inf)
        if st_old == 0 and (64 * EPS * keq >= 1e-6 or _orth_and_range(q_old, a)[0] >= 1e-12):
            silent.append(name)
    assert must_accept > 0 and must_flag > 0 and sides[0] > 0 and sides[sk.QR_RANK_DEFICIENT] > 0
    assert silent, "the pivot tests alone were expected to let an ill-conditioned matrix through"


def test_alt_index_schedule_follows_the_reference_rule():
    from aqc_research_amd.model_sketching.aqc_sketching import AltIndexSchedule

    d, k = 8, 4
    np.random.seed(5)
    sched = AltIndexSchedule(d, k, lanes=1)
    got = [sched.next()[0] for _ in range(5)]
    np.random.seed(5)
    perm, offset, want = np.random.permutation(d), 0, []
    for _ in range(5):
        if offset >= d:
            offset, perm = 0, np.random.permutation(d)
        want.append(perm[offset:offset + k])
        offset += k
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_driver_policy_replays_a_profile():
    """The restart policy of stochastic_aqc on a recorded profile: halving, at most 5 corrections, maxiter accounting."""
    from aqc_research_amd.model_sketching.aqc_sketching import ChunkPolicy
    from aqc_research_amd.optimizer import NotImproveStopper

    pol = ChunkPolicy(maxiter=1000, learn_rate=0.1, stopper=NotImproveStopper(num_iters=3), max_corrections=5)
    prof = [0.5, 0.6, 0.6, 0.6, 0.6, 0.6, 0.6, 0.6]     # stale from the 5th value on (4 iterations after the best at the 1st)
    assert pol.feed(prof) and pol.learn_rate == 0.05 and pol.corrections == 1 and pol.restart_from_best
    assert pol.remaining == 1000 - len(prof)             # the budget shrinks by all evaluations made so far (aqc_sketching.py:100)
    for _ in range(3):
        assert pol.feed(prof)
    assert pol.corrections == 4 and pol.learn_rate == pytest.approx(0.1 / 16)
    assert pol.feed(prof) and pol.corrections == 5       # the last correction: no halving, the stopper is disabled (:83-89)
    assert pol.learn_rate == pytest.approx(0.1 / 16) and not pol.restart_from_best
    assert pol.remaining == 1000 - len(prof) * (1 + 2 + 3 + 4 + 5) and not pol.finished
    assert not pol.feed(prof) and pol.exit_status is None
    short = ChunkPolicy(maxiter=10, learn_rate=0.1, stopper=None)
    assert not short.feed(prof) and not short.finished
    assert not short.feed(prof[:2]) and short.finished and short.exit_status == "normal"
    late = ChunkPolicy(maxiter=8, learn_rate=0.1, stopper=NotImproveStopper(num_iters=3))
    assert late.feed(prof) and late.finished and late.exit_status == "premature"
