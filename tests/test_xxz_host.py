"""CPU-only checks of csrc/aqc_xxz_rule.h, the host-visible rules of exact XXZ evolution (anti-alignment mask, diagonal, partner
index, series length, Bessel values by Miller's recurrence, series coefficients): built by g++ under ASan + UBSan as a stand-alone
program (tests/native/xxz_rule_selftest.cpp) and compared with the NumPy statement (tests/xxz_ref.py) and SciPy."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.special import jv

from tests import xxz_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
BESSEL_X = (1e-3, 0.3, 2.7, 14.25, 97.2, 136.8, 800.0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    path = str(tmp_path_factory.mktemp("xxz_rule") / "xxz_rule_selftest")
    out = subprocess.run(["g++", "-std=c++17", *SAN, os.path.join(ROOT, "tests", "native", "xxz_rule_selftest.cpp"), "-o", path],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    return path


def _hex(values) -> str:
    return " ".join(f"{int(b):016x}" for b in np.ascontiguousarray(values, dtype=np.float64).ravel().view(np.uint64))


def _run(exe, mode, text):
    out = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr
    return out.stdout.split()


def _f64(words) -> np.ndarray:
    return np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64)


@pytest.mark.parametrize("n", range(2, 11))
def test_rule_action_matches_statement(exe, n):
    for k, delta in enumerate((1.0, 0.5, -0.7, 0.0, 2.5)):
        psi = xxz_ref.random_states(n, 1, 100 * n + k)[0]
        got = _f64(_run(exe, "mul", f"{n} {_hex([delta])} {_hex(psi.view(np.float64))}")).view(np.complex128)
        err = float(np.max(np.abs(got - xxz_ref.mul_vec(psi, delta))))
        assert err <= 1e-14, (n, delta, err)


@pytest.mark.parametrize("x", BESSEL_X)
def test_series_length_and_bessel_values(exe, x):
    words = _run(exe, "bessel", _hex([x]))
    K = int(words[0])
    assert K == xxz_ref.series_length(x)
    J = _f64(words[1:])
    assert J.size == K + 1
    err = float(np.max(np.abs(J - jv(np.arange(K + 1), x))))
    print(f"x = {x}: K = {K}, max |J - scipy| = {err:.3g}")
    assert err <= 1e-13, (x, err)


@pytest.mark.parametrize("x", (0.0, 1e-12, -0.3, 2.7, -14.25, 97.2))
def test_coefficients_match_statement(exe, x):
    """c_k for signed x, x = 0 and the power-series branch of tiny x included.  |c_k| = 2 |J_k|: twice the bound on the Bessel values."""
    words = _run(exe, "coef", _hex([x]))
    ref = xxz_ref.coefficients(x)
    assert int(words[0]) == ref.size - 1
    got = _f64(words[1:]).view(np.complex128)
    assert float(np.max(np.abs(got - ref))) <= 2e-13


def test_series_refuses_what_it_cannot_hold(exe):
    for x in (float("inf"), float("nan"), 1e9):
        assert int(_run(exe, "bessel", _hex([x]))[0]) == -1
