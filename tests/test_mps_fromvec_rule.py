"""CPU: the rule header of the conversion of dense vectors into MPS states (csrc/aqc_mps_fromvec_rule.h) as a stand-alone program under
AddressSanitizer + UBSan, the route through the ABI (which needs no device), and the argument errors of the Python layer that are
raised before any device call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import mps_fromvec_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_rule_header_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mps_fromvec_rule_selftest")
    build = subprocess.run(["g++", "-std=c++17", *SAN, os.path.join(ROOT, "tests", "native", "mps_fromvec_rule_selftest.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    print(run.stdout)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr


def test_route_through_the_abi():
    from aqc_research_amd import _lib
    from aqc_research_amd.mps_engine import FROM_VECTOR_FUSED_CAP, from_vector_route

    L = _lib.lib()
    assert FROM_VECTOR_FUSED_CAP == mps_fromvec_ref.CAP == 32
    assert from_vector_route(11) == "fused" and from_vector_route(12) == "host"
    assert from_vector_route(12, 32) == "fused" and from_vector_route(12, 33) == "host"
    assert from_vector_route(30, 32) == "fused" and from_vector_route(31, 32) == "host" and from_vector_route(2) == "fused" and from_vector_route(1) == "host"
    for n in range(1, 34):
        for cap in (0, 1, 7, 32, 33, 1000):
            assert from_vector_route(n, cap) == mps_fromvec_ref.route(n, cap), (n, cap)
    assert L.aqc_mps_from_vec_route(12, 32) == 1 and L.aqc_mps_from_vec_route(12, 0) == 2
    assert L.aqc_mps_from_vec_route(0, 0) == -1 and L.aqc_mps_from_vec_route(5, -1) == -1
    for bad in ((0, 0), (5, -1), (-3, 2)):
        with pytest.raises(ValueError):
            from_vector_route(*bad)


def test_budget_hook_returns_the_earlier_value():
    from aqc_research_amd import _lib

    L = _lib.lib()
    default = L.aqc_mps_from_vec_budget(12345)
    try:
        assert default == 8 << 30
        assert L.aqc_mps_from_vec_budget(0) == 12345 and L.aqc_mps_from_vec_budget(-1) == default
    finally:
        L.aqc_mps_from_vec_budget(0)


def test_argument_errors_of_the_python_layer():
    """Raised before any device call: the inputs are arrays and no device is touched."""
    from aqc_research_amd import mps_engine as me

    v = np.zeros(16, dtype=np.complex128)
    v[3] = 1.0
    for method in ("dense", 1, "Fused", "canonical"):
        with pytest.raises(ValueError):
            me.from_vectors(v, method=method)
    for thr, cap in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0), (0.0, -1)):
        with pytest.raises(ValueError):
            me.from_vectors(v, thr, cap)
    for vecs in (np.zeros(12, dtype=np.complex128), np.zeros(2, dtype=np.complex128), np.zeros(1), np.zeros((2, 3, 4)), np.zeros((3, 12)), [], 42,
                 [v, np.zeros(8, dtype=np.complex128)], [np.zeros((2, 4))], np.zeros(0), "ab"):
        with pytest.raises(ValueError):
            me.from_vectors(vecs)
    big = np.zeros(2 ** 12, dtype=np.complex128)
    big[0] = 1.0
    with pytest.raises(ValueError):
        me.from_vectors(big, method="fused")                    # 12 qubits without a cap: the rule refuses
    with pytest.raises(ValueError):
        me.from_vectors(big, 0.0, 33, method="fused")
    with pytest.raises(ValueError):
        me.DeviceMPS.from_vector(np.zeros((2, 16)))
    assert np.count_nonzero(v) == 1 and v[3] == 1.0
