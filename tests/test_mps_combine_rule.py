"""CPU: the rule header of MPS linear combinations (csrc/aqc_mps_combine_rule.h) as a stand-alone program under AddressSanitizer +
UBSan, the route through the ABI (which needs no device), and the argument errors of the Python layer that are raised before any
device call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_rule_header_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mps_combine_rule_selftest")
    build = subprocess.run(["g++", "-std=c++17", *SAN, os.path.join(ROOT, "tests", "native", "mps_combine_rule_selftest.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    print(run.stdout)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr


def test_route_through_the_abi():
    from ctypes import POINTER, c_int32

    from aqc_research_amd import _lib
    from aqc_research_amd.mps_engine import COMPRESS_FUSED_CAP, combine_route

    L = _lib.lib()
    i32 = lambda a: a.ctypes.data_as(POINTER(c_int32))   # noqa: E731
    assert COMPRESS_FUSED_CAP == 64
    four = [[1, 2, 4, 8, 16, 8, 4, 2, 1]] * 4
    assert combine_route(four) == "fused"                                       # a summed bond of exactly 64
    assert combine_route(four + [[1] * 9]) == "canonical"                       # 65
    assert combine_route([[1, 2, 64, 2, 1]]) == "fused" and combine_route([[1, 2, 65, 2, 1]]) == "canonical"
    assert combine_route([[1, 1]] * 100) == "fused"                             # one qubit: no bond to sum
    good = np.array([[1, 32, 1], [1, 32, 1]], dtype=np.int32)
    assert L.aqc_mps_combine_route(2, 2, i32(good)) == 1
    assert L.aqc_mps_combine_route(2, 2, i32(np.array([[1, 32, 1], [1, 33, 1]], dtype=np.int32))) == 2
    assert L.aqc_mps_combine_route(0, 2, i32(good)) == -1 and L.aqc_mps_combine_route(2, 0, i32(good)) == -1 and L.aqc_mps_combine_route(2, 2, None) == -1
    assert L.aqc_mps_combine_route(2, 2, i32(np.array([[1, 32, 1], [1, 0, 1]], dtype=np.int32))) == -1
    for dims in ([1, 2, 1], [[1]], [[1, 0, 1]], []):
        with pytest.raises(ValueError):
            combine_route(dims)


def test_argument_errors_of_the_python_layer():
    """Raised before anything is uploaded: the states here are QiskitMPS tuples, and no device is touched."""
    from aqc_research_amd import mps_engine as me
    from tests import mps_obs_ref

    a = mps_obs_ref.hand_made([1, 2, 2, 1], 1)
    b = mps_obs_ref.hand_made([1, 2, 2, 1], 2)
    longer = mps_obs_ref.hand_made([1, 2, 2, 2, 1], 3)
    wide = mps_obs_ref.hand_made([1, 2, 33, 2, 1], 4)
    for method in ("dense", 1, "Fused", "gemm"):
        with pytest.raises(ValueError):
            me.linear_combinations([a, b], [1.0, 1.0], method=method)
    for thr, cap in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0), (0.0, -1)):
        with pytest.raises(ValueError):
            me.linear_combinations([a, b], [1.0, 1.0], thr, cap)
    for coeffs in ([1.0], [1.0, 1.0, 1.0], [[1.0], [1.0]], np.ones((2, 2, 2)), 1.0, np.ones((0, 2))):
        with pytest.raises(ValueError):
            me.linear_combinations([a, b], coeffs)
    with pytest.raises(ValueError, match="zero"):
        me.linear_combinations([a, b], [0.0, 0.0])
    with pytest.raises(ValueError, match="output 1"):
        me.linear_combinations([a, b], [[1.0, 0.0], [0.0, 0.0]])
    with pytest.raises(ValueError):
        me.linear_combinations([a, longer], [1.0, 1.0])
    with pytest.raises(ValueError, match="fused"):
        me.linear_combinations([wide, wide], [1.0, 1.0], method="fused")        # 33 + 33 = 66
    with pytest.raises(ValueError, match="output 1"):
        me.linear_combinations([wide, wide], [[1.0, 0.0], [1.0, 1.0]], method="fused")
    for states in ([], 42, [42], [None], "ab", a):
        with pytest.raises(ValueError):
            me.linear_combinations(states, [1.0])
