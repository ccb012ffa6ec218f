"""CPU: the rule header of the Pauli strings between MPS states (csrc/aqc_mps_pauli_rule.h) as a stand-alone program under
AddressSanitizer + UBSan, the supports and the route through the ABI (which need no device) with their refusals, and the argument errors
of the Python layer that are raised before any device call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_rule_header_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mps_pauli_rule_selftest")
    build = subprocess.run(["g++", "-std=c++17", *SAN, os.path.join(ROOT, "tests", "native", "mps_pauli_rule_selftest.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr


def test_support_and_route_through_the_abi():
    from ctypes import POINTER, c_int32, c_uint8

    from aqc_research_amd import _lib
    from aqc_research_amd.mps_observables import pauli_route

    L = _lib.lib()
    i32 = lambda a: a.ctypes.data_as(POINTER(c_int32))   # noqa: E731
    u8 = lambda a: a.ctypes.data_as(POINTER(c_uint8))    # noqa: E731
    strings = np.array([[0, 0, 0, 0, 0], [0, 1, 0, 3, 0], [2, 2, 2, 2, 2], [0, 0, 0, 0, 3], [1, 0, 0, 0, 0]], dtype=np.uint8)
    first, last = np.full(5, -1, np.int32), np.full(5, -1, np.int32)
    assert L.aqc_mps_pauli_support(5, 5, u8(strings), i32(first), i32(last)) == 0
    assert first.tolist() == [0, 1, 0, 4, 0] and last.tolist() == [0, 3, 4, 4, 0]
    # refusals
    assert L.aqc_mps_pauli_support(5, 5, None, i32(first), i32(last)) == 1
    assert L.aqc_mps_pauli_support(5, 5, u8(strings), None, i32(last)) == 1 and L.aqc_mps_pauli_support(5, 5, u8(strings), i32(first), None) == 1
    assert L.aqc_mps_pauli_support(0, 5, u8(strings), i32(first), i32(last)) == 1
    assert L.aqc_mps_pauli_support(5, 0, u8(strings), i32(first), i32(last)) == 1 and b"at least one string" in L.aqc_last_error()
    bad = strings.copy()
    bad[3, 2] = 4
    assert L.aqc_mps_pauli_support(5, 5, u8(bad), i32(first), i32(last)) == 1
    assert b"string 3, qubit 2" in L.aqc_last_error() and b"not 4" in L.aqc_last_error()
    # the route over both states' bonds
    assert pauli_route(None, [1, 2, 64, 64, 2, 1]) == "fused" and pauli_route(None, [1, 2, 65, 2, 1]) == "gemm"
    assert pauli_route([1, 2, 64, 2, 1], [1, 2, 3, 2, 1]) == "fused" and pauli_route([1, 2, 65, 2, 1], [1, 2, 3, 2, 1]) == "gemm"
    assert pauli_route([1, 2, 3, 2, 1], [1, 2, 65, 2, 1]) == "gemm" and pauli_route(None, [1, 1]) == "fused"
    good = np.array([1, 2, 2, 1], dtype=np.int32)
    assert L.aqc_mps_pauli_route(0, None, i32(good)) == -1 and L.aqc_mps_pauli_route(3, None, None) == -1
    assert L.aqc_mps_pauli_route(3, i32(np.array([1, 0, 2, 1], dtype=np.int32)), i32(good)) == -1
    assert L.aqc_mps_pauli_route(3, i32(good), i32(good)) == 1
    for dims in ([1], [[1, 2], [2, 1]]):
        with pytest.raises(ValueError):
            pauli_route(None, dims)
    with pytest.raises(ValueError):
        pauli_route([1, 2, 1], [1, 2, 2, 1])


def test_argument_errors_of_the_python_layer():
    from aqc_research_amd import mps_observables as mo
    from tests import mps_obs_ref

    state = mps_obs_ref.hand_made([1, 2, 2, 1], 1)   # a QiskitMPS tuple: nothing is uploaded for a refused call
    other = mps_obs_ref.hand_made([1, 2, 2, 2, 1], 2)
    for bad in ([], ["XYZZ"], ["XY"], ["XAZ"], [("XZ", (0,))], [("XZ", (0, 3))], [("XX", (1, 1))], [("Q", (1,))], [7], "XYZ",
                np.zeros((0, 3), np.uint8), np.zeros((2, 4), np.uint8), np.full((1, 3), 4, np.uint8), np.zeros(3, np.uint8),
                np.zeros((1, 3), np.float64)):
        with pytest.raises(ValueError):
            mo.pauli_strings(state, bad)
    for states in ([], 42, [42], [None], "ab", [state, other]):
        with pytest.raises(ValueError):
            mo.pauli_strings(states, ["XYZ"])
    for bras in ([state], [state, state], other, 42):
        with pytest.raises(ValueError):
            mo.pauli_strings(state, ["XYZ"], bras=bras)
    with pytest.raises(ValueError):
        mo.pauli_strings([state, state], ["XYZ"], bras=[state])
    with pytest.raises(ValueError):
        mo.pauli_strings([state, state], ["XYZ"], bras=state)
    for method in ("dense", 1, "Fused"):
        with pytest.raises(ValueError):
            mo.pauli_strings(state, ["XYZ"], method=method)
        with pytest.raises(ValueError):
            mo.overlaps([state], [state], method=method)
    for bras, kets in ((state, [state]), ([state], state), ([], [state]), ([state], []), ([state], [other])):
        with pytest.raises(ValueError):
            mo.overlaps(bras, kets)
    for terms in ([], "XYZ", [("XYZ",)], [(float("nan"), "XYZ")], [(1.0, "XY")], [1.0]):
        with pytest.raises(ValueError):
            mo.energy(state, terms)
    # what the three forms of a string list mean, without a device
    assert np.array_equal(mo._strings(["IXYZ", "ZIII"], 4), [[0, 1, 2, 3], [3, 0, 0, 0]])
    assert np.array_equal(mo._strings([("XZ", (3, 0)), ("", ())], 4), [[3, 0, 0, 1], [0, 0, 0, 0]])
    assert np.array_equal(mo._strings(np.array([[0, 1, 2, 3]]), 4), [[0, 1, 2, 3]])
