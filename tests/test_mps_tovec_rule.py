"""CPU: the rule header of the conversion of MPS states into dense vectors and blocks of amplitudes (csrc/aqc_mps_tovec_rule.h) as a
stand-alone program under AddressSanitizer + UBSan, the route and the budget hook through the ABI (which need no device), and the
argument errors of the Python layer, which are raised before any device work: the states of these tests are stand-ins that answer the
three host questions the checks ask (qubits, bonds, device) and own nothing on a device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import mps_obs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_rule_header_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mps_tovec_rule_selftest")
    build = subprocess.run(["g++", "-std=c++17", *SAN, os.path.join(ROOT, "tests", "native", "mps_tovec_rule_selftest.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    print(run.stdout)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr


def test_route_through_the_abi():
    from aqc_research_amd import _lib
    from aqc_research_amd.mps_engine import TO_VECTOR_FUSED_CAP, to_vector_route

    L = _lib.lib()
    assert TO_VECTOR_FUSED_CAP == 64
    assert to_vector_route(mps_obs_ref.PROFILE_A) == "fused" and to_vector_route(mps_obs_ref.PROFILE_D) == "gemm"
    assert to_vector_route(mps_obs_ref.PROFILE_C) == "fused" and to_vector_route(mps_obs_ref.profile_b(7)) == "fused" and to_vector_route([1, 1]) == "fused"
    assert to_vector_route([1, 2, 64, 2, 1]) == "fused" and to_vector_route([1, 2, 65, 2, 1]) == "gemm"
    d = np.array([1, 2, 65, 2, 1], dtype=np.int32)
    assert L.aqc_mps_to_vec_route(4, _lib.iptr(d)) == 2 and L.aqc_mps_to_vec_route(0, _lib.iptr(d)) == -1 and L.aqc_mps_to_vec_route(4, None) == -1
    for bad in ([], [1], np.ones((2, 3)), 7):
        with pytest.raises(ValueError):
            to_vector_route(bad)


def test_budget_hook_returns_the_earlier_value():
    from aqc_research_amd import _lib

    L = _lib.lib()
    default = L.aqc_mps_to_vec_budget(12345)
    try:
        assert default == 8 << 30
        assert L.aqc_mps_to_vec_budget(0) == 12345 and L.aqc_mps_to_vec_budget(-1) == default
    finally:
        L.aqc_mps_to_vec_budget(0)


def _stand_in(dims, device=0):
    """A DeviceMPS that owns nothing: what the argument checks read of a state, and a handle that no native call may ever see."""
    from aqc_research_amd.mps_engine import DeviceMPS

    class StandIn(DeviceMPS):
        num_qubits = len(dims) - 1
        bond_dims = np.asarray(dims, dtype=np.int32)

        def __init__(self):
            self.handle, self._L = "not a handle", None

        def close(self):
            self.handle = None

    StandIn.device = device
    return StandIn()


def test_argument_errors_of_the_python_layer():
    """Every refusal is raised before the native call: a stand-in's handle would not survive one."""
    from aqc_research_amd import mps_engine as me

    a = _stand_in(mps_obs_ref.PROFILE_A)
    wide = _stand_in(mps_obs_ref.PROFILE_D)
    n = a.num_qubits
    for method in ("dense", 1, "Fused", "host"):
        with pytest.raises(ValueError):
            me.to_vectors(a, method=method)
        with pytest.raises(ValueError):
            me.amplitude_blocks(a, 5, np.zeros((1, n - 5), dtype=np.uint8), method=method)
    with pytest.raises(ValueError):
        me.amplitude_blocks(a, 5, np.zeros((1, n - 5), dtype=np.uint8), method="gemm")       # blocks are fused only
    for states in ([], 42, None, [a, "x"], (mps_obs_ref.hand_made([1, 2, 1], 1),)):
        with pytest.raises(ValueError):
            me.to_vectors(states)
    with pytest.raises(ValueError, match="size or device"):
        me.to_vectors([a, _stand_in(mps_obs_ref.PROFILE_C)])
    with pytest.raises(ValueError, match="size or device"):
        me.to_vectors([a, _stand_in(mps_obs_ref.PROFILE_A, device=1)])
    with pytest.raises(ValueError, match="30 qubits"):
        me.to_vectors(_stand_in([1] * 32))
    with pytest.raises(ValueError, match="state 1 has 96"):
        me.to_vectors([a, wide], method="fused")
    with pytest.raises(ValueError, match="state 0 has 96"):
        wide.to_vector(method="fused")
    closed = _stand_in(mps_obs_ref.PROFILE_A)
    closed.close()
    with pytest.raises(ValueError, match="closed"):
        me.to_vectors([a, closed])
    good = np.zeros(2 ** n, dtype=np.complex128)
    for out in (np.zeros(2 ** n), np.zeros(2 ** n, dtype=np.complex64), np.zeros(2 ** n - 1, dtype=np.complex128), np.zeros((1, 2 ** n), dtype=np.complex128),
                np.zeros(2 ** (n + 1), dtype=np.complex128)[::2], [0j] * 2 ** n, np.zeros((2 ** n, 2), dtype=np.complex128)[:, 0]):
        with pytest.raises(ValueError, match="out must be"):
            me.to_vectors(a, out=out)
    with pytest.raises(ValueError, match="out must be"):
        me.to_vectors([a, a], out=good)                                                     # a list wants [states][2^n]
    with pytest.raises(ValueError, match="out must be"):
        me.to_vectors([a, a], out=np.zeros((2 ** n, 2), dtype=np.complex128).T)            # the shape, not contiguous
    # blocks: the shape of the call
    for k in (0, n, n + 1, -1):
        with pytest.raises(ValueError, match="low_qubits"):
            me.amplitude_blocks(a, k, np.zeros((1, max(n - k, 1)), dtype=np.uint8))
    with pytest.raises(ValueError, match="low_qubits"):
        me.amplitude_blocks(_stand_in([1] * 41), 25, np.zeros((1, 15), dtype=np.uint8))      # beyond 24 low qubits
    with pytest.raises(ValueError, match="low_qubits"):
        me.amplitude_blocks(_stand_in([1, 1]), 1, np.zeros((1, 1), dtype=np.uint8))          # one qubit has no high site
    bits = np.zeros((3, n - 5), dtype=np.uint8)
    for bad in (bits[:, :-1], np.zeros((3, n - 4), dtype=np.uint8), bits[0], np.zeros((0, n - 5), dtype=np.uint8), bits.astype(np.float64)):
        with pytest.raises(ValueError):
            me.amplitude_blocks(a, 5, bad)
    two = bits.copy()
    two[1, 2] = 2
    with pytest.raises(ValueError, match="0 or 1"):
        me.amplitude_blocks(a, 5, two)
    with pytest.raises(ValueError, match="0 or 1"):
        a.amplitude_blocks(5, bits.astype(np.int64) - 1)
    with pytest.raises(ValueError, match="bond of 96"):
        me.amplitude_blocks([a, wide], 5, bits)
    assert a.handle == "not a handle" and wide.handle == "not a handle"


def test_native_refusals_need_no_device():
    """The ABI's own argument checks come before it looks for a device."""
    from aqc_research_amd import _lib

    L = _lib.lib()
    out = np.zeros(4, dtype=np.complex128)
    assert L.aqc_mps_to_vec(None, 1, 0, _lib.dptr(out), None) == 1 and b"null" in L.aqc_last_error()
    handles = (_lib._P * 1)(None)
    assert L.aqc_mps_to_vec(handles, 0, 0, _lib.dptr(out), None) == 1 and b"at least one state" in L.aqc_last_error()
    assert L.aqc_mps_to_vec(handles, 1, 7, _lib.dptr(out), None) == 1 and b"unknown method 7" in L.aqc_last_error()
    assert L.aqc_mps_to_vec(handles, 1, 0, _lib.dptr(out), None) == 1 and b"null state" in L.aqc_last_error()
    bits = np.zeros((1, 1), dtype=np.uint8)
    bptr = bits.ctypes.data_as(_lib.POINTER(_lib.c_uint8))
    assert L.aqc_mps_amp_blocks(handles, 1, 1, 1, bptr, 2, _lib.dptr(out)) == 1 and b"fused route only" in L.aqc_last_error()
    assert L.aqc_mps_amp_blocks(handles, 1, 1, 1, bptr, 0, _lib.dptr(out)) == 1 and b"null state" in L.aqc_last_error()
