"""CPU: the rule header of operator sums on MPS states (csrc/aqc_mps_opsum_rule.h) as a stand-alone program under AddressSanitizer +
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
    exe = str(tmp_path / "mps_opsum_rule_selftest")
    build = subprocess.run(["g++", "-std=c++17", *SAN, os.path.join(ROOT, "tests", "native", "mps_opsum_rule_selftest.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    print(run.stdout)
    assert run.returncode == 0 and " 0 failures" in run.stdout, run.stdout + run.stderr


def test_route_through_the_abi():
    from ctypes import POINTER, c_int32

    from aqc_research_amd import _lib
    from aqc_research_amd.mps_engine import COMPRESS_FUSED_CAP, MPO, opsum_route

    L = _lib.lib()
    i32 = lambda a: a.ctypes.data_as(POINTER(c_int32))   # noqa: E731
    assert COMPRESS_FUSED_CAP == 64
    xxz = MPO.xxz(8, 0.5).bond_dims
    assert xxz.tolist() == [1, 5, 5, 5, 5, 5, 5, 5, 1]
    assert opsum_route([[1, 2, 4, 8, 12, 8, 4, 2, 1]], [xxz]) == "fused"                          # 5 x 12 = 60
    assert opsum_route([[1, 2, 4, 8, 13, 8, 4, 2, 1]], [xxz]) == "canonical"                      # 65
    assert opsum_route([[1, 2, 4, 8, 12, 8, 4, 2, 1], [1, 2, 4, 4, 4, 4, 4, 2, 1]], [xxz, None]) == "fused"       # 60 + 4
    assert opsum_route([[1, 2, 4, 8, 12, 8, 4, 2, 1], [1, 2, 4, 5, 5, 4, 4, 2, 1]], [xxz, None]) == "canonical"   # 60 + 5
    assert opsum_route([[1, 2, 64, 2, 1]], [MPO.from_pauli_string("XYZI").bond_dims]) == "fused"  # Pauli strings: D = 1
    assert opsum_route([[1, 2, 64, 2, 1]], [None]) == "fused" and opsum_route([[1, 2, 65, 2, 1]], [None]) == "canonical"
    assert opsum_route([[1, 1]] * 100, [None] * 100) == "fused"                                    # one qubit: no bond to sum
    s, d = np.array([[1, 32, 1], [1, 16, 1]], dtype=np.int32), np.array([[1, 1, 1], [1, 2, 1]], dtype=np.int32)
    assert L.aqc_mps_opsum_route(2, 2, i32(s), i32(d)) == 1
    assert L.aqc_mps_opsum_route(2, 2, i32(s), i32(np.array([[1, 1, 1], [1, 3, 1]], dtype=np.int32))) == 2
    assert L.aqc_mps_opsum_route(0, 2, i32(s), i32(d)) == -1 and L.aqc_mps_opsum_route(2, 0, i32(s), i32(d)) == -1
    assert L.aqc_mps_opsum_route(2, 2, None, i32(d)) == -1 and L.aqc_mps_opsum_route(2, 2, i32(s), None) == -1
    assert L.aqc_mps_opsum_route(2, 2, i32(s), i32(np.array([[1, 1, 1], [1, 0, 1]], dtype=np.int32))) == -1
    big = np.array([[1, 2147483647, 1]], dtype=np.int32)
    assert L.aqc_mps_opsum_route(2, 1, i32(big), i32(big)) == 2                                    # 64-bit: the product does not wrap
    for states, ops in (([1, 2, 1], [None]), ([[1]], [None]), ([[1, 0, 1]], [None]), ([], []), ([[1, 2, 1]], [None, None]), ([[1, 2, 1]], [[1, 2]]),
                        ([[1, 2, 1]], [[1, 0, 1]])):
        with pytest.raises(ValueError):
            opsum_route(states, ops)


def test_mpo_shapes_are_validated():
    from aqc_research_amd.mps_engine import MPO

    w = lambda a, b: np.ones((a, b, 2, 2))   # noqa: E731
    good = MPO([w(1, 3), w(3, 2), w(2, 1)])
    assert good.num_qubits == 3 and good.bond_dims.tolist() == [1, 3, 2, 1] and good.sites[1].dtype == np.complex128
    with pytest.raises((ValueError, AttributeError)):
        good.sites[0][0, 0, 0, 0] = 2.0                                  # immutable
    with pytest.raises(AttributeError):
        good.extra = 1
    for sites in ([], None, [w(2, 1)], [w(1, 2)], [w(1, 3), w(2, 1)], [np.ones((1, 1, 2))], [np.ones((1, 1, 2, 3))], [np.ones((1, 1, 3, 2))],
                  [np.ones((1, 0, 2, 2)), np.ones((0, 1, 2, 2))], w(1, 1)):
        with pytest.raises(ValueError):
            MPO(sites)
    for bad in (lambda: MPO.identity(0), lambda: MPO.xxz(0, 1.0), lambda: MPO.product_operator([]), lambda: MPO.product_operator([np.eye(3)]),
                lambda: MPO.from_pauli_string("XQ"), lambda: MPO.from_pauli_sum([]), lambda: MPO.from_pauli_sum([(1.0, "XX"), (1.0, "XXX")]),
                lambda: MPO.from_pauli_string(("X", (0,))), lambda: MPO.identity(13).to_dense()):
        with pytest.raises(ValueError):
            bad()
    assert MPO.from_pauli_string(("XZ", (0, 2)), num_qubits=3).bond_dims.tolist() == [1, 1, 1, 1]


def test_argument_errors_of_the_python_layer():
    """Raised before anything is uploaded: the states here are QiskitMPS tuples, and no device is touched."""
    from aqc_research_amd import mps_engine as me
    from aqc_research_amd import mps_observables as mo
    from tests import mps_obs_ref

    a = mps_obs_ref.hand_made([1, 2, 2, 1], 1)
    b = mps_obs_ref.hand_made([1, 2, 2, 1], 2)
    longer = mps_obs_ref.hand_made([1, 2, 2, 2, 1], 3)
    wide = mps_obs_ref.hand_made([1, 2, 13, 2, 1], 4)
    h3, h4 = me.MPO.xxz(3, 0.5), me.MPO.xxz(4, 0.5)
    for method in ("dense", 1, "Fused", "gemm"):
        with pytest.raises(ValueError):
            me.operator_sums([[(1.0, h3, a)]], method=method)
        with pytest.raises(ValueError):
            me.apply_operator(h3, a, method=method)
    for thr, cap in ((-1.0, 0), (float("nan"), 0), (float("inf"), 0), (0.0, -1)):
        with pytest.raises(ValueError):
            me.operator_sums([[(1.0, h3, a)]], thr, cap)
        with pytest.raises(ValueError):
            me.apply_operator(h3, [a, b], thr, cap)
    with pytest.raises(ValueError, match="4 qubits"):
        me.operator_sums([[(1.0, h4, a)]])                                # operator and state of different n
    with pytest.raises(ValueError):
        me.apply_operator(h3, longer)
    with pytest.raises(ValueError, match="qubits"):
        me.operator_sums([[(1.0, h3, a)], [(1.0, None, longer)]])         # states of different n
    with pytest.raises(ValueError, match="output 0"):
        me.operator_sums([[]])                                            # an empty output
    with pytest.raises(ValueError, match="output 1"):
        me.operator_sums([[(1.0, h3, a)], [(0.0, h3, a), (0.0, None, b)]])
    with pytest.raises(ValueError, match="fused.*output 0"):
        me.operator_sums([[(1.0, h4, wide)]], method="fused")             # 5 x 13 = 65
    with pytest.raises(ValueError, match="output 1"):
        me.operator_sums([[(1.0, None, wide)], [(1.0, h4, wide)]], method="fused")
    with pytest.raises(ValueError, match="fused"):
        me.apply_operator(h4, wide, method="fused")
    for outputs in ([], 42, [42], [[42]], [[(1.0, a)]], [[(1.0, h3, 42)]], [[(1.0, "h", a)]], [[(1.0, np.eye(2), a)]], [(1.0, h3, a)], "ab"):
        with pytest.raises(ValueError):
            me.operator_sums(outputs)
    for op, states in ((None, a), ("h", a), (h3, []), (h3, 42), (h3, [42])):
        with pytest.raises(ValueError):
            me.apply_operator(op, states)
    with pytest.raises(ValueError):
        mo.variance(a, "h")
    with pytest.raises(ValueError):
        mo.variance([], h3)
