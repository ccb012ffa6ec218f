"""
Measurement of matrix-product states in the computational basis on the GPU, without ever forming the dense vector (aqc_mps_sample,
aqc_mps_amplitudes; kernels: csrc/aqc_mps_sample.hip, rules: csrc/aqc_mps_sample_rule.h): shots drawn from |psi(b)|^2 and the
amplitudes psi(b) of given bit strings, for comparing a simulated state with the counts that come back from hardware.

``bits[s][q]`` is the value of qubit q, which is site q of the chain and index bit q of the dense vector.  Nothing is rescaled: an
amplitude is that of the state as it is, and ``p(b) = |psi(b)|^2 / <psi|psi>``.  The uniforms of shot s of lane l (the position of the
state in the call) are

    np.random.Generator(np.random.Philox(key=[seed, SAMPLE_STREAM], counter=[0, first_shot + s, l, 0])).random(n)

bit for bit, so a shot depends on (state, seed, lane, shot number) alone: not on the number of shots in the call, on ``first_shot``
splitting a run into chunks, or on the other states.  For another measurement basis apply the basis change with ``gate1`` first.

``states`` is a ``DeviceMPS``, a QiskitMPS tuple or a list of those, as in ``mps_observables``; a list gives results a leading lanes
axis.  Tuples are uploaded for the call and closed afterwards; states are taken in whatever gauge they are in and are never modified.
``method``: ``None`` lets the rule choose per state (``"fused"`` -- 64 shots per workgroup walk the whole chain inside one launch on the
fp64 matrix cores -- when every bond dimension is at most ``FUSED_CAP``, else ``"gemm"``).
"""
from ctypes import POINTER, c_uint8
from typing import Optional

import numpy as np

from . import _lib
from ._lib import check, dptr, iptr
from .mps_engine import _BOND_DIMS_OF_A_STATE, _Lanes, _method_code, _route_of, _within_fused_cap

FUSED_CAP = 64       # AQC_MPS_SAMPLE_FUSED_CAP of include/aqc_hip.h
SAMPLE_STREAM = 16   # AQC_SAMPLE_STREAM
MAX_SHOTS = 1 << 24
_METHODS = {None: 0, "fused": 1, "gemm": 2}   # AQC_MPS_SAMPLE_*
_ROUTES = {1: "fused", 2: "gemm"}


def _u8ptr(arr: np.ndarray):
    return arr.ctypes.data_as(POINTER(c_uint8))


def route(bond_dims) -> str:
    """The route the rule picks for a state with these n + 1 bond dimensions: ``"fused"`` or ``"gemm"``."""
    d = np.ascontiguousarray(bond_dims, dtype=np.int32)
    return _route_of("aqc_mps_sample_route", _ROUTES, _BOND_DIMS_OF_A_STATE, (d.size - 1, iptr(d)) if d.ndim == 1 else None)


def _count(value, name: str, low: int, high: int) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not low <= int(value) <= high:
        raise ValueError(f"{name} must be an integer in [{low}, {high}]")
    return int(value)


def sample(states, shots: int, *, seed: int, first_shot: int = 0, method: Optional[str] = None, details: bool = False):
    """``shots`` measurements of every state: ``bits``, uint8 of shape ``(shots, n)`` for one state, ``(lanes, shots, n)`` for a list.
    Row s is shot number ``first_shot + s``.  ``details``: a dict of ``bits``, ``amplitudes`` (psi of every sampled string),
    ``probabilities`` (= |amplitude|^2 / norm2) and ``norm2`` (= <psi|psi>, a float or one per lane)."""
    shots = _count(shots, "shots", 1, MAX_SHOTS)
    seed = _count(seed, "seed", 0, 2 ** 64 - 1)
    first_shot = _count(first_shot, "first_shot", 0, 2 ** 64 - 1 - MAX_SHOTS)
    code = _method_code(method, _METHODS)
    lanes = _Lanes(states)
    _within_fused_cap(method, lanes.dims, FUSED_CAP)
    count, single = len(lanes.items), lanes.single
    bits = np.empty((count, shots, lanes.n), dtype=np.uint8)
    amps = np.empty((count, shots), dtype=np.complex128) if details else None
    norm2 = np.empty(count, dtype=np.float64) if details else None
    with lanes:
        check(_lib.lib().aqc_mps_sample(lanes.handles(), count, shots, first_shot, seed, code, _u8ptr(bits), dptr(amps) if details else None,
                                        dptr(norm2) if details else None))
    if not details:
        return bits[0] if single else bits
    prob = (amps.real ** 2 + amps.imag ** 2) / norm2[:, None]
    out = {"bits": bits, "amplitudes": amps, "probabilities": prob, "norm2": norm2}
    return {k: (v[0] if k != "norm2" else float(v[0])) for k, v in out.items()} if single else out


def amplitudes(states, bits, *, method: Optional[str] = None) -> np.ndarray:
    """psi(b) of the S bit strings ``bits`` (shape ``(S, n)``, values 0 / 1): complex128 of shape ``(S,)`` for one state, ``(lanes, S)``
    for a list."""
    arr = np.asarray(bits)
    if arr.ndim != 2 or arr.shape[0] < 1 or not (np.issubdtype(arr.dtype, np.integer) or arr.dtype == np.bool_):
        raise ValueError("expects a non-empty (S, n) array of bits")
    if arr.shape[0] > MAX_SHOTS:
        raise ValueError(f"at most {MAX_SHOTS} bit strings per call")
    if arr.size and (arr.min() < 0 or arr.max() > 1):
        raise ValueError("a bit is 0 or 1")
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    code = _method_code(method, _METHODS)
    lanes = _Lanes(states)
    _within_fused_cap(method, lanes.dims, FUSED_CAP)
    if arr.shape[1] != lanes.n:
        raise ValueError(f"the bit strings have {arr.shape[1]} bits, the states {lanes.n} qubits")
    out = np.empty((len(lanes.items), arr.shape[0]), dtype=np.complex128)
    with lanes:
        check(_lib.lib().aqc_mps_amplitudes(lanes.handles(), len(lanes.lanes), arr.shape[0], _u8ptr(arr), code, dptr(out)))
    return out[0] if lanes.single else out


def counts(bits):
    """``(rows, multiplicities)``: the distinct bit strings of ``bits`` (shape ``(S, n)``) in lexicographic order of their rows, and how
    often each occurs (host, NumPy)."""
    arr = np.asarray(bits)
    if arr.ndim != 2:
        raise ValueError("expects an (S, n) array of bits")
    rows, mult = np.unique(arr, axis=0, return_counts=True)
    return rows, mult
