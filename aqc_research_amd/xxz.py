"""
The XXZ chain Hamiltonian without its matrix, and exact time evolution under it, on the GPU (aqc_xxz_mul_vec / aqc_xxz_energy /
aqc_xxz_evolve; kernels: csrc/aqc_xxz.hip, rules: csrc/aqc_xxz_rule.h):

    H = -1/4 sum_{i=0}^{n-2} (X_i X_{i+1} + Y_i Y_{i+1} + delta Z_i Z_{i+1})        (make_hamiltonian, trotter.py:183-230)
    exp(-i H t) psi = sum_{k=0}^{K} c_k T_k(H / R) psi,  R = (n - 1)(1/2 + |delta| / 4),  c_0 = J_0(R t),  c_k = 2 (-i)^k J_k(R t)

States are C-contiguous complex128 arrays in host memory, ``(2^n,)`` or ``(lanes, 2^n)`` with 2 <= n <= 30; index bit q is qubit q.
Inputs are never modified and results are fresh arrays.  The series is exact to rounding at any time the drivers use, where the
reference's ``exact_evolution`` (a dense ``expm``) ends near 12 qubits.
"""
from typing import Optional

import numpy as np

from . import _lib
from ._lib import check, dptr, iptr
from .gates import _dev

MIN_QUBITS, MAX_QUBITS = 2, 30


def _lanes_of(states: np.ndarray):
    """(n, lanes or None) of a state vector (2^n,) or a stack of them (lanes, 2^n); the checks of ``gates.shape_of``."""
    if not (isinstance(states, np.ndarray) and states.dtype == np.complex128 and states.flags.c_contiguous and states.ndim in (1, 2)):
        raise TypeError("expects a C-contiguous complex128 state vector or a (lanes, 2^n) stack of them")
    dim = int(states.shape[-1])
    n = dim.bit_length() - 1
    if dim < 4 or (1 << n) != dim or n > MAX_QUBITS:
        raise ValueError(f"the state dimension must be 2^n with {MIN_QUBITS} <= n <= {MAX_QUBITS}")
    if states.ndim == 2 and states.shape[0] < 1:
        raise ValueError("expects at least one lane")
    return n, (None if states.ndim == 1 else int(states.shape[0]))


def _finite(value, name: str) -> float:
    value = float(value)
    if not np.isfinite(value):
        raise ValueError(f"{name} must be finite")
    return value


def spectral_radius(num_qubits: int, delta: float) -> float:
    """R = (n - 1)(1/2 + |delta| / 4) >= ||H||: every bond term has norm 1/2 + |delta| / 4."""
    if not (isinstance(num_qubits, (int, np.integer)) and MIN_QUBITS <= num_qubits <= MAX_QUBITS):
        raise ValueError(f"num_qubits must be an integer in [{MIN_QUBITS}, {MAX_QUBITS}]")
    return float(num_qubits - 1) * (0.5 + 0.25 * abs(_finite(delta, "delta")))


def xxz_mul_vec(states: np.ndarray, delta: float, *, device: Optional[int] = None) -> np.ndarray:
    """H psi for one state or for every lane, the same shape as ``states``."""
    n, lanes = _lanes_of(states)
    delta = _finite(delta, "delta")
    out = np.empty_like(states)
    check(_lib.lib().aqc_xxz_mul_vec(_dev(device), n, lanes or 1, delta, dptr(states), dptr(out)))
    return out


def xxz_energy(states: np.ndarray, delta: float, *, device: Optional[int] = None):
    """Re <psi|H|psi>: a float for a 1-D state, float64[lanes] for a stack.  Summed in a fixed order: two calls give the same bits."""
    n, lanes = _lanes_of(states)
    delta = _finite(delta, "delta")
    out = np.empty(lanes or 1, dtype=np.float64)
    check(_lib.lib().aqc_xxz_energy(_dev(device), n, lanes or 1, delta, dptr(states), dptr(out)))
    return float(out[0]) if lanes is None else out


def xxz_evolve(states: np.ndarray, delta: float, evol_time, *, device: Optional[int] = None, details: bool = False):
    """exp(-i H t) psi.

    ``evol_time`` is a scalar or a 1-D array (any sign, zero included):
      * 1-D ``states``, scalar time      -> ``(2^n,)``
      * 1-D ``states``, L times          -> ``(L, 2^n)``; the state is shared and uploaded once
      * ``(lanes, 2^n)``, scalar time    -> the same time on every lane
      * ``(lanes, 2^n)``, ``lanes`` times -> lane l evolves by ``evol_time[l]``
    Lanes share the kernel launches, one per term of the longest series.  ``details=True`` also returns
    ``{"terms": int32[lanes], "radius": float}``: the series length K of every lane and R."""
    n, lanes = _lanes_of(states)
    delta = _finite(delta, "delta")
    times = np.asarray(evol_time, dtype=np.float64)
    if times.ndim > 1:
        raise ValueError("evol_time must be a scalar or a 1-D array")
    if not np.all(np.isfinite(times)):
        raise ValueError("evol_time must be finite")
    shared = lanes is None
    if times.ndim == 0:
        times = np.full(lanes or 1, float(times))
        out_shape = states.shape
    else:
        if times.size < 1:
            raise ValueError("evol_time is empty")
        if not shared and times.size != lanes:
            raise ValueError(f"{lanes} lanes but {times.size} evolution times")
        out_shape = (times.size, states.shape[-1])
    times = np.ascontiguousarray(times)
    out = np.empty(out_shape, dtype=np.complex128)
    terms = np.zeros(times.size, dtype=np.int32)
    check(_lib.lib().aqc_xxz_evolve(_dev(device), n, int(times.size), int(shared), delta, dptr(times), dptr(states), dptr(out),
                                    iptr(terms)))
    if details:
        return out, {"terms": terms, "radius": spectral_radius(n, delta)}
    return out
