"""
One- and two-site observables of matrix-product states from pair density matrices computed on the GPU without ever forming the dense
vector (aqc_mps_obs_pairs; kernels: csrc/aqc_mps_obs.hip, rules: csrc/aqc_mps_obs_rule.h): ``observables.py`` for registers beyond
dense reach.

Conventions are those of ``observables.py``: for the pair (i, j) the row index is ``value(i) + 2 value(j)``,

    rho[a][b] = sum_rest psi(rest, a) conj psi(rest, b)

with no normalisation (``tr rho = <psi|psi>``), so ``(j, i)`` gives the matrix of ``(i, j)`` with its two index bits transposed.

``states`` is a ``DeviceMPS``, a QiskitMPS tuple (``DenseBackedMPS`` included) or a list of those; a list gives results a leading lanes
axis.  Tuples are uploaded for the call and closed afterwards; states are taken in whatever gauge they are in and are never modified.
All pairs with the same lower qubit share one walk along the chain (``plan``).  ``method``: ``None`` lets the rule choose per state
(``"fused"`` -- the whole walk of a chain inside one launch -- when every bond dimension is at most ``FUSED_CAP``, else ``"gemm"``).
Every matrix is exactly Hermitian, and a pair's matrix does not depend on which other pairs or states are in the call: lane l of a
list equals the one-state call bit for bit.

Device calls: ``pair_density_matrices``, ``reduced_density_matrix`` (and ``plan``, which needs no device).  The rest is NumPy on
their results.
"""
from ctypes import c_void_p
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check, dptr, iptr
from .mps_engine import DeviceMPS
from .observables import (_bond_energies_of, _bond_pairs, _correlation_letters, _correlation_of, _correlation_pairs, _magnetisation_of,
                          _magnetisation_pairs, _single_axis, pauli_expectation, pauli_matrix)  # noqa: F401  (the last two: for callers)
from .xxz import _finite

FUSED_CAP = 64   # AQC_MPS_OBS_FUSED_CAP of include/aqc_hip.h
_METHODS = {None: 0, "fused": 1, "gemm": 2}   # AQC_MPS_OBS_*


def _pairs(pairs, n: int) -> np.ndarray:
    """int32[npairs][2] of two different qubits below n each."""
    arr = np.asarray(pairs)
    if arr.ndim != 2 or arr.shape[0] < 1 or arr.shape[1] != 2 or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError("expects a non-empty list of pairs of qubit numbers")
    if arr.min() < 0 or arr.max() >= n:
        raise ValueError(f"qubit out of range: {n} qubits")
    if np.any(arr[:, 0] == arr[:, 1]):
        raise ValueError("a qubit is listed twice in one pair")
    return np.ascontiguousarray(arr, dtype=np.int32)


def plan(num_qubits: int, pairs: Sequence[Sequence[int]]) -> dict:
    """The walks that ``pair_density_matrices(states, pairs)`` makes (aqc_mps_obs_plan; no device needed): ``{"chains": {start site:
    last site}, "emissions": number of different (chain, site) matrices, "serves": [(chain, emitting site, transposed) per pair]}``."""
    if not (isinstance(num_qubits, (int, np.integer)) and num_qubits >= 2):
        raise ValueError("num_qubits must be an integer >= 2")
    n = int(num_qubits)
    arr = _pairs(pairs, n)
    last = np.zeros(n, np.int32)
    nemits = np.zeros(1, np.int32)
    serves = np.zeros((arr.shape[0], 3), np.int32)
    check(_lib.lib().aqc_mps_obs_plan(n, arr.shape[0], iptr(arr), iptr(last), iptr(nemits), iptr(serves)))
    return {
        "chains": {int(i): int(e) for i, e in enumerate(last) if e >= 0},
        "emissions": int(nemits[0]),
        "serves": [(int(c), int(s), bool(t)) for c, s, t in serves],
    }


def route(bond_dims) -> str:
    """The route the rule picks for a state with these n + 1 bond dimensions: ``"fused"`` or ``"gemm"``."""
    d = np.ascontiguousarray(bond_dims, dtype=np.int32)
    r = _lib.lib().aqc_mps_obs_route(d.size - 1, iptr(d))
    if r not in (1, 2):
        raise ValueError("expects the n + 1 bond dimensions of a state")
    return "fused" if r == 1 else "gemm"


def _is_tuple_state(s) -> bool:
    return isinstance(s, tuple) and len(s) == 2   # a QiskitMPS (gammas, lambdas); several states come as a list


class _Lanes:
    """The states of a call as DeviceMPS handles; what was uploaded for the call is closed on exit."""

    def __init__(self, states):
        self.single = isinstance(states, DeviceMPS) or _is_tuple_state(states)
        if not self.single and not isinstance(states, list):
            raise ValueError("states is a DeviceMPS, a QiskitMPS tuple or a list of those")
        self.items = [states] if self.single else list(states)
        if not self.items:
            raise ValueError("expects at least one state")
        self.own = []
        self.lanes = []

    def __enter__(self):
        try:
            for s in self.items:
                if isinstance(s, DeviceMPS):
                    if not s.handle:
                        raise ValueError("a closed DeviceMPS")
                    self.lanes.append(s)
                elif _is_tuple_state(s):
                    m = DeviceMPS.from_qiskit(s, assume_canonical=True)   # exact arithmetic: the gauge is taken as it is
                    self.own.append(m)
                    self.lanes.append(m)
                else:
                    raise ValueError("a state is a DeviceMPS or a QiskitMPS tuple")
        except Exception:
            self.__exit__(None, None, None)
            raise
        n = self.lanes[0].num_qubits
        if any(m.num_qubits != n for m in self.lanes):
            self.__exit__(None, None, None)
            raise ValueError("the states differ in the number of qubits")
        return self

    def __exit__(self, *exc):
        for m in self.own:
            m.close()
        self.own = []
        return False


def _rdms(lanes: _Lanes, arr: np.ndarray, method: Optional[str]) -> np.ndarray:
    if method not in _METHODS:
        raise ValueError(f"method must be None, 'fused' or 'gemm', not {method!r}")
    if method == "fused":
        for m in lanes.lanes:
            if int(m.bond_dims.max()) > FUSED_CAP:
                raise ValueError(f"the fused route takes bond dimensions up to {FUSED_CAP}, not {int(m.bond_dims.max())}")
    handles = (c_void_p * len(lanes.lanes))(*[m.handle for m in lanes.lanes])
    out = np.empty((len(lanes.lanes), arr.shape[0], 4, 4), dtype=np.complex128)
    check(_lib.lib().aqc_mps_obs_pairs(handles, len(lanes.lanes), arr.shape[0], iptr(arr), _METHODS[method], dptr(out)))
    return out[0] if lanes.single else out


def pair_density_matrices(states, pairs=None, *, method: Optional[str] = None) -> np.ndarray:
    """The two-qubit reduced density matrices of ``pairs`` (``None``: all i < j in lexicographic order): ``(P, 4, 4)`` for one state,
    ``(lanes, P, 4, 4)`` for a list."""
    with _Lanes(states) as lanes:
        n = lanes.lanes[0].num_qubits
        if n < 2:
            raise ValueError("pair density matrices need at least 2 qubits")
        if pairs is None:
            pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
        return _rdms(lanes, _pairs(pairs, n), method)


def reduced_density_matrix(states, qubits: Sequence[int], *, method: Optional[str] = None) -> np.ndarray:
    """The reduced density matrix of 1 or 2 listed qubits: ``(2^k, 2^k)`` for one state, ``(lanes, 2^k, 2^k)`` for a list.  One qubit
    is read from the pair with a neighbour, whose other qubit is traced out."""
    qs = np.asarray(qubits)
    if qs.ndim != 1 or qs.size not in (1, 2) or not np.issubdtype(qs.dtype, np.integer):
        raise ValueError("expects a flat list of 1 or 2 qubit numbers")
    with _Lanes(states) as lanes:
        n = lanes.lanes[0].num_qubits
        if n < 2:
            raise ValueError("pair density matrices need at least 2 qubits")
        if qs.size == 2:
            out = _rdms(lanes, _pairs(qs[None, :], n), method)
            return out[0] if lanes.single else out[:, 0]
        q = int(qs[0])
        if not 0 <= q < n:
            raise ValueError(f"qubit out of range: {n} qubits")
        other = q + 1 if q + 1 < n else q - 1
        rho = _rdms(lanes, _pairs([(q, other)], n), method)
        rho = rho[0] if lanes.single else rho[:, 0]
        r = rho.reshape(rho.shape[:-2] + (2, 2, 2, 2))   # [other][q][other'][q']
        return r[..., 0, :, 0, :] + r[..., 1, :, 1, :]




def _rho_of(states, pairs_of, method: Optional[str]):
    """``(rho, n)``: the matrices of the pairs ``pairs_of(n)`` that a derived observable of ``observables.py`` asks for."""
    with _Lanes(states) as lanes:
        n = lanes.lanes[0].num_qubits
        return _rdms(lanes, _pairs(pairs_of(n), n), method), n


def magnetisation(states, axis: str = "z", *, method: Optional[str] = None) -> np.ndarray:
    """<sigma_i> along ``axis`` for every qubit: ``(n,)`` or ``(lanes, n)``.  Read from the ceil(n / 2) pairs (0, 1), (2, 3), ...
    (the last qubit of an odd chain with its left neighbour).  Not divided by <psi|psi>."""
    a = _single_axis(axis)
    rho, n = _rho_of(states, _magnetisation_pairs, method)
    return _magnetisation_of(rho, n, a)


def correlation_matrix(states, letters: str = "zz", connected: bool = False, *, method: Optional[str] = None) -> np.ndarray:
    """C[i][j] = <a_i b_j> for ``letters = "ab"`` out of x, y, z, over all pairs: ``(n, n)`` or ``(lanes, n, n)``.  The diagonal is 1
    for equal letters and 0 otherwise, as in ``observables.correlation_matrix``.  ``connected``: minus <a_i><b_j>."""
    a, b = _correlation_letters(letters)
    rho, n = _rho_of(states, _correlation_pairs, method)
    return _correlation_of(rho, n, a, b, connected)


def bond_energies(states, delta: float, *, method: Optional[str] = None) -> np.ndarray:
    """-1/4 tr rho_{i,i+1} (XX + YY + delta ZZ) for the n - 1 bonds of the open XXZ chain: ``(n - 1,)`` or ``(lanes, n - 1)``."""
    delta = _finite(delta, "delta")
    rho, _ = _rho_of(states, _bond_pairs, method)
    return _bond_energies_of(rho, delta)
