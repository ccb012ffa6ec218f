"""
One- and two-site observables of state vectors from reduced density matrices computed on the GPU (aqc_obs_rdm; kernel:
csrc/aqc_obs.hip, plan and partial trace: csrc/aqc_obs_rule.h).

Index convention: state index bit q is qubit q, as everywhere in the package.  For listed qubits ``(q_0, ..., q_{k-1})`` the matrix's
row index has bit m = the value of q_m:

    rho[a][b] = sum_rest psi(rest, a) conj psi(rest, b)

so ``pair_density_matrices(psi, [(j, i)])`` is that of ``(i, j)`` with its two index bits transposed.  States are C-contiguous
complex128 arrays in host memory, ``(2^n,)`` or ``(lanes, 2^n)`` with 2 <= n <= 30 (the checks of ``xxz._lanes_of``); inputs are never
modified.  Every sum runs in a fixed order that does not depend on the number of lanes: lane l of a stack equals the one-state call bit
for bit.  The matrices are exactly Hermitian.

Device calls: ``pair_density_matrices``, ``reduced_density_matrix`` (and ``plan``, which needs no device).  The rest is NumPy on their
results: ``pauli_expectation``, ``magnetisation``, ``correlation_matrix``, ``bond_energies``.
"""
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check, dptr, iptr
from .gates import _dev
from .xxz import _finite, _lanes_of

TILE_BITS, LOW_BITS, MAX_SUBSETS = 11, 5, 16   # AQC_OBS_* of include/aqc_hip.h

_PAULI = {
    "i": np.eye(2, dtype=np.complex128),
    "x": np.array([[0, 1], [1, 0]], dtype=np.complex128),
    "y": np.array([[0, -1j], [1j, 0]], dtype=np.complex128),
    "z": np.array([[1, 0], [0, -1]], dtype=np.complex128),
}


def _qubit_sets(qubits, n: int, k: Optional[int] = None) -> np.ndarray:
    """int32[nsets][k] of different qubits below n each."""
    sets = np.asarray(qubits)
    if sets.ndim != 2 or sets.shape[0] < 1 or sets.shape[1] < 1 or not np.issubdtype(sets.dtype, np.integer):
        raise ValueError("expects a non-empty list of equally long tuples of qubit numbers")
    if k is not None and sets.shape[1] != k:
        raise ValueError(f"expects tuples of {k} qubits")
    if sets.shape[1] > min(4, n):
        raise ValueError(f"a reduced density matrix takes 1 to {min(4, n)} qubits here, not {sets.shape[1]}")
    if sets.min() < 0 or sets.max() >= n:
        raise ValueError(f"qubit out of range: {n} qubits")
    ordered = np.sort(sets, axis=1)
    if np.any(ordered[:, 1:] == ordered[:, :-1]):
        raise ValueError("a qubit is listed twice in one tuple")
    return np.ascontiguousarray(sets, dtype=np.int32)


def plan(num_qubits: int, pairs: Sequence[Sequence[int]]) -> dict:
    """The passes over the state that ``pair_density_matrices(states, pairs)`` makes (aqc_obs_plan; no device needed):
    ``{"passes": [qubits of the pass, ascending], "subsets": [per pass a list of 4-tuples of tile-local positions], "serves":
    [(pass, subset within the pass) per pair]}``.  Tile-local position j is the j-th lowest qubit of the pass."""
    if not (isinstance(num_qubits, (int, np.integer)) and 2 <= num_qubits <= 30):
        raise ValueError("num_qubits must be an integer in [2, 30]")
    sets = _qubit_sets(pairs, int(num_qubits), 2)
    npairs = sets.shape[0]
    cap = npairs   # every pass and every subset serves at least one pair that none before it served
    npasses, nsubsets = np.zeros(1, np.int32), np.zeros(1, np.int32)
    pass_bits = np.zeros((cap, TILE_BITS), np.int32)
    pass_nsub = np.zeros(cap, np.int32)
    subsets = np.zeros((cap, 4), np.int32)
    serves = np.zeros((npairs, 2), np.int32)
    check(_lib.lib().aqc_obs_plan(int(num_qubits), npairs, iptr(sets), cap, cap, iptr(npasses), iptr(nsubsets), iptr(pass_bits),
                                  iptr(pass_nsub), iptr(subsets), iptr(serves)))
    first = np.concatenate(([0], np.cumsum(pass_nsub[: npasses[0]])))
    return {
        "passes": [[int(q) for q in row if q >= 0] for row in pass_bits[: npasses[0]]],
        "subsets": [[tuple(int(v) for v in s) for s in subsets[first[p]: first[p + 1]]] for p in range(int(npasses[0]))],
        "serves": [(int(p), int(s)) for p, s in serves],
    }


def _rdm(states: np.ndarray, sets: np.ndarray, device: Optional[int]) -> np.ndarray:
    n, lanes = _lanes_of(states)
    nsets, k = sets.shape
    out = np.empty((lanes or 1, nsets, 1 << k, 1 << k), dtype=np.complex128)
    check(_lib.lib().aqc_obs_rdm(_dev(device), n, lanes or 1, dptr(states), int(k), int(nsets), iptr(sets), dptr(out)))
    return out[0] if lanes is None else out


def pair_density_matrices(states: np.ndarray, pairs=None, *, device: Optional[int] = None) -> np.ndarray:
    """The two-qubit reduced density matrices of ``pairs`` (``None``: all i < j in lexicographic order): ``(P, 4, 4)`` for a 1-D state,
    ``(lanes, P, 4, 4)`` for a stack.  For the pair (i, j) the row index is ``value(i) + 2 value(j)``."""
    n, _ = _lanes_of(states)
    if pairs is None:
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    return _rdm(states, _qubit_sets(pairs, n, 2), device)


def reduced_density_matrix(states: np.ndarray, qubits: Sequence[int], *, device: Optional[int] = None) -> np.ndarray:
    """The reduced density matrix of 1 to 4 listed qubits: ``(2^k, 2^k)`` for a 1-D state, ``(lanes, 2^k, 2^k)`` for a stack."""
    n, lanes = _lanes_of(states)
    qs = np.asarray(qubits)
    if qs.ndim != 1:
        raise ValueError("expects a flat list of 1 to 4 qubit numbers")
    out = _rdm(states, _qubit_sets(qs[None, :], n), device)
    return out[0] if lanes is None else out[:, 0]


def pauli_matrix(letters: str) -> np.ndarray:
    """The operator of a Pauli string on the row index of a reduced density matrix: letter m acts on listed qubit m (index bit m)."""
    if not isinstance(letters, str) or not letters or any(c not in _PAULI for c in letters.lower()):
        raise ValueError(f"a Pauli string holds the letters I, X, Y, Z, not {letters!r}")
    op = np.ones((1, 1), dtype=np.complex128)
    for c in letters.lower():   # later letters are higher index bits: they go to the left of the Kronecker product
        op = np.kron(_PAULI[c], op)
    return op


def pauli_expectation(rdm: np.ndarray, letters: str):
    """tr(rho P) for the Pauli string ``letters`` (letter m on listed qubit m): a float, or an array over the leading axes of ``rdm``."""
    op = pauli_matrix(letters)
    rdm = np.asarray(rdm)
    if rdm.ndim < 2 or rdm.shape[-2:] != op.shape:
        raise ValueError(f"{len(letters)} letters need density matrices of shape (..., {op.shape[0]}, {op.shape[0]})")
    val = np.einsum("...ab,ba->...", rdm, op).real
    return float(val) if val.ndim == 0 else val


def _single_axis(axis: str) -> str:
    if not isinstance(axis, str) or axis.lower() not in ("x", "y", "z"):
        raise ValueError(f"axis must be 'x', 'y' or 'z', not {axis!r}")
    return axis.lower()


# ---- derived observables: which pairs each one asks for, and the arithmetic on the matrices that come back.  Stated once, for the
# dense states here and for the matrix-product states of mps_observables.py: the two modules differ only in how rho is obtained.
def _magnetisation_pairs(n: int) -> list:
    return [(q, q + 1) for q in range(0, n - 1, 2)] + ([(n - 2, n - 1)] if n % 2 else [])


def _magnetisation_of(rho: np.ndarray, n: int, a: str) -> np.ndarray:
    first, second = np.atleast_1d(pauli_expectation(rho, a + "i")), np.atleast_1d(pauli_expectation(rho, "i" + a))
    out = np.empty(rho.shape[:-3] + (n,), dtype=np.float64)
    half = n // 2
    out[..., 0:2 * half:2] = first[..., :half]
    out[..., 1:2 * half:2] = second[..., :half]
    if n % 2:
        out[..., n - 1] = second[..., half]
    return out


def _correlation_pairs(n: int) -> list:
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def _correlation_of(rho: np.ndarray, n: int, a: str, b: str, connected: bool) -> np.ndarray:
    pairs = _correlation_pairs(n)
    upper, lower = np.atleast_1d(pauli_expectation(rho, a + b)), np.atleast_1d(pauli_expectation(rho, b + a))   # <a_i b_j> and <b_i a_j> for i < j
    out = np.empty(rho.shape[:-3] + (n, n), dtype=np.float64)
    iu = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    out[..., iu[0], iu[1]] = upper
    out[..., iu[1], iu[0]] = lower
    out[..., np.arange(n), np.arange(n)] = 1.0 if a == b else 0.0
    if connected:
        # single-site values from the leading pairs (0, 1), (0, 2), ..., (0, n - 1): qubit 0 from the first, qubit q from (0, q)
        lead = rho[..., : n - 1, :, :]
        ma, mb = (np.concatenate((np.atleast_1d(pauli_expectation(lead[..., :1, :, :], c + "i")), np.atleast_1d(pauli_expectation(lead, "i" + c))), axis=-1)
                  for c in (a, b))
        out = out - ma[..., :, None] * mb[..., None, :]
    return out


def _correlation_letters(letters: str):
    if not isinstance(letters, str) or len(letters) != 2:
        raise ValueError("letters must name two axes, such as 'zz'")
    return _single_axis(letters[0]), _single_axis(letters[1])


def _bond_pairs(n: int) -> list:
    return [(q, q + 1) for q in range(n - 1)]


def _bond_energies_of(rho: np.ndarray, delta: float) -> np.ndarray:
    op = -0.25 * (pauli_matrix("xx") + pauli_matrix("yy") + delta * pauli_matrix("zz"))
    return np.einsum("...ab,ba->...", rho, op).real


def magnetisation(states: np.ndarray, axis: str = "z", *, device: Optional[int] = None) -> np.ndarray:
    """<sigma_i> along ``axis`` for every qubit: ``(n,)`` or ``(lanes, n)``.  Read from the ceil(n / 2) pairs (0, 1), (2, 3), ...
    (the last qubit of an odd chain with its left neighbour)."""
    a = _single_axis(axis)
    n, _ = _lanes_of(states)
    return _magnetisation_of(pair_density_matrices(states, _magnetisation_pairs(n), device=device), n, a)


def correlation_matrix(states: np.ndarray, letters: str = "zz", connected: bool = False, *, device: Optional[int] = None) -> np.ndarray:
    """C[i][j] = <a_i b_j> for ``letters = "ab"`` out of x, y, z, over all pairs: ``(n, n)`` or ``(lanes, n, n)``.  The diagonal is 1
    (a_i a_i = 1; for two different letters a_i b_i = +-i c_i, whose real part is 0).  ``connected``: minus <a_i><b_j>."""
    a, b = _correlation_letters(letters)
    n, _ = _lanes_of(states)
    return _correlation_of(pair_density_matrices(states, _correlation_pairs(n), device=device), n, a, b, connected)


def bond_energies(states: np.ndarray, delta: float, *, device: Optional[int] = None) -> np.ndarray:
    """-1/4 tr rho_{i,i+1} (XX + YY + delta ZZ) for the n - 1 bonds of the open XXZ chain: ``(n - 1,)`` or ``(lanes, n - 1)``.  Their
    sum is the energy ``xxz.xxz_energy(states, delta)``."""
    delta = _finite(delta, "delta")
    n, _ = _lanes_of(states)
    return _bond_energies_of(pair_density_matrices(states, _bond_pairs(n), device=device), delta)
