"""The NumPy statement of reduced density matrices and of the Pauli algebra on them: what aqc_research_amd/observables.py and
csrc/aqc_obs.hip are tested against.  Written without the kernel's decomposition (no tiles, no 4-qubit sets, no partial traces).

Convention: state index bit q is qubit q.  For listed qubits (q_0, ..., q_{k-1}) the row index has bit m = the value of q_m:
    rho[a][b] = sum_rest psi(rest, a) conj psi(rest, b)
"""
import numpy as np

PAULI = {
    "i": np.eye(2, dtype=np.complex128),
    "x": np.array([[0, 1], [1, 0]], dtype=np.complex128),
    "y": np.array([[0, -1j], [1j, 0]], dtype=np.complex128),
    "z": np.array([[1, 0], [0, -1]], dtype=np.complex128),
}


def rdm(psi: np.ndarray, qubits) -> np.ndarray:
    """The reduced density matrix of the listed qubits of one state vector."""
    n = psi.size.bit_length() - 1
    k = len(qubits)
    t = psi.reshape((2,) * n)                                       # axis a is qubit n - 1 - a
    # the listed qubits to the front, the last listed one first: it is the highest bit of the row index
    t = np.moveaxis(t, [n - 1 - q for q in reversed(qubits)], range(k))
    a = t.reshape(2**k, -1)
    return a @ a.conj().T


def pair_rdms(states: np.ndarray, pairs) -> np.ndarray:
    """(P, 4, 4) for a 1-D state, (lanes, P, 4, 4) for a stack."""
    if states.ndim == 1:
        return np.stack([rdm(states, p) for p in pairs])
    return np.stack([np.stack([rdm(s, p) for p in pairs]) for s in states])


def all_pairs(n: int):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def pauli_on_rdm(letters: str) -> np.ndarray:
    """The operator of a Pauli string on the row index of rdm(psi, qubits): letter m acts on listed qubit m = index bit m."""
    op = np.ones((1, 1), dtype=np.complex128)
    for c in letters.lower():
        op = np.kron(PAULI[c], op)
    return op


def expectation(rho: np.ndarray, letters: str) -> float:
    return float(np.trace(rho @ pauli_on_rdm(letters)).real)


def dense_pauli(n: int, placed: dict) -> np.ndarray:
    """The 2^n x 2^n matrix of the Paulis ``placed`` = {qubit: letter}: qubit q is index bit q, so it is factor n - 1 - q of the
    Kronecker product."""
    op = np.ones((1, 1), dtype=np.complex128)
    for q in range(n - 1, -1, -1):
        op = np.kron(op, PAULI[placed.get(q, "i")])
    return op


def dense_expectation(psi: np.ndarray, placed: dict) -> float:
    n = psi.size.bit_length() - 1
    return float(np.vdot(psi, dense_pauli(n, placed) @ psi).real)
