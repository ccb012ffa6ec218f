"""The NumPy statement of Pauli strings between matrix-product states, <phi|P|psi>, twice: what aqc_research_amd/mps_observables.py
(pauli_strings, overlaps, energy) and csrc/aqc_mps_pauli.hip are tested against.  tests/test_mps_pauli_ref.py holds the two to each other.

States are QiskitMPS tuples read as tests/mps_obs_ref.site_tensors reads them: psi(b) = T_0[b_0] ... T_{n-1}[b_{n-1}], any gauge.  A
string is a sequence of n letters 0, 1, 2, 3 = I, X, Y, Z; entry q acts on qubit q = site q = index bit q of the dense vector.  Nothing
is normalised."""
import numpy as np

from tests import mps_obs_ref

PAULI = (
    np.eye(2, dtype=np.complex128),
    np.array([[0, 1], [1, 0]], dtype=np.complex128),
    np.array([[0, -1j], [1j, 0]], dtype=np.complex128),
    np.array([[1, 0], [0, -1]], dtype=np.complex128),
)


def by_transfer(bra, ket, strings) -> np.ndarray:
    """(S,) complex128: the transfer-matrix walk, site by site with plain matrix products, over the whole chain:
    M' = sum_{a,c} P[a][c] B[a]^H M T[c]."""
    bs, ts = mps_obs_ref.site_tensors(bra), mps_obs_ref.site_tensors(ket)
    out = np.empty(len(strings), dtype=np.complex128)
    for s, string in enumerate(strings):
        m = np.ones((1, 1), dtype=np.complex128)
        for q, letter in enumerate(string):
            p = PAULI[int(letter)]
            m = sum(p[a, c] * (bs[q][a].conj().T @ m @ ts[q][c]) for a in range(2) for c in range(2) if p[a, c] != 0)
        out[s] = m[0, 0]
    return out


def apply_dense(psi: np.ndarray, string) -> np.ndarray:
    """P psi by bit flips and signs on the dense vector."""
    n = psi.size.bit_length() - 1
    idx = np.arange(psi.size)
    out = np.array(psi, dtype=np.complex128)
    for q, letter in enumerate(string):
        bit = (idx >> q) & 1
        if letter == 1:
            out = out[idx ^ (1 << q)]
        elif letter == 2:                  # Y|0> = i|1>, Y|1> = -i|0>: the new amplitude at bit value 1 is i times the old one at 0
            out = out[idx ^ (1 << q)] * np.where(bit == 1, 1j, -1j)
        elif letter == 3:
            out = out * np.where(bit == 1, -1.0, 1.0)
        elif letter != 0:
            raise ValueError("a letter is 0, 1, 2 or 3")
    assert len(string) == n
    return out


def by_dense(bra, ket, strings, dense_bra=None, dense_ket=None) -> np.ndarray:
    """(S,) complex128: np.vdot of the dense bra with the letters applied to the dense ket."""
    phi = mps_obs_ref.dense(bra) if dense_bra is None else dense_bra
    psi = mps_obs_ref.dense(ket) if dense_ket is None else dense_ket
    return np.array([np.vdot(phi, apply_dense(psi, s)) for s in strings], dtype=np.complex128)


def ref_strings(n: int, seed: int, random_count: int = 40) -> np.ndarray:
    """uint8 (S, n): identity, each letter alone at site 0, in the middle and at n - 1, all-Y, and ``random_count`` random strings of
    weight 1 .. n."""
    rng = np.random.default_rng(seed)
    rows = [np.zeros(n, dtype=np.uint8)]
    for q in sorted({0, n // 2, n - 1}):
        for letter in (1, 2, 3):
            r = np.zeros(n, dtype=np.uint8)
            r[q] = letter
            rows.append(r)
    rows.append(np.full(n, 2, dtype=np.uint8))
    for k in range(random_count):
        r = np.zeros(n, dtype=np.uint8)
        weight = 1 + k % n
        r[rng.choice(n, size=weight, replace=False)] = rng.integers(1, 4, size=weight)
        rows.append(r)
    return np.stack(rows)


def xxz_terms(n: int, delta: float):
    """[(weight, string)] of the open XXZ chain -1/4 sum_q (XX + YY + delta ZZ)_{q,q+1}, bond by bond: XX, YY, ZZ of bond 0, then bond 1, ..."""
    terms = []
    for q in range(n - 1):
        for letter, w in ((1, -0.25), (2, -0.25), (3, -0.25 * delta)):
            r = np.zeros(n, dtype=np.uint8)
            r[q] = r[q + 1] = letter
            terms.append((w, r))
    return terms
