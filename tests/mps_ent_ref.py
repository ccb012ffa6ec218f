"""The NumPy statement of the Schmidt spectra of an MPS: what aqc_research_amd/mps_observables.py (schmidt_values) and
csrc/aqc_mps_ent.hip are tested against beyond dense reach.  tests/test_mps_ent_ref.py holds it to SVDs of the dense vector.

State and notation of tests/mps_obs_ref.py: psi(b) = T_0[b_0] ... T_{n-1}[b_{n-1}], T_q of shape (2, chi_q, chi_{q+1}), any gauge.

    left    C_0 = [1], C_{q+1} = the R factor (chi_{q+1} x chi_{q+1}, zero rows beyond min(2 chi_q, chi_{q+1})) of [C_q T_q[0]; C_q T_q[1]]
    right   D_n = [1], D_q = the R factor of [D_{q+1} T_q[0]^T; D_{q+1} T_q[1]^T]
    cut q   the singular values of C_q D_q^T, descending, q = 1 .. n - 1 (qubits 0 .. q-1 | q .. n-1); nothing is normalised

The R factor is taken by unpivoted Householder reflections (``householder_r``, the rule of csrc/aqc_mps_ent_rule.h); any R with
R^H R = M^H M gives the same singular values.  ``schmidt_by_squares`` is the method that is NOT used: eigenvalues of L_q R_q."""
import numpy as np

from tests import mps_obs_ref


def householder_r(m: np.ndarray) -> np.ndarray:
    """The cols x cols R factor of ``m`` (rows x cols): column j takes its reflection from rows j .., a column that is zero
    there (or below 1e-150, where its reflection cannot be formed: ``mps_ent_reflects`` of the rule) is skipped, the last row needs
    none; rows beyond min(rows, cols) are zero."""
    a = np.array(m, dtype=np.complex128)
    rows, cols = a.shape
    for j in range(min(rows - 1, cols)):
        x = a[j:, j].copy()
        norm2 = float(np.sum(x.real ** 2 + x.imag ** 2))
        if norm2 < 1e-300:   # zero, or so small (|x| < 1e-150: deeply rank-deficient sums) that the reflection's 1 / |x|^2 overflows
            continue
        nrm, ax = np.sqrt(norm2), abs(x[0])
        phase = x[0] / ax if ax > 0.0 else 1.0
        v = x
        v[0] = x[0] + phase * nrm
        tau = 1.0 / (nrm * (nrm + ax))
        a[j:, j + 1:] -= np.outer(v, tau * (v.conj() @ a[j:, j + 1:]))
        a[j, j] = -phase * nrm
        a[j + 1:, j] = 0.0
    r = np.zeros((cols, cols), dtype=np.complex128)
    k = min(rows, cols)
    r[:k] = np.triu(a[:k])
    return r


def factors(ts):
    """``(C, D)``: lists of n + 1 matrices, C[q] and D[q] of bond q (chi_q x chi_q); C[0] = D[n] = [1]; C[n] and D[0] are 1 x 1."""
    n = len(ts)
    c = [np.ones((1, 1), dtype=np.complex128)]
    for t in ts:
        c.append(householder_r(np.concatenate([c[-1] @ t[0], c[-1] @ t[1]])))
    d = [np.ones((1, 1), dtype=np.complex128)]
    for t in reversed(ts):
        d.append(householder_r(np.concatenate([d[-1] @ t[0].T, d[-1] @ t[1].T])))
    d = d[::-1]
    assert len(c) == len(d) == n + 1
    return c, d


def schmidt(qiskit_mps) -> np.ndarray:
    """(n - 1, K) float64, K the largest inner bond dimension (1 for n = 1): row q - 1 holds the chi_q values of cut q, descending,
    then zeros."""
    ts = mps_obs_ref.site_tensors(qiskit_mps)
    n = len(ts)
    c, d = factors(ts)
    k = max([1] + [ts[q].shape[1] for q in range(1, n)])
    out = np.zeros((n - 1, k), dtype=np.float64)
    for q in range(1, n):
        s = np.linalg.svd(c[q] @ d[q].T, compute_uv=False)
        out[q - 1, :s.size] = s
    return out


def schmidt_by_squares(qiskit_mps) -> np.ndarray:
    """The same from the eigenvalues of L_q R_q of the environments (the squared method): loses what lies below ~1e-8 s_max."""
    ts = mps_obs_ref.site_tensors(qiskit_mps)
    n = len(ts)
    left, right = mps_obs_ref.left_environments(ts), mps_obs_ref.right_environments(ts)
    k = max([1] + [ts[q].shape[1] for q in range(1, n)])
    out = np.zeros((n - 1, k), dtype=np.float64)
    for q in range(1, n):
        ev = np.linalg.eigvals(left[q] @ right[q])   # L_q = M_l^H M_l, R_q = M_r M_r^H with psi = M_l M_r: the squares of the values
        out[q - 1, :ev.size] = np.sort(np.sqrt(np.abs(ev.real)))[::-1]
    return out


def schmidt_dense(psi: np.ndarray, dims) -> np.ndarray:
    """The same from SVDs of the dense vector (index bit q is qubit q), zero-padded or cut to the bond dimensions ``dims`` (n + 1)."""
    n = len(dims) - 1
    k = max([1] + [int(dims[q]) for q in range(1, n)])
    out = np.zeros((n - 1, k), dtype=np.float64)
    for q in range(1, n):
        s = np.linalg.svd(np.asarray(psi).reshape(2 ** (n - q), 2 ** q), compute_uv=False)
        m = min(s.size, int(dims[q]))
        out[q - 1, :m] = s[:m]
    return out


def pad_case():
    """dims [1, 2, 4, 8, 8, 8, 4, 2, 1], seed 5, columns 4 .. of site 3 zeroed: the cut after site 3 has rank 4 at bond 8."""
    gam, lam = mps_obs_ref.hand_made([1, 2, 4, 8, 8, 8, 4, 2, 1], 5)
    g0, g1 = gam[3]
    g0, g1 = g0.copy(), g1.copy()
    g0[:, 4:] = 0.0
    g1[:, 4:] = 0.0
    gam = list(gam)
    gam[3] = (g0, g1)
    return gam, lam


def nested_pairs(angles):
    """An exact MPS of n = 2 len(angles) qubits: the pairs (k, n - 1 - k) in cos a_k |00> + sin a_k |11>.  The middle cut's values are
    the products of one of (cos a_k, sin a_k) per pair.  Returns ``(QiskitMPS tuple, the middle cut's 2^len(angles) values descending)``."""
    m = len(angles)
    n = 2 * m
    gam = []
    for q in range(n):
        k = q if q < m else n - 1 - q                         # the pair this qubit belongs to
        chi_l, chi_r = 2 ** min(q, n - q), 2 ** min(q + 1, n - q - 1)
        t = np.zeros((2, chi_l, chi_r), dtype=np.complex128)
        if q < m:      # opens pair k: the bond index gains bit k (the lowest bits are the outer pairs) = the value of this qubit
            for x in range(chi_l):
                for b in range(2):
                    t[b, x, x | (b << k)] = np.cos(angles[k]) if b == 0 else np.sin(angles[k])
        else:          # closes pair k: the qubit's value must equal bit k of the bond index, which is removed (the highest one)
            for u in range(chi_r):
                for b in range(2):
                    t[b, u | (b << k), u] = 1.0
        gam.append((t[0], t[1]))
    lam = [np.ones(gam[q][0].shape[1]) for q in range(n - 1)]
    vals = np.ones(1)
    for a in angles:
        vals = np.outer(vals, [np.cos(a), np.sin(a)]).ravel()
    return (gam, lam), np.sort(vals)[::-1]
