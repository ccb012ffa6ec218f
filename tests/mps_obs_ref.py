"""The NumPy statement of the pair density matrices of an MPS: what aqc_research_amd/mps_observables.py and csrc/aqc_mps_obs.hip are
tested against beyond dense reach.  Written site by site with matrix products, without the kernel's chains, components or mirroring;
tests/test_mps_obs_ref.py holds it to tests/obs_ref.rdm of the dense state.

State: psi(b) = T_0[b_0] T_1[b_1] ... T_{n-1}[b_{n-1}] with site tensors T_q of shape (2, chi_q, chi_{q+1}) in any gauge.
Convention of obs_ref: for the pair (i, j) the row index is value(i) + 2 value(j), rho[a][b] = sum_rest psi(rest, a) conj psi(rest, b);
no normalisation."""
import numpy as np


def site_tensors(qiskit_mps):
    """T_q = Gamma_q lambda_q (the last site has no Schmidt vector): the tensors the engine keeps."""
    gam, lam = qiskit_mps
    n = len(gam)
    out = []
    for q in range(n):
        t = np.stack([np.asarray(gam[q][0], dtype=np.complex128), np.asarray(gam[q][1], dtype=np.complex128)])
        if q < n - 1:
            t = t * np.asarray(lam[q], dtype=np.float64).ravel()[None, None, :]
        out.append(t)
    return out


def hand_made(dims, seed, norm=1.0):
    """A QiskitMPS tuple with N(0, 1) tensors of the bond dimensions ``dims`` (n + 1 of them) and unit Schmidt vectors, scaled so that
    the dense vector has norm ``norm``."""
    rng = np.random.default_rng(seed)
    n = len(dims) - 1
    ts = [rng.standard_normal((2, dims[q], dims[q + 1])) + 1j * rng.standard_normal((2, dims[q], dims[q + 1])) for q in range(n)]
    # scale site by site so that no partial product over- or underflows
    left = np.ones((1, 1), dtype=np.complex128)
    for q in range(n):
        left = np.einsum("cxu,xy,cyv->uv", ts[q].conj(), left, ts[q], optimize=True)
        s = np.sqrt(np.trace(left).real)
        ts[q] = ts[q] / s
        left = left / (s * s)
    ts[0] = ts[0] * (norm / np.sqrt(np.trace(left).real))
    gam = [(t[0].copy(), t[1].copy()) for t in ts]
    lam = [np.ones(dims[q + 1]) for q in range(n - 1)]
    return gam, lam


def left_environments(ts):
    envs = [np.ones((1, 1), dtype=np.complex128)]
    for t in ts:
        envs.append(np.einsum("cxu,xy,cyv->uv", t.conj(), envs[-1], t, optimize=True))
    return envs   # envs[q] = L_q, q = 0 .. n


def right_environments(ts):
    envs = [np.ones((1, 1), dtype=np.complex128)]
    for t in reversed(ts):
        envs.append(np.einsum("cxu,uv,cyv->xy", t, envs[-1], t.conj(), optimize=True))
    return envs[::-1]   # envs[q] = R_q, q = 0 .. n


def norm2(qiskit_mps) -> float:
    """<psi|psi>."""
    return float(left_environments(site_tensors(qiskit_mps))[-1][0, 0].real)


def pair_rdms(qiskit_mps, pairs) -> np.ndarray:
    """(P, 4, 4) complex128 for the listed pairs, either order of the two qubits."""
    ts = site_tensors(qiskit_mps)
    left, right = left_environments(ts), right_environments(ts)
    out = np.empty((len(pairs), 4, 4), dtype=np.complex128)
    for p, (qa, qb) in enumerate(pairs):
        i, j = min(qa, qb), max(qa, qb)
        th = ts[i].conj().transpose(0, 2, 1)
        e = th[None, :] @ (left[i] @ ts[i])[:, None]                         # [a][b] = T_i[b]^H (L_i T_i[a])
        for q in range(i + 1, j):
            e = sum(t.conj().T @ e @ t for t in ts[q])                       # every [a][b] block: sum_c T_q[c]^H E T_q[c]
        k = (ts[j] @ right[j + 1])[:, None] @ ts[j].conj().transpose(0, 2, 1)[None, :]   # [c][d] = T_j[c] R_{j+1} T_j[d]^H
        rho = np.einsum("abxy,cdyx->acbd", e, k)          # [a][c][b][d]
        if qa > qb:                                        # listed as (j, i): the first listed qubit is the low index bit
            rho = rho.transpose(1, 0, 3, 2)
        out[p] = rho.transpose(1, 0, 3, 2).reshape(4, 4)   # row = first + 2 second
    return out


def dense(qiskit_mps) -> np.ndarray:
    """The dense vector in NumPy (index bit q is qubit q), for tests that run without a device."""
    ts = site_tensors(qiskit_mps)
    v = np.ones((1, 1), dtype=np.complex128)                 # [index of the qubits so far][bond]
    for q, t in enumerate(ts):
        v = np.einsum("ix,cxu->ciu", v, t).reshape(2 ** (q + 1), t.shape[2])   # the new qubit is the highest bit so far
    return v[:, 0]


# bond profiles of the tests (the n + 1 bond dimensions)
PROFILE_A = [1, 2, 3, 5, 7, 13, 17, 33, 64, 37, 16, 5, 2, 1]     # non-multiples of 4 and 16, rectangular sites, the fused cap itself
PROFILE_C = [1, 2, 1, 3, 1]                                       # a bond of 1 inside
PROFILE_D = [1, 2, 4, 8, 16, 32, 65, 96, 40, 16, 8, 4, 2, 1]      # beyond the fused cap


def profile_b(n):
    return [1] * (n + 1)                                          # product states
