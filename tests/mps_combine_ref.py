"""The NumPy statement of linear combinations of MPS states: what aqc_research_amd/mps_engine.py (linear_combinations) and
csrc/aqc_mps_combine.hip are tested against.  tests/test_mps_combine_ref.py holds it to sum_k c_k dense(psi_k).

State and notation of tests/mps_ent_ref.py: psi(b) = T_0[b_0] ... T_{n-1}[b_{n-1}], T_q of shape (2, chi_q, chi_{q+1}), any gauge.  The rule of
csrc/aqc_mps_combine_rule.h, for terms psi_k with sites T^k_q and coefficients c_k:

    sum     the direct sum S with bonds Sigma_q = sum_k chi^k_q (0 < q < n), Sigma_0 = Sigma_n = 1:
            S_0[s] = [c_0 T^0_0[s] | c_1 T^1_0[s] | ...],  S_q[s] = diag(T^0_q[s], ..., T^{K-1}_q[s]),  S_{n-1}[s] the column stack;
            n = 1: S_0[s] = sum_k c_k T^k_0[s]
    result  ``mps_compress_ref.compress`` of S; its discarded weight is what these cuts dropped, the terms' own weights are not carried
    scale   sum_k |c_k| |psi_k|: what errors are relative to (an exact cancellation is not detected)

``CASES`` are the sums that the CPU and the GPU tests share."""
import functools

import numpy as np

from tests import mps_compress_ref, mps_obs_ref


def direct_sum(states, coeffs):
    """The direct sum as a QiskitMPS tuple with unit bond vectors."""
    ts = [mps_obs_ref.site_tensors(s) for s in states]
    c = np.asarray(coeffs, dtype=np.complex128).ravel()
    n = len(ts[0])
    if len(ts) != c.size or not ts or any(len(t) != n for t in ts):
        raise ValueError("one coefficient per state, one qubit count")
    if n == 1:
        total = sum(ck * t[0] for ck, t in zip(c, ts))
        return [(total[0], total[1])], []
    gam = []
    for q in range(n):
        rows = [t[q].shape[1] for t in ts] if q > 0 else None
        cols = [t[q].shape[2] for t in ts] if q < n - 1 else None
        site = np.zeros((2, sum(rows) if rows else 1, sum(cols) if cols else 1), dtype=np.complex128)
        r0 = c0 = 0
        for k, t in enumerate(ts):
            block = c[k] * t[q] if q == 0 else t[q]
            site[:, r0:r0 + block.shape[1], c0:c0 + block.shape[2]] = block
            r0 += block.shape[1] if rows else 0
            c0 += block.shape[2] if cols else 0
        gam.append((site[0], site[1]))
    return gam, [np.ones(g[0].shape[1]) for g in gam[:-1]]


def combine(states, coeffs, thr: float = 0.0, max_bond: int = 0):
    """``mps_compress_ref.compress`` of the direct sum (a ``mps_trunc_ref.RefMPS`` with the decisions of its cuts)."""
    return mps_compress_ref.compress(direct_sum(states, coeffs), thr, max_bond)


def dense_sum(states, coeffs):
    """(sum_k c_k dense(psi_k), scale)."""
    vecs = [mps_obs_ref.dense(s) for s in states]
    c = np.asarray(coeffs, dtype=np.complex128).ravel()
    return sum(ck * v for ck, v in zip(c, vecs)), float(sum(abs(ck) * np.linalg.norm(v) for ck, v in zip(c, vecs)))


def _basis(n, index):
    gam = [(np.array([[1.0 - ((index >> q) & 1)]], dtype=np.complex128), np.array([[float((index >> q) & 1)]], dtype=np.complex128)) for q in range(n)]
    return gam, [np.ones(1) for _ in range(n - 1)]


P5, P7, P16 = [1, 2, 3, 5, 3, 2, 1], [1, 2, 4, 7, 4, 2, 1], [1, 2, 4, 8, 16, 8, 4, 2, 1]


@functools.lru_cache(maxsize=None)
def case(name):
    """(states, coefficients, the bonds the exact result must have).  A state listed twice is the same tuple object."""
    hm = mps_obs_ref.hand_made
    if name == "three":
        return [hm(P5, 701), hm(P7, 702), hm([1] * 7, 703)], [0.7 - 0.2j, -1.1j, 0.4], [1, 2, 4, 8, 4, 2, 1]
    if name in ("twice", "half", "nearly"):
        psi = hm(P5, 704)
        return [psi, psi], [1.0, {"twice": 1.0, "half": -0.5, "nearly": -0.999}[name]], P5
    if name == "n2":
        return [hm([1, 2, 1], 705), hm([1, 1, 1], 706), hm([1, 2, 1], 707)], [0.3 + 0.4j, -0.8, 1.2j], [1, 2, 1]
    if name == "n3":
        return [hm([1, 2, 2, 1], 708), hm([1, 1, 2, 1], 709)], [1.0, -0.6 + 0.3j], [1, 2, 2, 1]
    if name == "n1":
        return [hm([1, 1], 710), hm([1, 1], 711), hm([1, 1], 712)], [0.5, -0.25j, 1.5 + 0.5j], [1, 1]
    if name == "cap64":
        return [hm(P16, 713 + k) for k in range(4)], [0.6, -0.7j, 0.5 + 0.5j, -0.9], P16
    if name == "w8":
        return [_basis(8, 1 << q) for q in range(8)], [1.0 / np.sqrt(8.0)] * 8, [1, 2, 2, 2, 2, 2, 2, 2, 1]
    raise KeyError(name)


CASES = ("three", "twice", "half", "nearly", "n2", "n3", "n1", "cap64", "w8")
TRUNCATED = ("three", "cap64", "n3")   # the cases that are also cut: thresholds and caps by mps_compress_ref.pick on the direct sum


@functools.lru_cache(maxsize=None)
def truncation(name, as_cap):
    """(threshold, max_bond, the statement's result, smallest relative gap or None), chosen once on the direct-sum tuple."""
    states, coeffs, _ = case(name)
    total = direct_sum(states, coeffs)
    scale2 = dense_sum(states, coeffs)[1] ** 2
    cands = mps_compress_ref.CAPS if as_cap else tuple(t * scale2 for t in mps_compress_ref.THRESHOLDS)
    value, ref = mps_compress_ref.pick(total, cands, as_cap)
    thr, cap = (0.0, value) if as_cap else (value, 0)
    gaps = mps_compress_ref.gaps(ref.decisions, mps_compress_ref.spectra(total, thr, cap))
    return thr, cap, ref, (min(gaps) if gaps else None)
