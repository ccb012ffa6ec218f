"""Plain NumPy reference of the truncated MPS arithmetic of the native engine: the engine's stated rule, walked gate by gate.

This is a test helper, not a conftest.  It restates the algorithm of ``aqc_mps_engine.cpp`` (``gate_adjacent``, ``gate2_pair``,
``apply_circuit``, ``fast_dot_gradient``) and of ``mps_engine.DeviceMPS.canonicalize`` in complex128 with LAPACK SVDs, so that the
single-lane engine and the lockstep lanes (``aqc_mps_lanes.hip``) can be checked against something other than each other.  It is
not an idealised optimal truncation: after a cut the form is only nearly canonical, and the values the next gate decides on
depend on the gauge, so the gauge of the engine is followed exactly:

* site q holds ``T_q[b][l][r] = Gamma_q[b] diag(lambda_q)`` (lambda on the right), ``|psi> = prod_q T_q``, plus the Schmidt
  vector of every bond and the accumulated discarded weight;
* a gate on (q, q + 1) forms ``theta[(a,l),(b,r)] = lambda_{q-1}[l] sum_m T_q[a][l][m] T_{q+1}[b][m][r]``, applies the 4 x 4
  matrix on the index ``2a + b``, splits by SVD and keeps ``k`` values (``decide``);
* ``T_q' = U S rescale / lambda_{q-1}``, ``T_{q+1}' = V^H``, ``lambda_q' = S rescale``.

Every truncation decision records a margin (``Decision``): how far its inputs are from flipping it.  Tests keep their cases at
margins where the rounding differences between the device's Jacobi SVD and LAPACK, or between the lanes' butterfly sums and a
sequential loop, cannot change a decision; any mismatch is then a fault.  Inner products are taken by transfer matrices, never
by densifying, so the walk also runs on registers beyond dense reach.  Aer's own truncation arithmetic is not what is restated
here; that stays unpinned.
"""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

FLOOR = 1e-14   # rank floor of the engine: values <= FLOOR * smax are numerically zero

_X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
_Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
_Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)
_P1 = np.diag([0, 1]).astype(np.complex128)
SWAP = np.eye(4, dtype=np.complex128)[[0, 2, 1, 3]]


def rz(t):
    return np.diag([np.exp(-0.5j * t), np.exp(0.5j * t)])


def ry(t):
    c, s = np.cos(0.5 * t), np.sin(0.5 * t)
    return np.array([[c, -s], [s, c]], dtype=np.complex128)


def rx(t):
    c, s = np.cos(0.5 * t), np.sin(0.5 * t)
    return np.array([[c, -1j * s], [-1j * s, c]], dtype=np.complex128)


def entangler(kind: str, angle: float = 0.0) -> np.ndarray:
    """|0><0| x I + |1><1| x {X, Z, diag(1, e^{i angle})}, index 2 ctrl + targ."""
    m = np.eye(4, dtype=np.complex128)
    m[2:, 2:] = {"cx": _X, "cz": _Z}.get(kind, np.diag([1.0, np.exp(1j * angle)]))
    return m


def permute(g4: np.ndarray) -> np.ndarray:
    """The same 2-qubit gate with the roles of its qubits swapped (index 2a + b -> 2b + a)."""
    p = [0, 2, 1, 3]
    return np.asarray(g4)[np.ix_(p, p)]


def svd(a: np.ndarray):
    """Thin SVD by LAPACK; the QR-iteration driver when divide and conquer gives up (as mps_operations._svd)."""
    try:
        return np.linalg.svd(a, full_matrices=False)
    except np.linalg.LinAlgError:
        import scipy.linalg

        return scipy.linalg.svd(a, full_matrices=False, lapack_driver="gesvd")


# ---- the rule ------------------------------------------------------------------------------------------------------------

@dataclass
class Decision:
    """One rank decision: ``k`` values kept of ``s`` (descending), their weights, and the margins of the three parts."""
    k: int
    total: float
    kept: float
    floor_margin: float            # min |s - FLOOR smax| / (FLOOR smax) over the values whose side of the floor decides k
    cap_margin: Optional[float]    # (s_{k-1} - s_k) / smax when max_bond made the cut, else None
    tail_margin: Optional[float]   # min |suffix weight - thr| / thr around the cut when thr > 0, else None

    @property
    def rescale(self) -> float:
        return float(np.sqrt(self.total / self.kept)) if self.kept > 0 else 1.0


def _final_rank(s: np.ndarray, k: int, thr: float, max_bond: int) -> Tuple[int, float]:
    """(rank, weight dropped by the tail) from ``k`` values above the floor: the cap, then the tail drop."""
    if max_bond > 0:
        k = min(k, max_bond)
    dropped = 0.0
    if thr > 0.0:
        while k > 1 and dropped + s[k - 1] ** 2 < thr:
            dropped += s[k - 1] ** 2
            k -= 1
    return k, dropped


def decide(s: np.ndarray, thr: float, max_bond: int) -> Decision:
    """Rank of a split by the engine's stated rule (aqc_mps_engine.cpp, gate_adjacent): values above ``FLOOR * smax``, then at
    most ``max_bond`` of them (> 0), then the tail dropped while ``k > 1`` and its accumulated weight stays strictly below the
    absolute threshold ``thr`` (> 0).  ``total`` covers every value, those under the floor and beyond the cap included.

    Margins: the floor's counts only the values whose side of the floor decides the final rank (a value of rounding size next
    to the floor is dropped by any tail threshold far above its weight, whichever side it lands on)."""
    s = np.asarray(s, dtype=np.float64)
    smax = float(s[0])
    if not (smax > 0.0 and np.isfinite(smax)):
        raise ValueError("zero or non-finite spectrum")
    total = 0.0
    k_floor = 0
    for j, v in enumerate(s):
        total += v * v
        if v > FLOOR * smax:
            k_floor = j + 1
    k, dropped = _final_rank(s, k_floor, thr, max_bond)
    floor_margin = np.inf
    for j, v in enumerate(s):   # value j on the other side of the floor
        if _final_rank(s, j if j < k_floor else j + 1, thr, max_bond)[0] != k:
            floor_margin = min(floor_margin, abs(v - FLOOR * smax) / (FLOOR * smax))
    cap_margin = float(s[max_bond - 1] - s[max_bond]) / smax if 0 < max_bond < k_floor else None
    tail_margin = None
    if thr > 0.0:
        tail_margin = (thr - dropped) / thr   # the weight that went
        if k > 1:                             # the value that stayed
            tail_margin = min(tail_margin, abs(dropped + s[k - 1] ** 2 - thr) / thr)
    kept = 0.0
    for j in range(k):
        kept += s[j] * s[j]
    return Decision(k, total, kept, floor_margin, cap_margin, tail_margin)


MIN_MARGIN = 1e-6        # tail drop (relative to thr) and cap (relative to smax)
MIN_FLOOR_MARGIN = 0.5   # rank floor, in units of the floor: a value near zero carries an absolute rounding of ~1e-16 smax


def smallest_margins(decisions: List[Decision]) -> dict:
    """The smallest margin of each kind met in ``decisions`` (inf where none was made)."""
    out = {"floor": np.inf, "cap": np.inf, "tail": np.inf}
    for d in decisions:
        for kind, m in (("floor", d.floor_margin), ("cap", d.cap_margin), ("tail", d.tail_margin)):
            if m is not None:
                out[kind] = min(out[kind], m)
    return out


def check_margins(decisions: List[Decision]) -> dict:
    """Asserts that no decision of ``decisions`` sits where rounding could flip it; returns ``smallest_margins``."""
    for d in decisions:
        assert d.floor_margin >= MIN_FLOOR_MARGIN, f"a singular value sits next to the rank floor: {d}"
        assert d.cap_margin is None or d.cap_margin >= MIN_MARGIN, f"max_bond cuts a (nearly) degenerate pair: {d}"
        assert d.tail_margin is None or d.tail_margin >= MIN_MARGIN, f"a suffix weight sits next to the threshold: {d}"
    return smallest_margins(decisions)


# ---- the state -----------------------------------------------------------------------------------------------------------

class RefMPS:
    """An MPS in the engine's gauge (see the module docstring), with the decisions of every truncated split it went through."""

    def __init__(self, sites: List[np.ndarray], lams: List[np.ndarray], discarded: float = 0.0):
        self.t = [np.array(x, dtype=np.complex128) for x in sites]
        self.lam = [np.array(v, dtype=np.float64).ravel() for v in lams]
        self.discarded = float(discarded)
        self.decisions: List[Decision] = []

    @classmethod
    def from_qiskit(cls, qiskit_mps, discarded: float = 0.0) -> "RefMPS":
        """``T_q = Gamma_q diag(lambda_q)`` as aqc_mps_create forms it; ``discarded`` as clone / set_targets carry it over."""
        gam, lam = qiskit_mps
        n = len(gam)
        sites = []
        for q in range(n):
            t = np.stack([np.asarray(gam[q][0], dtype=np.complex128), np.asarray(gam[q][1], dtype=np.complex128)])
            if q < n - 1:
                t = t * np.asarray(lam[q], dtype=np.float64).reshape(1, 1, -1)
            sites.append(t)
        return cls(sites, [np.asarray(v, dtype=np.float64).ravel() for v in lam], discarded)

    @classmethod
    def basis_state(cls, n: int, index: int = 0) -> "RefMPS":
        sites = [np.array([[[1.0 - ((index >> q) & 1)]], [[float((index >> q) & 1)]]], dtype=np.complex128) for q in range(n)]
        return cls(sites, [np.ones(1) for _ in range(n - 1)])

    def copy(self) -> "RefMPS":
        out = RefMPS(self.t, self.lam, self.discarded)
        out.decisions = list(self.decisions)
        return out

    @property
    def n(self) -> int:
        return len(self.t)

    @property
    def bond_dims(self) -> np.ndarray:
        return np.array([1] + [int(x.shape[2]) for x in self.t], dtype=np.int32)

    def to_qiskit(self):
        gam = []
        for q, x in enumerate(self.t):
            g = x / self.lam[q].reshape(1, 1, -1) if q < self.n - 1 else x
            gam.append((g[0].copy(), g[1].copy()))
        return gam, [v.copy() for v in self.lam]

    def to_vector(self) -> np.ndarray:
        """Dense state, index bit q <-> qubit q (small registers only)."""
        acc = self.t[0][:, 0, :]
        for x in self.t[1:]:
            acc = np.einsum("ia,bac->bic", acc, x).reshape(-1, x.shape[2])
        return acc.reshape(-1)

    # -- gates --
    def gate1(self, g: np.ndarray, q: int) -> "RefMPS":
        self.t[q] = np.einsum("ab,blr->alr", np.asarray(g, dtype=np.complex128), self.t[q])
        return self

    def gate_adjacent(self, q: int, g4: np.ndarray, thr: float = 0.0, max_bond: int = 0) -> Decision:
        """One 4 x 4 gate on (q, q + 1), index 2 bit_q + bit_{q+1} (aqc_mps_engine.cpp gate_adjacent, aqc_mps_dev.h theta / split)."""
        a, b = self.t[q], self.t[q + 1]
        chil, chir = a.shape[1], b.shape[2]
        lam_left = self.lam[q - 1] if q > 0 else np.ones(1)
        theta = np.einsum("alm,bmr->albr", a, b) * lam_left.reshape(1, -1, 1, 1)           # [a][l][b][r]
        theta = np.einsum("xy,ylr->xlr", np.asarray(g4, dtype=np.complex128), theta.transpose(0, 2, 1, 3).reshape(4, chil, chir))
        theta = theta.reshape(2, 2, chil, chir).transpose(0, 2, 1, 3).reshape(2 * chil, 2 * chir)
        u, s, vh = svd(theta)
        order = np.argsort(-s, kind="stable")
        u, s, vh = u[:, order], s[order], vh[order]
        d = decide(s, thr, max_bond)
        k, r = d.k, d.rescale
        self.discarded += d.total - d.kept
        left = (u[:, :k] * (s[:k] * r)).reshape(2, chil, k) / lam_left.reshape(1, -1, 1)
        self.t[q] = left
        self.t[q + 1] = vh[:k].reshape(k, 2, chir).transpose(1, 0, 2).copy()
        self.lam[q] = s[:k] * r
        self.decisions.append(d)
        return d

    def gate2(self, g4: np.ndarray, ctrl: int, targ: int, thr: float = 0.0, max_bond: int = 0) -> "RefMPS":
        """4 x 4 gate (index 2 bit_ctrl + bit_targ) on any pair: swaps down from ``hi``, the gate, swaps back -- every swap
        truncated as well (aqc_mps_engine.cpp gate2_pair)."""
        lo, hi = min(ctrl, targ), max(ctrl, targ)
        for p in range(hi - 1, lo, -1):
            self.gate_adjacent(p, SWAP, thr, max_bond)
        self.gate_adjacent(lo, permute(g4) if ctrl > targ else g4, thr, max_bond)
        for p in range(lo + 1, hi):
            self.gate_adjacent(p, SWAP, thr, max_bond)
        return self

    def canonicalize(self) -> "RefMPS":
        """Identity "gates" right to left, then left to right, exact (mps_engine.DeviceMPS.canonicalize)."""
        eye4 = np.eye(4, dtype=np.complex128)
        for q in range(self.n - 2, -1, -1):
            self.gate_adjacent(q, eye4, 0.0, 0)
        for q in range(self.n - 1):
            self.gate_adjacent(q, eye4, 0.0, 0)
        return self


def dot(a: RefMPS, b: RefMPS, ops_a=()) -> complex:
    """<(prod_i G_i on qubit_i) a | b> by transfer matrices; ``ops_a = [(qubit, 2x2), ...]`` act on a's side."""
    ops = dict(ops_a)
    e = np.ones((1, 1), dtype=np.complex128)
    for q in range(a.n):
        x = a.t[q]
        if q in ops:
            x = np.einsum("ab,blr->alr", np.asarray(ops[q], dtype=np.complex128), x)
        e = np.einsum("xy,bxu,byv->uv", e, np.conj(x), b.t[q])
    return complex(e[0, 0])


# ---- the ansatz ----------------------------------------------------------------------------------------------------------

def _blocks(a):
    """(running index i, parameter block j, ctrl, targ), incl. the tail half-layer of a 2nd-order Trotter ansatz."""
    L = a.num_blocks
    tail = 3 * (a.n // 2) if (a.trotter and a.second_order) else 0
    return [(i, i % L, int(a.blocks[0, i % L]), int(a.blocks[1, i % L])) for i in range(L + tail)] if L else []


def _as_ansatz(circ):
    from oracle import aqc_oracle as orc

    return orc.as_ansatz(circ)


def apply_circuit(circ, thetas, m: RefMPS, inverse: bool = False, thr: float = 0.0, max_bond: int = 0) -> RefMPS:
    """V(thetas)|m> or V^H|m> in place, the gate order of aqc_mps_engine.cpp apply_circuit (Trotter rz(-+pi/2) included)."""
    a = _as_ansatz(circ)
    n, tpb = a.n, a.tpb
    th = np.asarray(thetas, dtype=np.float64)
    t2 = th[3 * n:]
    rs = rx if a.entangler == "cx" else rz
    hp = np.pi / 2
    blocks = _blocks(a)
    if not inverse:
        for q in range(n):
            m.gate1(rz(th[3 * q]) @ ry(th[3 * q + 1]) @ rz(th[3 * q + 2]), q)
        for i, j, c, t in blocks:
            p = t2[tpb * j: tpb * j + tpb]
            if a.trotter and i % 3 == 0:
                m.gate1(rz(-hp), c)
            m.gate2(entangler(a.entangler, p[4] if tpb == 5 else 0.0), c, t, thr, max_bond)
            m.gate1(rz(p[1]) @ ry(p[0]), c)
            m.gate1(rs(p[3]) @ ry(p[2]), t)
            if a.trotter and i % 3 == 2:
                m.gate1(rz(hp), t)
    else:
        for i, j, c, t in reversed(blocks):
            p = t2[tpb * j: tpb * j + tpb]
            if a.trotter and i % 3 == 2:
                m.gate1(rz(-hp), t)
            m.gate1(ry(-p[2]) @ rs(-p[3]), t)
            m.gate1(ry(-p[0]) @ rz(-p[1]), c)
            m.gate2(entangler(a.entangler, -p[4] if tpb == 5 else 0.0), c, t, thr, max_bond)
            if a.trotter and i % 3 == 0:
                m.gate1(rz(hp), c)
        for q in range(n):
            m.gate1(rz(-th[3 * q + 2]) @ ry(-th[3 * q + 1]) @ rz(-th[3 * q]), q)
    return m


def fast_dot_gradient(circ, thetas, lvec: RefMPS, vh_phi: RefMPS, thr: float = 0.0, max_bond: int = 0,
                      block_range: Optional[Tuple[int, int]] = None, front_layer: bool = True):
    """(complex gradient of <V lvec|phi> given vh_phi = V^H|phi>, w, z): the walk of aqc_mps_engine.cpp fast_dot_gradient on
    copies w <- lvec, z <- vh_phi -- front layer rz, ry, rz right to left with 0.5j <P w|z>; per block the cp record
    -1j <P11 P11 w|z> before the gate, the gate on z then w (truncated), then the four 1-qubit records.  The final (w, z)
    come back with their decisions."""
    a = _as_ansatz(circ)
    n, tpb = a.n, a.tpb
    th = np.asarray(thetas, dtype=np.float64)
    lo, hi = (0, a.num_blocks) if block_range is None else (int(block_range[0]), int(block_range[1]))
    grad = np.zeros(a.num_thetas, dtype=np.complex128)
    w, z = lvec.copy(), vh_phi.copy()
    w.decisions, z.decisions = [], []
    cx = a.entangler == "cx"
    hp = np.pi / 2

    def both(g, q):
        w.gate1(g, q)
        z.gate1(g, q)

    for q in range(n):
        for slot in (2, 1, 0):
            is_y = slot == 1
            both((ry if is_y else rz)(th[3 * q + slot]), q)
            if front_layer:
                grad[3 * q + slot] += 0.5j * dot(w, z, [(q, _Y if is_y else _Z)])
    for i, j, c, t in _blocks(a):
        p = th[3 * n + tpb * j: 3 * n + tpb * j + tpb]
        base = 3 * n + tpb * j
        live = lo <= j < hi
        if a.trotter and i % 3 == 0:
            both(rz(-hp), c)
        if live and tpb == 5:
            grad[base + 4] += -1j * dot(w, z, [(c, _P1), (t, _P1)])
        ent = entangler(a.entangler, p[4] if tpb == 5 else 0.0)
        z.gate2(ent, c, t, thr, max_bond)
        w.gate2(ent, c, t, thr, max_bond)
        for k, (q, g, pauli) in enumerate(((c, ry(p[0]), _Y), (c, rz(p[1]), _Z), (t, ry(p[2]), _Y),
                                           (t, rx(p[3]) if cx else rz(p[3]), _X if cx else _Z))):
            both(g, q)
            if live:
                grad[base + k] += 0.5j * dot(w, z, [(q, pauli)])
        if a.trotter and i % 3 == 2:
            both(rz(hp), t)
    return grad, w, z
