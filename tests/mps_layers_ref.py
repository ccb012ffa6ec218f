"""The NumPy statement of gate layers on MPS states: what aqc_research_amd/mps_engine.py (apply_gates, v_mul_mps_many) and
csrc/aqc_mps_layers.hip are tested against.  tests/test_mps_layers_ref.py holds it to the program applied in its own order on the
dense vector.

A program is a list of ``(matrix, qubit)`` (2 x 2) and ``(matrix, (a, b))`` (4 x 4 on the index 2 bit_a + bit_b), applied in order.
The rule of csrc/aqc_mps_layers_rule.h, restated:

    routing   a pair that is not adjacent: swaps down from the upper qubit, the gate on (lo, lo + 1) (with its qubits' roles swapped
              when a is the upper one), swaps back -- ``mps_trunc_ref.RefMPS.gate2``
    folding   every 1-qubit op goes into the next 2-qubit op on its qubit; where there is none, into the last earlier one, from the
              left; a qubit that no 2-qubit op touches keeps the product of its 1-qubit ops
    layering  as soon as possible: a gate on (q, q + 1) goes into layer max(ready[q], ready[q + 1]), both become that + 1

``apply`` runs ``mps_trunc_ref.RefMPS.gate_adjacent`` per folded gate in layer order on a ``RefMPS`` (imported, not edited) and keeps the
decisions, with the spectrum each one was taken on (``spectra``), for the margins and gaps of the tests."""
import numpy as np

from tests import mps_trunc_ref
from tests.mps_trunc_ref import SWAP, RefMPS, permute

EYE2 = np.eye(2, dtype=np.complex128)


def is_pair(where) -> bool:
    return not np.isscalar(where) and np.ndim(where) == 1


def route(gates):
    """The program on adjacent sites: ``[(two, q, matrix)]``, a 2-qubit matrix on the index 2 bit_q + bit_{q+1}."""
    out = []
    for g, where in gates:
        g = np.asarray(g, dtype=np.complex128)
        if not is_pair(where):
            out.append((False, int(where), g))
            continue
        a, b = int(where[0]), int(where[1])
        lo, hi = min(a, b), max(a, b)
        for p in range(hi - 1, lo, -1):
            out.append((True, p, SWAP))
        out.append((True, lo, permute(g) if a > b else g))
        for p in range(lo + 1, hi):
            out.append((True, p, SWAP))
    return out


def fold(n: int, routed):
    """``(folded, singles)``: ``folded = [(q, layer, 4 x 4)]`` in program order, ``singles = {qubit: 2 x 2}`` of the untouched qubits."""
    pending = [EYE2.copy() for _ in range(n)]
    has_op = [False] * n
    last = [-1] * n
    ready = [0] * n
    folded = []
    for two, q, g in routed:
        if not two:
            pending[q] = g @ pending[q]
            has_op[q] = True
            continue
        layer = max(ready[q], ready[q + 1])
        ready[q] = ready[q + 1] = layer + 1
        folded.append([q, layer, g @ np.kron(pending[q], pending[q + 1])])
        pending[q], pending[q + 1] = EYE2.copy(), EYE2.copy()
        last[q] = last[q + 1] = len(folded) - 1
    singles = {}
    for q in range(n):
        if last[q] < 0:
            if has_op[q]:
                singles[q] = pending[q]
            continue
        item = folded[last[q]]
        item[2] = (np.kron(pending[q], EYE2) if item[0] == q else np.kron(EYE2, pending[q])) @ item[2]
    return [tuple(x) for x in folded], singles


def layers(folded):
    """The indices of the folded gates, layer by layer."""
    count = 1 + max([layer for _, layer, _ in folded], default=-1)
    return [[i for i, (_, layer, _) in enumerate(folded) if layer == l] for l in range(count)]


def theta_spectrum(m: RefMPS, q: int, g4) -> np.ndarray:
    """The descending spectrum ``RefMPS.gate_adjacent(q, g4)`` decides on."""
    a, b = m.t[q], m.t[q + 1]
    chil, chir = a.shape[1], b.shape[2]
    lam_left = m.lam[q - 1] if q > 0 else np.ones(1)
    theta = np.einsum("alm,bmr->albr", a, b) * lam_left.reshape(1, -1, 1, 1)
    theta = np.einsum("xy,ylr->xlr", np.asarray(g4, dtype=np.complex128), theta.transpose(0, 2, 1, 3).reshape(4, chil, chir))
    theta = theta.reshape(2, 2, chil, chir).transpose(0, 2, 1, 3).reshape(2 * chil, 2 * chir)
    return np.sort(mps_trunc_ref.svd(theta)[1])[::-1]


def apply(state, gates, thr: float = 0.0, max_bond: int = 0, with_spectra: bool = False) -> RefMPS:
    """The statement: a copy of ``state`` (a RefMPS or a QiskitMPS tuple) after the folded gates in layer order and the singles.
    ``decisions`` are those of this call, in the order taken; ``spectra`` (when asked for) what each was taken on."""
    m = state.copy() if isinstance(state, RefMPS) else RefMPS.from_qiskit(state)
    m.decisions, m.spectra = [], []
    folded, singles = fold(m.n, route(gates))
    for layer in layers(folded):
        for i in layer:
            q, _, g = folded[i]
            if with_spectra:
                m.spectra.append(theta_spectrum(m, q, g))
            m.gate_adjacent(q, g, thr, max_bond)
    for q, u in singles.items():
        m.gate1(u, q)
    return m


def in_order(state, gates, thr: float = 0.0, max_bond: int = 0) -> RefMPS:
    """What the call replaces: ``gate1`` / ``gate2`` per op in the program's own order, on the same reference class."""
    m = state.copy() if isinstance(state, RefMPS) else RefMPS.from_qiskit(state)
    m.decisions = []
    for g, where in gates:
        if is_pair(where):
            m.gate2(np.asarray(g, dtype=np.complex128), int(where[0]), int(where[1]), thr, max_bond)
        else:
            m.gate1(np.asarray(g, dtype=np.complex128), int(where))
    return m


# ---- dense vectors: index bit q <-> qubit q, as RefMPS.to_vector

def dense_gate1(psi, n, g, q):
    t = np.asarray(psi, dtype=np.complex128).reshape([2] * n)
    t = np.moveaxis(np.tensordot(np.asarray(g, dtype=np.complex128), t, axes=([1], [n - 1 - q])), 0, n - 1 - q)
    return t.reshape(-1)


def dense_gate2(psi, n, g4, a, b):
    t = np.asarray(psi, dtype=np.complex128).reshape([2] * n)
    g = np.asarray(g4, dtype=np.complex128).reshape(2, 2, 2, 2)   # [a'][b'][a][b]
    t = np.tensordot(g, t, axes=([2, 3], [n - 1 - a, n - 1 - b]))
    return np.moveaxis(t, [0, 1], [n - 1 - a, n - 1 - b]).reshape(-1)


def dense_program(psi, n, gates):
    """The program in its own order on the dense vector."""
    for g, where in gates:
        psi = dense_gate2(psi, n, g, int(where[0]), int(where[1])) if is_pair(where) else dense_gate1(psi, n, g, int(where))
    return psi


def dense_layered(psi, n, gates):
    """The routed, folded program in layer order on the dense vector, then the singles."""
    folded, singles = fold(n, route(gates))
    for layer in layers(folded):
        for i in layer:
            q, _, g = folded[i]
            psi = dense_gate2(psi, n, g, q, q + 1)
    for q, u in singles.items():
        psi = dense_gate1(psi, n, u, q)
    return psi


# ---- an ansatz as a program

def circuit_gates(circ, thetas, inverse: bool = False):
    """V(thetas) (or its conjugate transpose) as a list of gates, in the order of ``mps_trunc_ref.apply_circuit``."""
    ops = []

    class Recorder:
        def gate1(self, g, q):
            ops.append((np.asarray(g, dtype=np.complex128), int(q)))

        def gate2(self, g, c, t, thr=0.0, max_bond=0):
            ops.append((np.asarray(g, dtype=np.complex128), (int(c), int(t))))

    mps_trunc_ref.apply_circuit(circ, thetas, Recorder(), inverse)
    return ops


# ---- the truncated cases of the tests: chosen on the reference, never changed

MIN_GAP = 1e-3    # tests/test_mps_compress_ref.py


def gaps(decisions, spectra):
    """Per decision that dropped values above the rank floor: (s_{k-1} - s_k) / s_max, the relative gap next to the cut."""
    out = []
    for dec, s in zip(decisions, spectra):
        above = int(np.count_nonzero(s > mps_trunc_ref.FLOOR * s[0]))
        if dec.k < above:
            out.append(float(s[dec.k - 1] - s[dec.k]) / float(s[0]))
    return out


def pick(state, gates, candidates, as_cap: bool):
    """The first of ``candidates`` (thresholds, or max_bond values when ``as_cap``) at which every decision of ``apply`` is clear of
    rounding (``mps_trunc_ref.check_margins``), has a relative gap >= MIN_GAP next to it where it drops values, and at least one
    decision drops values.  ``(value, statement, smallest gap)``, or None when no candidate passes (the case is dropped then)."""
    for cand in candidates:
        ref = apply(state, gates, 0.0, cand, True) if as_cap else apply(state, gates, cand, 0, True)
        try:
            mps_trunc_ref.check_margins(ref.decisions)
        except AssertionError:
            continue
        found = gaps(ref.decisions, ref.spectra)
        if found and min(found) >= MIN_GAP:
            return cand, ref, min(found)
    return None
