"""
Device-resident matrix-product states with truncated 2-qubit gates (C ABI ``aqc_mps_*``): the part of the
reference that runs inside qiskit-aer's ``matrix_product_state`` simulator (``mps_operations.py:216-298``,
``mps_dot_objective.py:41-468``), for registers too large for a dense state.

``DeviceMPS`` wraps one state; ``fast_dot_gradient_mps`` is the gate-by-gate gradient sweep of
``mps_dot_objective.fast_dot_gradient`` (:41-242) on two such states, ``v_mul_mps`` / ``v_dagger_mul_mps`` the
circuit applications of ``mps_operations.py:326-371``.  With ``trunc_thr -> 0`` everything is exact (tested
against the dense oracle); Aer's truncation arithmetic itself is third party and parity unpinned.
"""
import ctypes
from ctypes import POINTER, byref, c_int, c_int32, c_void_p
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np

from . import _lib, gates
from ._lib import LanesRefused, check, dptr, iptr

_X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
_Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
_Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)
_P1 = np.diag([0, 1]).astype(np.complex128)


def _pack(qiskit_mps):
    gam, lam = qiskit_mps
    n = len(gam)
    dims = np.ones(n + 1, dtype=np.int32)
    for q in range(n):
        g0 = np.asarray(gam[q][0])
        if g0.ndim != 2 or np.asarray(gam[q][1]).shape != g0.shape or g0.shape[0] != dims[q]:
            raise ValueError("inconsistent MPS tensor shapes")
        dims[q + 1] = g0.shape[1]
    if dims[n] != 1 or len(lam) != n - 1:
        raise ValueError("not a valid MPS in Qiskit format")
    g = np.concatenate([np.stack([np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128)]).ravel() for a, b in gam])
    lm = np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in lam]) if n > 1 else np.zeros(1)
    for q in range(n - 1):
        if np.asarray(lam[q]).size != dims[q + 1]:
            raise ValueError("Schmidt vector size differs from the bond dimension")
    return n, dims, np.ascontiguousarray(g), np.ascontiguousarray(lm)


def is_canonical(qiskit_mps, tol: float = 1e-8) -> bool:
    """Vidal canonical form, checked on the host: with A_q[b] = Gamma_q[b] diag(lambda_q) every site is right-normalised,
    sum_b A_q[b] A_q[b]^H = 1, and with B_q[b] = diag(lambda_{q-1}) Gamma_q[b] left-normalised, sum_b B_q[b]^H B_q[b] = 1
    (O(n chi^3) on small matrices; Aer's states pass, hand-made tensors such as the oracle's random_mps do not)."""
    gam, lam = qiskit_mps
    n = len(gam)
    for q in range(n):
        g0, g1 = np.asarray(gam[q][0], dtype=np.complex128), np.asarray(gam[q][1], dtype=np.complex128)
        lr = np.asarray(lam[q], dtype=np.float64).ravel() if q < n - 1 else np.ones(1)
        ll = np.asarray(lam[q - 1], dtype=np.float64).ravel() if q > 0 else np.ones(1)
        right = sum((g * lr[None, :]) @ (g * lr[None, :]).conj().T for g in (g0, g1))
        left = sum((ll[:, None] * g).conj().T @ (ll[:, None] * g) for g in (g0, g1))
        if np.abs(right - np.eye(right.shape[0])).max() > tol or np.abs(left - np.eye(left.shape[0])).max() > tol:
            return False
    return True


def _default_device() -> int:
    from .engine import default_device

    return default_device()


_CANONICAL_CACHE: dict = {}   # id(tuple) -> (weak liveness token, verdict); a few entries (targets of running optimisations)


def _canonical_verdict(qiskit_mps) -> bool:
    """``is_canonical`` once per tuple object: the same target tuple arrives on every evaluation of an optimisation
    (mps_dot_objective.py:41).  Keyed by identity plus the shapes and a corner of every tensor (an in-place edit that keeps
    those is the caller's to announce by passing a new tuple)."""
    key = id(qiskit_mps)
    gam, lam = qiskit_mps
    mark = tuple((np.shape(g0), complex(np.asarray(g0).flat[0]), complex(np.asarray(g1).flat[-1])) for g0, g1 in gam)
    hit = _CANONICAL_CACHE.get(key)
    if hit is not None and hit[0] == mark:
        return hit[1]
    verdict = is_canonical(qiskit_mps)
    if len(_CANONICAL_CACHE) > 64:
        _CANONICAL_CACHE.clear()
    _CANONICAL_CACHE[key] = (mark, verdict)
    return verdict


_SERIALS = __import__("itertools").count(1)


class DeviceMPS:
    """One MPS resident on the GPU."""

    def __init__(self, handle: c_void_p):
        self.handle = handle
        self._L = _lib.lib()
        self.version = 0   # counts the in-place changes of the state (copies held elsewhere, e.g. by LockstepLanes, go stale)
        self.serial = next(_SERIALS)   # never reused (unlike id()): what holders of copies remember instead of a reference to the state

    @classmethod
    def from_qiskit(cls, qiskit_mps, device: Optional[int] = None, trunc_thr: float = 0.0, assume_canonical: bool = False) -> "DeviceMPS":
        """Uploads a QiskitMPS tuple.  The engine's truncation rule is stated on Schmidt values, i.e. for states in
        canonical (Vidal) form -- what Aer hands the reference (mps_operations.py:216-243).  When a real truncation is asked
        for (``trunc_thr`` > 1e-12) an input that is NOT canonical is brought into that form first (two sweeps of exact
        SVDs, ``canonicalize``); with exact arithmetic the gauge does not matter and the tensors are taken as they are.
        ``device`` None: this rank's GPU (``engine.default_device()``: LOCAL_RANK under a one-process-per-GPU launcher).
        The O(n chi^3) host check is made once per tuple (the verdict is remembered by the tuple's identity, the target of an
        optimisation arrives on every evaluation); ``assume_canonical`` skips it (states that come from Aer or this engine)."""
        n, dims, g, lm = _pack(qiskit_mps)
        h = c_void_p()
        dev = _default_device() if device is None else int(device)
        check(_lib.lib().aqc_mps_create(dev, n, iptr(dims), dptr(g), dptr(lm), byref(h)))
        m = cls(h)
        if trunc_thr > 1e-12 and not assume_canonical and not _canonical_verdict(qiskit_mps):
            m.canonicalize()
        return m

    def canonicalize(self) -> "DeviceMPS":
        """Canonical form by exact identity "gates" on every bond: right to left (all sites right-orthonormal), then left to
        right (the singular values of each bond are now the state's Schmidt values)."""
        eye4 = np.eye(4, dtype=np.complex128)
        n = self.num_qubits
        for q in range(n - 2, -1, -1):
            self.gate2(eye4, q, q + 1, 0.0)
        for q in range(n - 1):
            self.gate2(eye4, q, q + 1, 0.0)
        return self

    @classmethod
    def basis_state(cls, num_qubits: int, index: int = 0, device: Optional[int] = None) -> "DeviceMPS":
        """Product state |index> (bit q of ``index`` = qubit q)."""
        index = int(index)   # Python integer: registers beyond 63 qubits
        gam = [((np.array([[1.0 - ((index >> q) & 1)]], dtype=np.complex128)), np.array([[float((index >> q) & 1)]], dtype=np.complex128))
               for q in range(num_qubits)]
        return cls.from_qiskit((gam, [np.ones(1) for _ in range(num_qubits - 1)]), device)

    @classmethod
    def from_vector(cls, vec, trunc_thr: float = 0.0, max_bond: int = 0, *, device: Optional[int] = None, method=None, details: bool = False):
        """The MPS of one dense vector of 2^n amplitudes (index bit q is site q), every bond truncated: ``from_vectors`` of this vector."""
        if np.ndim(vec) != 1:
            raise ValueError("expects one vector of 2^n amplitudes")
        return from_vectors(np.asarray(vec), trunc_thr, max_bond, device=device, method=method, details=details)

    def clone(self) -> "DeviceMPS":
        h = c_void_p()
        check(self._L.aqc_mps_clone(self.handle, byref(h)))
        return DeviceMPS(h)

    @property
    def num_qubits(self) -> int:
        return int(self._L.aqc_mps_num_qubits(self.handle))

    @property
    def bond_dims(self) -> np.ndarray:
        d = np.zeros(self.num_qubits + 1, dtype=np.int32)
        check(self._L.aqc_mps_dims(self.handle, iptr(d)))
        return d

    @property
    def discarded_weight(self) -> float:
        """Sum of the squared singular values dropped by all truncations so far."""
        return float(self._L.aqc_mps_discarded_weight(self.handle))

    def to_qiskit(self):
        d = self.bond_dims
        n = self.num_qubits
        sizes = [2 * int(d[q]) * int(d[q + 1]) for q in range(n)]
        g = np.empty(sum(sizes), dtype=np.complex128)
        lm = np.empty(max(int(d[1:n].sum()), 1), dtype=np.float64)
        check(self._L.aqc_mps_export(self.handle, dptr(g), dptr(lm)))
        gam, lam, off, loff = [], [], 0, 0
        for q in range(n):
            t = g[off:off + sizes[q]].reshape(2, int(d[q]), int(d[q + 1]))
            gam.append((t[0].copy(), t[1].copy()))
            off += sizes[q]
            if q < n - 1:
                lam.append(lm[loff:loff + int(d[q + 1])].copy())
                loff += int(d[q + 1])
        return gam, lam

    def gate1(self, gate, qubit: int) -> "DeviceMPS":
        g = np.ascontiguousarray(gate, dtype=np.complex128)
        if g.shape != (2, 2):
            raise ValueError("expects a 2x2 gate")
        check(self._L.aqc_mps_gate1(self.handle, int(qubit), dptr(g)))
        self.version += 1
        return self

    def gate2(self, gate4, ctrl: int, targ: int, trunc_thr: float = 0.0, max_bond: int = 0) -> "DeviceMPS":
        g = np.ascontiguousarray(gate4, dtype=np.complex128)
        if g.shape != (4, 4):
            raise ValueError("expects a 4x4 gate")
        check(self._L.aqc_mps_gate2(self.handle, int(ctrl), int(targ), dptr(g), float(trunc_thr), int(max_bond)))
        self.version += 1
        return self

    def dot(self, other: "DeviceMPS") -> np.complex128:
        """<self|other>."""
        out = np.empty(1, dtype=np.complex128)
        check(self._L.aqc_mps_dot(self.handle, other.handle, dptr(out)))
        return np.complex128(out[0])

    def dot_ops(self, other: "DeviceMPS", ops) -> np.complex128:
        """<(prod G_i on qubit_i) self|other> for ``ops = [(qubit, 2x2 gate), ...]`` on distinct qubits, without
        building the transformed state."""
        qs = np.ascontiguousarray([q for q, _ in ops], dtype=np.int32)
        gs = np.ascontiguousarray(np.stack([np.asarray(g, dtype=np.complex128) for _, g in ops]))
        out = np.empty(1, dtype=np.complex128)
        check(self._L.aqc_mps_dot_ops(self.handle, other.handle, len(ops), iptr(qs), dptr(gs), dptr(out)))
        return np.complex128(out[0])

    def sample(self, shots: int, *, seed: int, first_shot: int = 0, method=None, details: bool = False):
        """Shots drawn from |psi(b)|^2: ``mps_sampling.sample`` of this state."""
        from .mps_sampling import sample

        return sample(self, shots, seed=seed, first_shot=first_shot, method=method, details=details)

    def amplitudes(self, bits, *, method=None) -> np.ndarray:
        """psi(b) of the given bit strings: ``mps_sampling.amplitudes`` of this state."""
        from .mps_sampling import amplitudes

        return amplitudes(self, bits, method=method)

    @property
    def device(self) -> int:
        return int(self._L.aqc_mps_device(self.handle))

    def to_vector(self, **kw):
        """The dense vector of 2^n amplitudes (n <= 30): ``to_vectors`` of this state."""
        return to_vectors(self, **kw)

    def amplitude_blocks(self, low_qubits: int, high_bits, **kw) -> np.ndarray:
        """The 2^low_qubits amplitudes of every listed row of high bits: ``amplitude_blocks`` of this state."""
        return amplitude_blocks(self, low_qubits, high_bits, **kw)

    def pauli_strings(self, strings, *, bra=None, method=None) -> np.ndarray:
        """<self|P_s|self> (with ``bra``: <bra|P_s|self>) of the given Pauli strings: ``mps_observables.pauli_strings`` of this state."""
        from .mps_observables import pauli_strings

        return pauli_strings(self, strings, bras=bra, method=method)

    def overlaps(self, kets, *, method=None) -> np.ndarray:
        """<self|psi_b> for a list of states, ``(len(kets),)``: row 0 of ``mps_observables.overlaps``."""
        from .mps_observables import overlaps

        return overlaps([self], kets, method=method)[0]

    def operator_elements(self, op, bras=None, *, method=None):
        """<self|O|self> for an ``MPO`` (``None``: the identity), or with ``bras`` (a list) the ``(len(bras),)`` values <bra|O|self>:
        ``mps_observables.operator_elements`` with this state as the ket."""
        from .mps_observables import operator_elements

        if bras is None:
            return operator_elements([(self, op, self)], method=method)[0]
        if not isinstance(bras, list):
            raise ValueError("bras is a list of states")
        return operator_elements([(b, op, self) for b in bras], method=method)

    def schmidt_values(self, *, method=None, details: bool = False):
        """The singular values of every cut, ``(n - 1, K)``: ``mps_observables.schmidt_values`` of this state (which it leaves as it is)."""
        from .mps_observables import schmidt_values

        return schmidt_values(self, method=method, details=details)

    def entropies(self, alpha: float = 1.0, *, method=None) -> np.ndarray:
        """The entanglement entropy of every cut, ``(n - 1,)``: ``mps_observables.entanglement_entropies`` of this state."""
        from .mps_observables import entanglement_entropies

        return entanglement_entropies(self, alpha, method=method)

    def compressed(self, trunc_thr: float = 0.0, max_bond: int = 0, *, method=None, details: bool = False):
        """A new state: this one in canonical form with every bond truncated (``compress`` of this state, which it leaves as it is)."""
        return compress(self, trunc_thr, max_bond, method=method, details=details)

    def compress(self, trunc_thr: float = 0.0, max_bond: int = 0, *, method=None) -> "DeviceMPS":
        """The same in place: this object takes over the compressed state (copies held elsewhere go stale, ``version`` counts it)."""
        new = compress(self, trunc_thr, max_bond, method=method)
        old, self.handle, new.handle = self.handle, new.handle, None
        self._L.aqc_mps_destroy(old)
        self.version += 1
        return self

    def plus(self, other, coeff=1.0, trunc_thr: float = 0.0, max_bond: int = 0, **kw):
        """A new state: self + coeff other, compressed (``linear_combinations`` of the two, which it leaves as they are)."""
        return linear_combinations([self, other], [1.0, coeff], trunc_thr, max_bond, **kw)

    def scaled(self, coeff) -> "DeviceMPS":
        """A new state: coeff self, in the engine's gauge (``linear_combinations`` of this state alone)."""
        return linear_combinations([self], [coeff])

    def applied_operator(self, op, trunc_thr: float = 0.0, max_bond: int = 0, **kw):
        """A new state: the ``MPO`` ``op`` applied to this one, compressed (``apply_operator`` of this state, which it leaves as it is)."""
        return apply_operator(op, self, trunc_thr, max_bond, **kw)

    def applied(self, gates, trunc_thr: float = 0.0, max_bond: int = 0, *, method=None, details: bool = False):
        """A new state: the program ``gates`` applied to this one (``apply_gates`` of this state, which it leaves as it is)."""
        return apply_gates(self, gates, trunc_thr, max_bond, method=method, details=details)

    def close(self) -> None:
        if self.handle:
            self._L.aqc_mps_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- what the wrappers of the many-state calls share (the Python side of DESIGN.md §6w): the states of a call, its method and
# truncation, the rule's route, and the new states of a truncating call

_BOND_DIMS_OF_A_STATE = "expects the n + 1 bond dimensions of a state"


def _is_tuple_state(s) -> bool:
    return isinstance(s, tuple) and len(s) == 2   # a QiskitMPS (gammas, lambdas); several states come as a list


def _call_states(states, device_only: bool = False):
    """``(single, items, n, bond dimensions)`` of the states of a call -- a DeviceMPS, a QiskitMPS tuple or a list of those -- read on
    the host, so that a refused call uploads nothing (a tuple is only packed).  ``device_only``: DeviceMPS only, on one device."""
    if device_only:
        single = isinstance(states, DeviceMPS)
        items = [states] if single else states
        if not isinstance(items, (list, tuple)) or not items or any(not isinstance(s, DeviceMPS) for s in items):
            raise ValueError("states is a DeviceMPS or a non-empty list of them")
    else:
        single = isinstance(states, DeviceMPS) or _is_tuple_state(states)
        if not single and not isinstance(states, list):
            raise ValueError("states is a DeviceMPS, a QiskitMPS tuple or a list of those")
        items = [states] if single else states
        if not items:
            raise ValueError("expects at least one state")
    dims = []
    for s in items:
        if isinstance(s, DeviceMPS):
            if not s.handle:
                raise ValueError("a closed DeviceMPS")
            dims.append(np.asarray(s.bond_dims))
        elif _is_tuple_state(s):
            dims.append(_pack(s)[1])
        else:
            raise ValueError("a state is a DeviceMPS or a QiskitMPS tuple")
    if len({d.size for d in dims}) > 1 or (device_only and len({s.device for s in items}) > 1):
        raise ValueError("the states differ in size or device" if device_only else "the states differ in the number of qubits")
    return single, list(items), dims[0].size - 1, dims


def _handles(lanes):
    """Open DeviceMPS states as the handle array that the native calls take."""
    return (c_void_p * len(lanes))(*[m.handle for m in lanes])


class _Lanes:
    """The states of a call as DeviceMPS handles.  Making one reads the states on the host (``_call_states``: ``single``, ``items``,
    ``n``, ``dims``) and refuses what is no call; entering it uploads the tuples; what was uploaded for the call is closed on exit."""

    def __init__(self, states):
        self.single, self.items, self.n, self.dims = _call_states(states)
        self.own = []
        self.lanes = []

    def __enter__(self):
        try:
            for s in self.items:
                if not isinstance(s, DeviceMPS):
                    s = DeviceMPS.from_qiskit(s, assume_canonical=True)   # exact arithmetic: the gauge is taken as it is
                    self.own.append(s)
                self.lanes.append(s)
        except Exception:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        for m in self.own:
            m.close()
        self.own = []
        return False

    def handles(self):
        return _handles(self.lanes)


def _method_code(method, table) -> int:
    """The native code of a call's ``method`` out of the call's table of them."""
    if method not in table:
        names = [repr(k) for k in table]
        raise ValueError(f"method must be {', '.join(names[:-1])} or {names[-1]}, not {method!r}")
    return table[method]


def _within_fused_cap(method, dims, cap: int) -> None:
    """Refuses ``method="fused"`` for a state beyond the cap, before the native call."""
    if method == "fused":
        for d in dims:
            if int(d.max()) > cap:
                raise ValueError(f"the fused route takes bond dimensions up to {cap}, not {int(d.max())}")


def _truncation(trunc_thr, max_bond) -> Tuple[float, int]:
    trunc_thr, max_bond = float(trunc_thr), int(max_bond)
    if not (trunc_thr >= 0.0 and np.isfinite(trunc_thr)) or max_bond < 0:
        raise ValueError("trunc_thr and max_bond must be non-negative")
    return trunc_thr, max_bond


def _route_of(entry: str, names: dict, refusal: str, args) -> str:
    """The answer of the native rule ``entry`` to ``args`` by name (``args`` None: the caller's shape test failed); what the test or the
    rule itself refuses is a ``ValueError``."""
    r = getattr(_lib.lib(), entry)(*args) if args is not None else -1
    if r not in names:
        raise ValueError(refusal)
    return names[r]


def _adopt(out):
    """The handle array that a truncating call filled as ``DeviceMPS | None`` per lane."""
    return [DeviceMPS(c_void_p(h)) if h else None for h in out]


def _failed_cut(ranks) -> int:
    """The cut at which a lane of a sweep failed: the first one without a rank (0 for a single site)."""
    return int(np.flatnonzero(ranks == 0)[0]) + 1 if ranks.size else 0


def _finish(made, status, words, place, single, details, per_lane, per_call=()):
    """What a truncating call returns.  A lane with a status failed: without ``details`` every state the call made is closed and the
    first such lane raises ``RuntimeError`` (``place(lane)``: where, ``words``: why); with ``details`` its entry of ``made`` is None.
    ``per_lane`` info is unwrapped with the states for a single one, ``per_call`` info is not."""
    bad = np.flatnonzero(status)
    if bad.size and not details:
        lane = int(bad[0])
        for m in made:
            if m is not None:
                m.close()
        raise RuntimeError(f"{place(lane)}: {words.get(int(status[lane]), 'failed')}")
    result = made[0] if single else made
    if not details:
        return result
    info = {k: v[0] for k, v in per_lane.items()} if single else dict(per_lane)
    info.update(per_call)
    return result, info


# ---- compression: canonical form and truncation of every bond (aqc_mps_compress; rules: csrc/aqc_mps_compress_rule.h, kernels:
# csrc/aqc_mps_compress.hip)

COMPRESS_FUSED_CAP = 64                                       # AQC_MPS_ENT_FUSED_CAP
_COMPRESS_METHODS = {None: 0, "fused": 1, "canonical": 2}     # AQC_MPS_ENT_*
_COMPRESS_ROUTES = {1: "fused", 2: "canonical"}
_COMPRESS_STATUS = {1: "the SVD of the cut reached its sweep limit", 2: "the state is zero or not finite"}


def compress_route(bond_dims) -> str:
    """The route ``compress`` picks for a state with these n + 1 bond dimensions: ``"fused"`` when every bond is at most
    ``COMPRESS_FUSED_CAP``, else ``"canonical"``."""
    d = np.ascontiguousarray(bond_dims, dtype=np.int32)
    return _route_of("aqc_mps_compress_route", _COMPRESS_ROUTES, _BOND_DIMS_OF_A_STATE, (d.size - 1, iptr(d)) if d.ndim == 1 and d.size >= 2 else None)


def compress(states, trunc_thr: float = 0.0, max_bond: int = 0, *, method: Optional[str] = None, details: bool = False):
    """New states: the given ones in the engine's canonical gauge (site tensors Gamma_q lambda_q, the bond vectors the Schmidt values),
    every bond truncated left to right by the engine's rank rule at ``trunc_thr`` / ``max_bond`` with the rescaling of a truncating
    gate -- the decisions of ``clone().canonicalize()`` followed by a sweep of truncating identity ``gate2`` calls, in one call for one
    or many states.  ``states``: a DeviceMPS, a QiskitMPS tuple or a list of those, any gauge, one qubit count; they are not modified.
    Returns a DeviceMPS for one state, a list for a list; ``discarded_weight`` is the input's plus what the cuts dropped.  At
    ``trunc_thr`` = 0 (and no binding ``max_bond``) the bond vectors are the state's Schmidt values and the state itself is unchanged;
    with truncation a bond vector holds the values of its cut when it was decided, as after the loop of gates.

    ``method``: ``None`` lets the rule choose per state (``compress_route``): ``"fused"`` (bonds up to ``COMPRESS_FUSED_CAP``) sweeps all
    states of the call together on the device, the rank decisions included, with one synchronisation per call; ``"canonical"`` (any
    bond) runs the engine's sweeps on a clone.  A state's result does not depend on which other states are in the call.

    A state that is zero or not finite, or whose SVD reaches its sweep limit, fails alone: without ``details`` that raises
    ``RuntimeError`` naming the lane and the cut; with ``details`` its entry is ``None`` and the second return value
    ``{"ranks", "dropped", "sweeps", "status", "route"}`` tells why (ranks are 0 from the failed cut on)."""
    code = _method_code(method, _COMPRESS_METHODS)
    trunc_thr, max_bond = _truncation(trunc_thr, max_bond)
    lanes = _Lanes(states)
    if method == "fused" and any(int(d.max()) > COMPRESS_FUSED_CAP for d in lanes.dims):
        raise ValueError(f"the fused route takes bond dimensions up to {COMPRESS_FUSED_CAP}")
    count, n = len(lanes.items), lanes.n
    routes = [method or compress_route(d) for d in lanes.dims]
    out = (c_void_p * count)()
    ranks, sweeps = np.zeros((count, n - 1), dtype=np.int32), np.zeros((count, n - 1), dtype=np.int32)
    dropped, status = np.zeros((count, n - 1), dtype=np.float64), np.zeros(count, dtype=np.int32)
    with lanes:
        check(_lib.lib().aqc_mps_compress(lanes.handles(), count, trunc_thr, max_bond, code, out, iptr(ranks), dptr(dropped), iptr(sweeps), iptr(status)))
        made = _adopt(out)
    return _finish(made, status, _COMPRESS_STATUS, lambda lane: f"state {lane}, cut {_failed_cut(ranks[lane])}", lanes.single, details,
                   {"ranks": ranks, "dropped": dropped, "sweeps": sweeps, "status": status, "route": routes})


# ---- linear combinations: sums of states, compressed (aqc_mps_combine; rules: csrc/aqc_mps_combine_rule.h, kernel:
# csrc/aqc_mps_combine.hip, the sweep of compression)

def combine_route(bond_dims_of_terms) -> str:
    """The route ``linear_combinations`` picks for an output whose terms have these bond dimensions (K rows of n + 1): ``"fused"`` when
    every summed bond is at most ``COMPRESS_FUSED_CAP``, else ``"canonical"``."""
    d = np.ascontiguousarray(bond_dims_of_terms, dtype=np.int32)
    fits = d.ndim == 2 and d.shape[0] >= 1 and d.shape[1] >= 2
    return _route_of("aqc_mps_combine_route", _COMPRESS_ROUTES, "expects the n + 1 bond dimensions of every term, (K, n + 1)",
                     (d.shape[1] - 1, d.shape[0], iptr(d)) if fits else None)


def linear_combinations(states, coeffs, trunc_thr: float = 0.0, max_bond: int = 0, *, method: Optional[str] = None, details: bool = False):
    """New states sum_k coeffs[k] states[k], compressed: the direct sum of the terms (bonds sum_k chi^k_q, assembled on the device) goes
    through ``compress`` at ``trunc_thr`` / ``max_bond`` -- the engine's gauge, every bond cut left to right by the engine's rank rule,
    the same statuses.  ``states``: a list of K DeviceMPS or QiskitMPS tuples of one qubit count, any gauge; the same object may be
    listed twice; they are not modified.  ``coeffs``: complex ``(K,)`` gives one new state, ``(J, K)`` a list of J.  An exactly zero
    coefficient leaves its term out of that output (outputs may have different numbers of terms); a row of zeros is a ``ValueError``.

    The result's ``discarded_weight`` is what the cuts of this call dropped; the weights the terms carry are not taken over.  Errors are
    of the size of rounding relative to ``scale = sum_k |c_k| |psi_k|``, not to the norm of the result: an exact cancellation is not
    detected (psi - psi gives rounding of that size, not a failure).

    ``method``: ``None`` lets the rule choose per output (``combine_route``): ``"fused"`` (summed bonds up to ``COMPRESS_FUSED_CAP``)
    sweeps all outputs of the call together with one synchronisation; ``"canonical"`` (any bond) adopts the sum as an engine state and
    runs the engine's sweeps on it.  An output's result does not depend on which other outputs are in the call.

    An output whose coefficients or tensors are not finite, or whose SVD reaches its sweep limit, fails alone: without ``details`` that
    raises ``RuntimeError`` naming the output and the cut; with ``details`` its entry is ``None`` and the second return value
    ``{"ranks", "dropped", "sweeps", "status", "route"}`` tells why."""
    code = _method_code(method, _COMPRESS_METHODS)
    trunc_thr, max_bond = _truncation(trunc_thr, max_bond)
    if not isinstance(states, list) or not states:
        raise ValueError("states is a list of DeviceMPS or QiskitMPS tuples")
    # the same object listed twice is uploaded once and is one state of the call
    first, distinct = {}, []
    for s in states:
        if id(s) not in first:
            first[id(s)] = len(distinct)
            distinct.append(s)
    index = np.array([first[id(s)] for s in states], dtype=np.int32)
    lanes = _Lanes(distinct)
    shapes, n = [lanes.dims[k] for k in index], lanes.n
    c = np.asarray(coeffs, dtype=np.complex128)
    single = c.ndim == 1
    if c.ndim not in (1, 2) or c.shape[-1] != len(states) or c.size == 0:
        raise ValueError(f"coeffs must have shape ({len(states)},) or (J, {len(states)})")
    c = np.atleast_2d(c)
    term_off, term_state, routes = [0], [], []
    for j, row in enumerate(c):
        used = [k for k in range(len(states)) if row[k] != 0]   # (NaN != 0: a NaN coefficient is data, and fails its output)
        if not used:
            raise ValueError(f"output {j}: every coefficient is zero")
        term_state += used
        term_off.append(len(term_state))
        route = combine_route(np.stack([shapes[k] for k in used]))
        if method == "fused" and route != "fused":
            raise ValueError(f"the fused route takes summed bond dimensions up to {COMPRESS_FUSED_CAP} (output {j})")
        routes.append(method or route)
    term_off, term_state = np.array(term_off, dtype=np.int32), np.array(term_state, dtype=np.int32)
    cf = np.ascontiguousarray(np.concatenate([row[term_state[term_off[j]:term_off[j + 1]]] for j, row in enumerate(c)]))
    term_state = np.ascontiguousarray(index[term_state])
    count = c.shape[0]
    out = (c_void_p * count)()
    ranks, sweeps = np.zeros((count, max(n - 1, 0)), dtype=np.int32), np.zeros((count, max(n - 1, 0)), dtype=np.int32)
    dropped, status = np.zeros((count, max(n - 1, 0)), dtype=np.float64), np.zeros(count, dtype=np.int32)
    with lanes:
        check(_lib.lib().aqc_mps_combine(lanes.handles(), len(lanes.lanes), count, iptr(term_off), iptr(term_state), dptr(cf), trunc_thr, max_bond,
                                         code, out, iptr(ranks), dptr(dropped), iptr(sweeps), iptr(status)))
        made = _adopt(out)
    return _finish(made, status, _COMPRESS_STATUS, lambda lane: f"output {lane}, cut {_failed_cut(ranks[lane])}", single, details,
                   {"ranks": ranks, "dropped": dropped, "sweeps": sweeps, "status": status, "route": routes})


# ---- operator sums: sum_t c_t O_t psi_t, compressed (aqc_mps_opsum; rules: csrc/aqc_mps_opsum_rule.h, kernel: csrc/aqc_mps_opsum.hip,
# the sweep of compression)

_PAULIS = (np.eye(2, dtype=np.complex128), _X, _Y, _Z)
MPO_DENSE_MAX_QUBITS = 12


class MPO:
    """A matrix-product operator on the host: sites W_q of shape ``(D_q, D_{q+1}, 2, 2)``, complex128, indexed ``[a][b][s_out][s_in]``,
    D_0 = D_n = 1.  O(b_out, b_in) = W_0[:, :, b_out0, b_in0] ... W_{n-1}[...] as a product of D x D matrices; qubit q is index bit q of
    the dense vector (the project's order).  No gauge or Hermiticity is assumed.  Immutable: the sites are copies that cannot be written."""

    __slots__ = ("_sites", "_dims")

    def __init__(self, sites):
        if not isinstance(sites, (list, tuple)) or len(sites) < 1:
            raise ValueError("an MPO is a non-empty list of site tensors (D_q, D_{q+1}, 2, 2)")
        made, dims = [], [1]
        for q, w in enumerate(sites):
            w = np.array(w, dtype=np.complex128, order="C")
            if w.ndim != 4 or w.shape[2:] != (2, 2) or w.shape[0] < 1 or w.shape[1] < 1:
                raise ValueError(f"MPO site {q}: expects shape (D_q, D_q+1, 2, 2), not {w.shape}")
            if w.shape[0] != dims[-1]:
                raise ValueError(f"MPO site {q}: its left bond {w.shape[0]} differs from the bond {dims[-1]} before it")
            dims.append(w.shape[1])
            w.setflags(write=False)
            made.append(w)
        if dims[-1] != 1:
            raise ValueError(f"the last bond of an MPO is 1, not {dims[-1]}")
        object.__setattr__(self, "_sites", tuple(made))
        object.__setattr__(self, "_dims", np.array(dims, dtype=np.int32))
        self._dims.setflags(write=False)

    def __setattr__(self, name, value):
        raise AttributeError("an MPO is immutable")

    @property
    def sites(self):
        return self._sites

    @property
    def num_qubits(self) -> int:
        return len(self._sites)

    @property
    def bond_dims(self) -> np.ndarray:
        """D_0 .. D_n."""
        return self._dims

    def to_dense(self) -> np.ndarray:
        """The 2^n x 2^n matrix (n <= ``MPO_DENSE_MAX_QUBITS``), row b_out, column b_in, contracted from site 0 on."""
        n = self.num_qubits
        if n > MPO_DENSE_MAX_QUBITS:
            raise ValueError(f"to_dense takes operators on up to {MPO_DENSE_MAX_QUBITS} qubits, not {n}")
        acc = np.ones((1, 1, 1), dtype=np.complex128)   # [rows][columns][bond]
        for w in self._sites:
            r, c = acc.shape[:2]
            acc = np.einsum("rca,abst->srtcb", acc, w).reshape(2 * r, 2 * c, w.shape[1])   # bit q is the major one so far
        return np.ascontiguousarray(acc[:, :, 0])

    def adjoint(self) -> "MPO":
        """O^H: every site with s_out and s_in swapped and conjugated; the bonds stay.  Exact."""
        return MPO([w.transpose(0, 1, 3, 2).conj() for w in self._sites])

    def times(self, other: "MPO") -> "MPO":
        """self . other (``other`` acts first) as an MPO with bonds D_self D_other, self's index the major one:
        W[(a2, a1)][(b2, b1)][s][s'] = sum_t W_self[a2][b2][s][t] W_other[a1][b1][t][s'].  Nothing is compressed."""
        if not isinstance(other, MPO):
            raise ValueError("an operator is an MPO")
        if other.num_qubits != self.num_qubits:
            raise ValueError(f"an operator on {self.num_qubits} qubits meets one on {other.num_qubits}")
        return MPO([np.einsum("abst,cdtu->acbdsu", w2, w1).reshape(w2.shape[0] * w1.shape[0], w2.shape[1] * w1.shape[1], 2, 2)
                    for w2, w1 in zip(self._sites, other._sites)])

    @classmethod
    def product_operator(cls, matrices) -> "MPO":
        """M_0 on qubit 0 (x) M_1 on qubit 1 ...: bond dimension 1 (projectors, local rotations)."""
        if not isinstance(matrices, (list, tuple)) or len(matrices) < 1:
            raise ValueError("expects a non-empty list of 2 x 2 matrices")
        mats = [np.asarray(m, dtype=np.complex128) for m in matrices]
        if any(m.shape != (2, 2) for m in mats):
            raise ValueError("expects 2 x 2 matrices")
        return cls([m.reshape(1, 1, 2, 2) for m in mats])

    @classmethod
    def identity(cls, num_qubits: int) -> "MPO":
        if int(num_qubits) < 1:
            raise ValueError("an operator acts on at least one qubit")
        return cls.product_operator([_PAULIS[0]] * int(num_qubits))

    @staticmethod
    def _letters(strings, num_qubits):
        from .mps_observables import _strings

        if num_qubits is None:
            first = strings[0] if isinstance(strings, (list, tuple)) and len(strings) else None
            if isinstance(strings, np.ndarray) and strings.ndim == 2:
                num_qubits = strings.shape[1]
            elif isinstance(first, str):
                num_qubits = len(first)
            else:
                raise ValueError("num_qubits is needed for strings given as (letters, qubits)")
        if int(num_qubits) < 1:
            raise ValueError("an operator acts on at least one qubit")
        return _strings(strings, int(num_qubits))

    @classmethod
    def from_pauli_string(cls, string, coeff=1.0, *, num_qubits: Optional[int] = None) -> "MPO":
        """coeff P for one Pauli string as ``mps_observables.pauli_strings`` takes it (letter q acts on qubit q): bond dimension 1,
        the coefficient on site 0."""
        return cls.from_pauli_sum([(coeff, string)], num_qubits=num_qubits)

    @classmethod
    def from_pauli_sum(cls, terms, *, num_qubits: Optional[int] = None) -> "MPO":
        """sum_k w_k P_k for ``terms = [(weight, string), ...]`` as ``mps_observables.energy`` takes them, complex weights allowed: the
        direct sum of the strings, bond dimension = the number of terms, exact (nothing is compressed); the weights sit on site 0."""
        if not isinstance(terms, (list, tuple)) or len(terms) < 1 or any(not (isinstance(t, tuple) and len(t) == 2) for t in terms):
            raise ValueError("terms is a non-empty list of (weight, string)")
        w = np.array([complex(t[0]) for t in terms], dtype=np.complex128)
        strings = [t[1] for t in terms]
        letters = cls._letters(np.stack(strings) if isinstance(strings[0], np.ndarray) else strings, num_qubits)
        k, n = letters.shape
        if n == 1:
            return cls([sum(w[t] * _PAULIS[letters[t, 0]] for t in range(k)).reshape(1, 1, 2, 2)])
        sites = []
        for q in range(n):
            site = np.zeros((1 if q == 0 else k, 1 if q == n - 1 else k, 2, 2), dtype=np.complex128)
            for t in range(k):
                site[0 if q == 0 else t, 0 if q == n - 1 else t] = (w[t] if q == 0 else 1.0) * _PAULIS[letters[t, q]]
            sites.append(site)
        return cls(sites)

    @classmethod
    def xxz(cls, num_qubits: int, delta: float) -> "MPO":
        """H = -1/4 sum_i (X_i X_{i+1} + Y_i Y_{i+1} + delta Z_i Z_{i+1}) on the open chain of ``xxz.py``: the automaton of bond
        dimension 5 (0: nothing placed yet, 1 .. 3: X, Y, Z placed on the site before, 4: a bond term is complete)."""
        n, delta = int(num_qubits), float(delta)
        if n < 1:
            raise ValueError("an operator acts on at least one qubit")
        if n == 1:
            return cls([np.zeros((1, 1, 2, 2), dtype=np.complex128)])
        full = np.zeros((5, 5, 2, 2), dtype=np.complex128)
        full[0, 0] = full[4, 4] = _PAULIS[0]
        for a, (p, weight) in enumerate(((_X, -0.25), (_Y, -0.25), (_Z, -0.25 * delta)), start=1):
            full[0, a] = p
            full[a, 4] = weight * p
        return cls([full[:1]] + [full] * (n - 2) + [full[:, 4:]])


def _op_dims(op):
    if not isinstance(op, MPO):
        raise ValueError("an operator is an MPO or None")
    return op.bond_dims


def _packed_ops(ops, n: int):
    """``(op_dims (K, n + 1) int32, op_off (K, n + 1) int64, op_data complex128)``: the operators of a call in the packed layout of
    aqc_mps_opsum (site q of operator k at element ``op_off[k][q]``)."""
    op_dims = np.ascontiguousarray([op.bond_dims for op in ops], dtype=np.int32).reshape(len(ops), n + 1)
    sizes = np.array([[w.size for w in op.sites] for op in ops], dtype=np.int64).reshape(len(ops), n)
    op_off = np.zeros((len(ops), n + 1), dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(sizes.sum(axis=1))]) if len(ops) else np.zeros(1, dtype=np.int64)
    for k in range(len(ops)):
        op_off[k] = starts[k] + np.concatenate([[0], np.cumsum(sizes[k])])
    op_data = np.ascontiguousarray(np.concatenate([w.ravel() for op in ops for w in op.sites])) if ops else np.zeros(1, dtype=np.complex128)
    return op_dims, op_off, op_data


def opsum_route(bond_dims_of_states, bond_dims_of_ops) -> str:
    """The route ``operator_sums`` picks for an output whose terms have states and operators of these bond dimensions (K rows of n + 1
    each; ``None`` in place of an operator's row: no operator): ``"fused"`` when every summed product bond sum_t D^t_q chi^t_q is at most
    ``COMPRESS_FUSED_CAP``, else ``"canonical"``.  An XXZ Hamiltonian (D = 5) alone stays fused for state bonds up to 12, a Pauli string
    (D = 1) up to 64."""
    bad = "expects the n + 1 bond dimensions of every term's state and operator, (K, n + 1) each"
    try:
        d = np.ascontiguousarray(bond_dims_of_states, dtype=np.int32)
        if d.ndim != 2 or d.shape[0] < 1 or d.shape[1] < 2 or len(bond_dims_of_ops) != d.shape[0]:
            raise ValueError(bad)
        w = np.ascontiguousarray([np.ones(d.shape[1], dtype=np.int32) if r is None else np.asarray(r, dtype=np.int32) for r in bond_dims_of_ops], dtype=np.int32)
    except (TypeError, ValueError):
        raise ValueError(bad) from None
    return _route_of("aqc_mps_opsum_route", _COMPRESS_ROUTES, bad, (d.shape[1] - 1, d.shape[0], iptr(d), iptr(w)) if w.shape == d.shape else None)


def operator_sums(outputs, trunc_thr: float = 0.0, max_bond: int = 0, *, method: Optional[str] = None, details: bool = False):
    """New states sum_t c_t O_t psi_t, compressed, one per output: ``outputs`` is a list of outputs, each a list of terms
    ``(coeff, op_or_None, state)`` with ``op`` an ``MPO`` (``None``: the identity, the state itself) and ``state`` a DeviceMPS or a
    QiskitMPS tuple of the operator's qubit count, any gauge.  H psi, (H - E) psi and a Lanczos residual H v - alpha v - beta w are one
    output each, and all outputs of a call share one truncating sweep.  Nothing given is modified; operators and states that are the same
    object are uploaded once.  An exactly zero coefficient leaves its term out; an output left without terms is a ``ValueError``.

    The product O psi has bonds D_q chi_q (``MPO.bond_dims`` times the state's), the direct sum of an output's terms the sum of those;
    it is assembled on the device and goes through ``compress`` at ``trunc_thr`` / ``max_bond`` -- the engine's gauge, every bond cut
    left to right by the engine's rank rule, the same statuses.  The result's ``discarded_weight`` is what the cuts of this call dropped.
    Errors are of the size of rounding relative to ``scale = sum_t |c_t| |O_t|_2 |psi_t|``, not to the norm of the result.

    ``method``: ``None`` lets the rule choose per output (``opsum_route``): ``"fused"`` (summed product bonds up to
    ``COMPRESS_FUSED_CAP``: an XXZ Hamiltonian on state bonds up to 12, Pauli strings up to 64) sweeps all outputs of the call together
    with one synchronisation; ``"canonical"`` (any bond) adopts the sum as an engine state and runs the engine's sweeps on it.  An
    output's result does not depend on which other outputs are in the call.

    An output that is exactly zero (a projector that annihilates the state), whose coefficients, operator entries or tensors are not
    finite, or whose SVD reaches its sweep limit fails alone: without ``details`` that raises ``RuntimeError`` naming the output and the
    cut; with ``details`` its entry is ``None`` and the second return value ``{"ranks", "dropped", "sweeps", "status", "route"}`` tells
    why."""
    code = _method_code(method, _COMPRESS_METHODS)
    trunc_thr, max_bond = _truncation(trunc_thr, max_bond)
    if not isinstance(outputs, list) or not outputs:
        raise ValueError("outputs is a non-empty list of outputs, each a list of (coeff, op_or_None, state)")
    states, ops, state_at, op_at = [], [], {}, {}
    term_off, term_state, term_op, cf, routes, n = [0], [], [], [], [], None
    for j, terms in enumerate(outputs):
        if not isinstance(terms, list) or any(not (isinstance(t, tuple) and len(t) == 3) for t in terms):
            raise ValueError(f"output {j}: expects a list of (coeff, op_or_None, state)")
        chi, dop = [], []
        for coeff, op, state in terms:
            coeff = complex(coeff)
            sd = _call_states([state])[3][0]   # (a term takes one state: a list in its place is refused as no state)
            od = None if op is None else _op_dims(op)
            n = sd.size - 1 if n is None else n
            if sd.size - 1 != n:
                raise ValueError("the states differ in the number of qubits")
            if od is not None and od.size - 1 != n:
                raise ValueError(f"output {j}: an operator on {od.size - 1} qubits meets a state of {n}")
            if coeff == 0:   # (NaN != 0: a NaN coefficient is data, and fails its output)
                continue
            if id(state) not in state_at:
                state_at[id(state)] = len(states)
                states.append(state)
            if op is not None and id(op) not in op_at:
                op_at[id(op)] = len(ops)
                ops.append(op)
            term_state.append(state_at[id(state)])
            term_op.append(-1 if op is None else op_at[id(op)])
            cf.append(coeff)
            chi.append(sd)
            dop.append(od)
        if len(term_state) == term_off[-1]:
            raise ValueError(f"output {j}: no term is left (an output needs a term with a coefficient that is not zero)")
        term_off.append(len(term_state))
        route = opsum_route(np.stack(chi), dop)
        if method == "fused" and route != "fused":
            raise ValueError(f"the fused route takes summed product bond dimensions up to {COMPRESS_FUSED_CAP} (output {j})")
        routes.append(method or route)
    term_off, term_state, term_op = (np.array(a, dtype=np.int32) for a in (term_off, term_state, term_op))
    cf = np.ascontiguousarray(cf, dtype=np.complex128)
    op_dims, op_off, op_data = _packed_ops(ops, n)
    count = len(outputs)
    out = (c_void_p * count)()
    ranks, sweeps = np.zeros((count, max(n - 1, 0)), dtype=np.int32), np.zeros((count, max(n - 1, 0)), dtype=np.int32)
    dropped, status = np.zeros((count, max(n - 1, 0)), dtype=np.float64), np.zeros(count, dtype=np.int32)
    with _Lanes(states) as lanes:
        check(_lib.lib().aqc_mps_opsum(lanes.handles(), len(lanes.lanes), len(ops), iptr(op_dims) if ops else None,
                                       op_off.ctypes.data_as(POINTER(ctypes.c_int64)) if ops else None, dptr(op_data) if ops else None, count,
                                       iptr(term_off), iptr(term_state), iptr(term_op), dptr(cf), trunc_thr, max_bond, code, out,
                                       iptr(ranks), dptr(dropped), iptr(sweeps), iptr(status)))
        made = _adopt(out)
    return _finish(made, status, _COMPRESS_STATUS, lambda lane: f"output {lane}, cut {_failed_cut(ranks[lane])}", False, details,
                   {"ranks": ranks, "dropped": dropped, "sweeps": sweeps, "status": status, "route": routes})


def apply_operator(op, states, trunc_thr: float = 0.0, max_bond: int = 0, *, method: Optional[str] = None, details: bool = False):
    """New states O psi, compressed: ``operator_sums`` with one term per output.  ``states``: a DeviceMPS or a QiskitMPS tuple gives a
    state, a list gives a list."""
    single = isinstance(states, (DeviceMPS, tuple))
    items = [states] if single else states
    if not isinstance(items, list) or not items:
        raise ValueError("states is a DeviceMPS, a QiskitMPS tuple or a non-empty list of those")
    if not isinstance(op, MPO):
        raise ValueError("an operator is an MPO")
    result = operator_sums([[(1.0, op, s)] for s in items], trunc_thr, max_bond, method=method, details=details)
    if not single:
        return result
    if not details:
        return result[0]
    return result[0][0], {k: v[0] for k, v in result[1].items()}


def svd(a: np.ndarray, device: Optional[int] = None):
    """(U, S, Vh, sweeps) of a complex matrix by the engine's one-sided Jacobi kernel."""
    a = np.ascontiguousarray(a, dtype=np.complex128)
    if a.ndim != 2:
        raise ValueError("expects a matrix")
    m, n = a.shape
    k = min(m, n)
    u, s, vh = np.empty((m, k), dtype=np.complex128), np.empty(k), np.empty((k, n), dtype=np.complex128)
    sweeps = c_int(0)
    check(_lib.lib().aqc_svd(_default_device() if device is None else int(device), m, n, dptr(a), dptr(u), dptr(s), dptr(vh), byref(sweeps)))
    return u, s, vh, sweeps.value


SVD_BATCH_MAX = 256   # kSvdbMaxDim of csrc/aqc_svd_blocks.h


def svd_batch(a: np.ndarray, rows=None, cols=None, device: Optional[int] = None):
    """(U, S, Vh, sweeps, status) of ``count`` complex matrices in one call (``aqc_svd_batch``: block Jacobi on the matrix cores, a
    workgroup per matrix).  ``a`` is complex128 of shape (count, m, n), m, n <= 256; matrix i is active in its leading
    ``rows[i] x cols[i]`` corner (None: all of it).  With k = min(m, n): U (count, m, k), S (count, k), Vh (count, k, n), zero outside
    the leading rows[i] x k_i, k_i, k_i x cols[i] parts.  status: 0 converged, 1 sweep limit, 2 non-finite input (outputs zero)."""
    if not isinstance(a, np.ndarray):
        raise TypeError("expects a numpy array")
    if a.dtype != np.complex128:
        raise TypeError("expects a complex128 array")
    if a.ndim != 3:
        raise ValueError("expects an array of shape (count, m, n)")
    count, m, n = a.shape
    if count < 1 or not (1 <= m <= SVD_BATCH_MAX and 1 <= n <= SVD_BATCH_MAX):
        raise ValueError(f"expects count >= 1 and 1 <= m, n <= {SVD_BATCH_MAX}")
    a = np.ascontiguousarray(a)

    def sizes(v, top, name):
        if v is None:
            return None, None
        v = np.asarray(v)
        if v.shape != (count,) or not np.issubdtype(v.dtype, np.integer):
            raise ValueError(f"{name} must hold one integer per matrix")
        if np.any(v < 1) or np.any(v > top):
            raise ValueError(f"{name} must lie in 1..{top}")
        v = np.ascontiguousarray(v, dtype=np.int32)
        return v, iptr(v)

    rows, prows = sizes(rows, m, "rows")
    cols, pcols = sizes(cols, n, "cols")
    k = min(m, n)
    u, s, vh = np.empty((count, m, k), dtype=np.complex128), np.empty((count, k)), np.empty((count, k, n), dtype=np.complex128)
    sweeps, status = np.zeros(count, dtype=np.int32), np.zeros(count, dtype=np.int32)
    check(_lib.lib().aqc_svd_batch(_default_device() if device is None else int(device), count, m, n, prows, pcols, dptr(a), dptr(u), dptr(s), dptr(vh),
                                   iptr(sweeps), iptr(status)))
    return u, s, vh, sweeps, status


# ---- circuits on MPS ------------------------------------------------------------------------------------

def _ent_matrix(entangler: str, angle: float) -> np.ndarray:
    if entangler == "cx":
        return gates.controlled(_X)
    if entangler == "cz":
        return gates.controlled(_Z)
    return gates.controlled(np.diag([1.0, np.exp(1j * angle)]))


def _blocks_of(circ):
    """(running index i, parameter block j, ctrl, targ) incl. the virtual trailing half-layer of a 2nd-order
    Trotter ansatz (parametric_circuit.py:328-333)."""
    L = circ.num_blocks
    trotter = hasattr(circ, "is_second_order")
    tail = 3 * (circ.num_qubits // 2) if (trotter and circ.is_second_order) else 0
    return trotter, [(i, i % L, int(circ.blocks[0, i % L]), int(circ.blocks[1, i % L])) for i in range(L + tail)]


class _CircuitDesc(ctypes.Structure):
    """``aqc_circuit`` of include/aqc_hip.h."""

    _fields_ = [("num_qubits", c_int32), ("entangler", c_int32), ("num_blocks", c_int32), ("trotter", c_int32),
                ("second_order", c_int32), ("blocks", POINTER(c_int32))]


def _describe(circ):
    """(aqc_circuit, keep-alive array) of a ParametricCircuit / TrotterAnsatz."""
    blocks = np.ascontiguousarray(circ.blocks, dtype=np.int32)
    trotter = hasattr(circ, "is_second_order")
    desc = _CircuitDesc(circ.num_qubits, _lib.ENTANGLERS[circ.entangler], circ.num_blocks, int(trotter),
                        int(trotter and circ.is_second_order), iptr(blocks))
    return desc, blocks


def _thetas(circ, thetas) -> np.ndarray:
    th = np.ascontiguousarray(thetas, dtype=np.float64)
    if th.shape != (circ.num_thetas,):
        raise ValueError(f"expected {circ.num_thetas} thetas, got an array of shape {th.shape}")
    return th


def _block_range(circ, block_range) -> Tuple[int, int]:
    """(block_from, block_to) as the ABI takes them; (-1, -1): all blocks."""
    if block_range is None:
        return -1, -1
    lo, hi = int(block_range[0]), int(block_range[1])
    if not 0 <= lo <= hi <= circ.num_blocks:
        raise ValueError("invalid block range")
    return lo, hi


def _apply_circuit(circ, thetas, mps: DeviceMPS, inverse: bool, trunc_thr: float, max_bond: int) -> DeviceMPS:
    """The whole ansatz in ONE ABI call (``aqc_mps_apply_circuit``)."""
    desc, keep = _describe(circ)
    th = _thetas(circ, thetas)
    check(_lib.lib().aqc_mps_apply_circuit(mps.handle, byref(desc), dptr(th), int(inverse), float(trunc_thr), int(max_bond)))
    mps.version += 1
    del keep
    return mps


def _apply_circuit_gatewise(circ, thetas, mps: DeviceMPS, inverse: bool, trunc_thr: float, max_bond: int) -> DeviceMPS:
    """The same walk with one ABI call per gate -- the cross-check of the C-side loop used by the tests."""
    n = circ.num_qubits
    th = np.asarray(thetas, dtype=np.float64)
    t1 = th[: 3 * n].reshape(n, 3)
    tpb = 5 if circ.entangler == "cp" else 4
    t2 = th[3 * n:].reshape(-1, tpb)
    rs = gates.rx_matrix if circ.entangler == "cx" else gates.rz_matrix
    trotter, blocks = _blocks_of(circ)
    if not inverse:   # core_operations.py:671-708
        for q in range(n):
            mps.gate1(gates.rz_matrix(t1[q, 0]) @ gates.ry_matrix(t1[q, 1]) @ gates.rz_matrix(t1[q, 2]), q)
        for i, j, c, t in blocks:
            b = t2[j]
            if trotter and i % 3 == 0:
                mps.gate1(gates.rz_matrix(-np.pi / 2), c)
            mps.gate2(_ent_matrix(circ.entangler, b[4] if tpb == 5 else 0.0), c, t, trunc_thr, max_bond)
            mps.gate1(gates.rz_matrix(b[1]) @ gates.ry_matrix(b[0]), c)
            mps.gate1(rs(b[3]) @ gates.ry_matrix(b[2]), t)
            if trotter and i % 3 == 2:
                mps.gate1(gates.rz_matrix(np.pi / 2), t)
    else:             # core_operations.py:787-818
        for i, j, c, t in reversed(blocks):
            b = t2[j]
            if trotter and i % 3 == 2:
                mps.gate1(gates.rz_matrix(-np.pi / 2), t)
            mps.gate1(gates.ry_matrix(-b[2]) @ rs(-b[3]), t)
            mps.gate1(gates.ry_matrix(-b[0]) @ gates.rz_matrix(-b[1]), c)
            mps.gate2(_ent_matrix(circ.entangler, -b[4] if tpb == 5 else 0.0), c, t, trunc_thr, max_bond)
            if trotter and i % 3 == 0:
                mps.gate1(gates.rz_matrix(np.pi / 2), c)
        for q in range(n):
            mps.gate1(gates.rz_matrix(-t1[q, 2]) @ gates.ry_matrix(-t1[q, 1]) @ gates.rz_matrix(-t1[q, 0]), q)
    return mps


def _fits_a_lane(num_qubits: int, max_bond: int, operands) -> bool:
    """Whether a call can start on the lockstep lanes: a register of two qubits or more, a bond cap and operands (all of the
    register's size) within ``LOCKSTEP_MAX_BOND``.  A bond that outgrows the lanes on the way is theirs to refuse (``LanesRefused``)."""
    return (num_qubits >= 2 and max_bond <= LOCKSTEP_MAX_BOND
            and all(m.num_qubits == num_qubits and int(m.bond_dims.max()) <= LOCKSTEP_MAX_BOND for m in operands))


def _one_lane(kind: str, like: DeviceMPS) -> "LockstepLanes":
    """The calling thread's single lockstep lane for ``kind`` of work, on the device and of the size of ``like`` (a lane of its own per
    host thread: the thread lanes of ``evaluate_lanes`` call in parallel)."""
    import threading

    n, dev = like.num_qubits, int(_lib.lib().aqc_mps_device(like.handle))
    return _lockstep_cached((dev, n, 1, kind, threading.get_ident()), 6, lambda: LockstepLanes(n, 1, dev))


def _apply_on_a_lane(circ, thetas, mps: DeviceMPS, inverse: bool, trunc_thr: float, max_bond: int) -> Optional[DeviceMPS]:
    """The circuit on a copy of ``mps`` through ONE lockstep lane (``LockstepLanes.apply_circuit``: the gates of a circuit layer in one
    launch, ranks decided on the device -- a 32-qubit Trotter circuit in a few milliseconds where the single-lane engine's launch chain
    takes tens); None when the state, the bond cap or a bond met on the way does not fit the lanes (bonds <= 32)."""
    if not _fits_a_lane(circ.num_qubits, max_bond, [mps]):
        return None
    ls = _one_lane("apply", mps)
    try:
        ls.set_targets(mps)
        ls.apply_circuit(circ, np.asarray(thetas, dtype=np.float64)[None, :], inverse=inverse, trunc_thr=trunc_thr, max_bond=max_bond)
        return ls.export(0)
    except LanesRefused:
        return None


def _apply_method(method: Optional[str]) -> str:
    import os

    method = os.environ.get("AQC_MPS_APPLY", "auto") if method is None else method
    if method not in ("auto", "single", "lockstep"):
        raise ValueError("method (or AQC_MPS_APPLY): 'auto', 'single' or 'lockstep'")
    return method


def _apply(circ, thetas, mps: DeviceMPS, inverse: bool, trunc_thr: float, max_bond: int, method: Optional[str]) -> DeviceMPS:
    method = _apply_method(method)
    if method != "single":
        out = _apply_on_a_lane(circ, thetas, mps, inverse, trunc_thr, max_bond)
        if out is not None:
            return out
        if method == "lockstep":
            raise LanesRefused("aqc_hip: the state or a bond on the way exceeds the lockstep lanes (bonds <= 32)")
    out = _apply_circuit(circ, thetas, mps.clone(), inverse, trunc_thr, max_bond)
    out.version = 0   # a new state, as the lanes' route hands it out
    return out


def v_mul_mps(circ, thetas, mps: DeviceMPS, trunc_thr: float = 0.0, max_bond: int = 0, method: Optional[str] = None) -> DeviceMPS:
    """V(thetas)|mps> on a copy (mps_operations.py:326-346).  ``method``: "single" -- the single-lane engine (one whole-circuit ABI
    call, any bond); "lockstep" / "auto" -- through one lockstep lane while bonds stay <= 32 ("auto" falls back to "single",
    "lockstep" raises ``LanesRefused``); None: the environment's AQC_MPS_APPLY, else "auto"."""
    return _apply(circ, thetas, mps, False, trunc_thr, max_bond, method)


def v_dagger_mul_mps(circ, thetas, mps: DeviceMPS, trunc_thr: float = 0.0, max_bond: int = 0, method: Optional[str] = None) -> DeviceMPS:
    """V(thetas)^H|mps> on a copy (mps_operations.py:349-371); ``method`` as in ``v_mul_mps``."""
    return _apply(circ, thetas, mps, True, trunc_thr, max_bond, method)


# ---- gate layers: whole programs on one or many states per call (aqc_mps_apply_gates / aqc_mps_apply_circuit_many; rules:
# csrc/aqc_mps_layers_rule.h, kernels: csrc/aqc_mps_layers.hip)

APPLY_FUSED_CAP = 64                                          # AQC_MPS_ENT_FUSED_CAP
_APPLY_METHODS = {None: 0, "fused": 1, "gatewise": 2}         # AQC_MPS_ENT_BY_RULE, AQC_MPS_ENT_FUSED, AQC_MPS_APPLY_GATEWISE
_APPLY_ROUTES = {1: "fused", 2: "gatewise"}
_APPLY_STATUS = {1: "the SVD of the gate reached its sweep limit", 2: "the state is zero or not finite",
                 3: "a rank passed the static bound of its bond"}


def apply_route(bond_dims, max_bond: int = 0) -> str:
    """The route ``apply_gates`` picks for a state with these n + 1 bond dimensions at this ``max_bond``: ``"fused"`` when no bond can
    pass ``APPLY_FUSED_CAP`` (``max_bond`` in 1 .. 64, or at most 13 qubits, and no input bond above the cap), else ``"gatewise"``."""
    d = np.ascontiguousarray(bond_dims, dtype=np.int32)
    fits = d.ndim == 1 and d.size >= 2 and int(max_bond) >= 0
    return _route_of("aqc_mps_apply_route", _APPLY_ROUTES, f"{_BOND_DIMS_OF_A_STATE} and a non-negative max_bond",
                     (d.size - 1, iptr(d), int(max_bond)) if fits else None)


def _apply_arguments(states, trunc_thr, max_bond, method):
    """What is refused before anything is uploaded; returns (trunc_thr, max_bond, the states of the call, not uploaded yet)."""
    _method_code(method, _APPLY_METHODS)
    trunc_thr, max_bond = _truncation(trunc_thr, max_bond)
    lanes = _Lanes(states)
    if method == "fused" and any(apply_route(d, max_bond) != "fused" for d in lanes.dims):
        raise ValueError(f"the fused route takes bond dimensions up to {APPLY_FUSED_CAP}: max_bond in 1 .. {APPLY_FUSED_CAP} or at most 13 qubits, "
                         f"and no input bond above {APPLY_FUSED_CAP}")
    return trunc_thr, max_bond, lanes


def _apply_results(lanes, call, plan, method, max_bond, details):
    """The outputs of one native call of the two entry points, as ``apply_gates`` returns them."""
    count = len(lanes.lanes)
    layers, ngates = int(plan[0]), int(plan[1])
    route = method
    if route is None:
        route = "fused" if all(apply_route(d, max_bond) == "fused" for d in lanes.dims) else "gatewise"
    out = (c_void_p * count)()
    ranks, sweeps = np.zeros((count, lanes.n + 1), dtype=np.int32), np.zeros((count, max(ngates, 1)), dtype=np.int32)
    dropped, status = np.zeros(count, dtype=np.float64), np.zeros((count, 3), dtype=np.int32)
    check(call(lanes.handles(), count, out, iptr(ranks), dptr(dropped), iptr(sweeps), iptr(status)))
    return _finish(_adopt(out), status[:, 0], _APPLY_STATUS, lambda lane: f"lane {lane}, layer {int(status[lane, 1])}, site {int(status[lane, 2])}",
                   lanes.single, details,
                   {"bonds": ranks, "dropped": dropped, "sweeps": sweeps[:, :ngates], "status": status[:, 0].copy(), "failed_at": status[:, 1:].copy()},
                   {"layers": layers, "route": route})


def apply_gates(states, gates, trunc_thr: float = 0.0, max_bond: int = 0, *, method: Optional[str] = None, details: bool = False):
    """New states: the program ``gates`` applied to the given ones, a whole program and one or many states per call.

    ``gates``: a list of ``(matrix, qubit)`` (2 x 2) and ``(matrix, (a, b))`` (4 x 4 on the index 2 bit_a + bit_b; any pair, routed by
    swaps as ``gate2`` routes it), applied in order.  A matrix may carry a leading axis of length ``len(states)``: the same program with
    other numbers for every state (then every matrix that is not given per state is shared, and every listing of a state is a lane of
    its own).  ``states``: a DeviceMPS, a QiskitMPS tuple (uploaded for the call) or a list of those, one qubit count; they are not
    modified.  Returns a DeviceMPS for one state, a list for a list; ``discarded_weight`` is the input's plus what the splits dropped.

    1-qubit gates are folded into neighbouring 2-qubit gates (exact), the 2-qubit gates are scheduled into layers of gates on disjoint
    sites, and every split is decided by the engine's rank rule at ``trunc_thr`` / ``max_bond``: the results are those of the loop of
    ``gate1`` / ``gate2`` calls up to rounding (at ``trunc_thr`` = 0) and up to the order in which gates of one layer meet the rule.

    ``method``: ``None`` lets the rule choose for the call (``apply_route``): ``"fused"`` keeps the working copies on the device and runs
    a layer for all states at once, the rank decisions included, with one synchronisation per call; ``"gatewise"`` (any bond) runs the
    engine's gate on a clone, folded gate by folded gate in layer order.  A lane's result does not depend on the other lanes.

    A lane whose state is zero or not finite, or whose SVD reaches its sweep limit, fails alone: without ``details`` that raises
    ``RuntimeError`` naming lane, layer and site; with ``details`` its entry is ``None`` and the second return value
    ``{"layers", "bonds", "dropped", "sweeps", "status", "failed_at", "route"}`` tells why."""
    trunc_thr, max_bond, lanes = _apply_arguments(states, trunc_thr, max_bond, method)
    if not isinstance(gates, (list, tuple)):
        raise ValueError("gates is a list of (matrix, qubit) and (matrix, (a, b))")
    count, n = len(lanes.items), lanes.n
    qubits, kinds, mats, per_state = np.zeros((len(gates), 2), dtype=np.int32), np.zeros(len(gates), dtype=np.int32), [], False
    for i, item in enumerate(gates):
        if not (isinstance(item, (list, tuple)) and len(item) == 2):
            raise ValueError(f"gate {i}: expects (matrix, qubit) or (matrix, (a, b))")
        m = np.asarray(item[0], dtype=np.complex128)
        two = not np.isscalar(item[1]) and np.ndim(item[1]) == 1
        side = 4 if two else 2
        if m.shape == (count, side, side) and m.ndim == 3:
            per_state = True
        elif m.shape != (side, side):
            raise ValueError(f"gate {i}: expects a {side} x {side} matrix, or one per state")
        if not np.all(np.isfinite(m)):
            raise ValueError(f"gate {i}: the matrix is not finite")
        qs = [int(x) for x in item[1]] if two else [int(item[1]), int(item[1])]
        if len(qs) != 2 or (two and qs[0] == qs[1]) or min(qs) < 0:
            raise ValueError(f"gate {i}: invalid qubits")
        qubits[i], kinds[i] = qs, 2 if two else 1
        mats.append(m)
    if per_state:
        mats = [m if m.ndim == 3 else np.broadcast_to(m, (count,) + m.shape) for m in mats]
        flat = np.concatenate([m.reshape(count, -1) for m in mats], axis=1) if mats else np.zeros((count, 1), dtype=np.complex128)
    else:
        flat = np.concatenate([m.ravel() for m in mats]) if mats else np.zeros(1, dtype=np.complex128)
    flat = np.ascontiguousarray(flat, dtype=np.complex128)
    if len(gates) and int(qubits.max()) >= n:
        raise ValueError("a qubit is out of range")
    with lanes:
        plan = np.zeros(2, dtype=np.int32)
        check(_lib.lib().aqc_mps_apply_plan(n, len(gates), iptr(qubits), iptr(kinds), iptr(plan), None, None))

        def call(handles, nstates, out, ranks, dropped, sweeps, status):
            return _lib.lib().aqc_mps_apply_gates(handles, nstates, len(gates), iptr(qubits), iptr(kinds), dptr(flat), int(per_state), trunc_thr, max_bond,
                                                  _APPLY_METHODS[method], out, ranks, dropped, sweeps, status)

        return _apply_results(lanes, call, plan, method, max_bond, details)


def _circuit_many(circ, thetas, states, inverse: bool, trunc_thr, max_bond, method, details):
    trunc_thr, max_bond, lanes = _apply_arguments(states, trunc_thr, max_bond, method)
    th = np.ascontiguousarray(thetas, dtype=np.float64)
    count = len(lanes.items)
    if th.shape not in ((circ.num_thetas,), (count, circ.num_thetas)):
        raise ValueError(f"expected {circ.num_thetas} thetas, or [{count}, {circ.num_thetas}], got an array of shape {th.shape}")
    if not np.all(np.isfinite(th)):
        raise ValueError("thetas must be finite")
    if lanes.n != circ.num_qubits:
        raise ValueError("circuit and states differ in the number of qubits")
    desc, keep = _describe(circ)
    with lanes:
        plan = np.zeros(2, dtype=np.int32)
        check(_lib.lib().aqc_mps_apply_circuit_plan(byref(desc), int(inverse), iptr(plan)))

        def call(handles, nstates, out, ranks, dropped, sweeps, status):
            return _lib.lib().aqc_mps_apply_circuit_many(byref(desc), dptr(th), circ.num_thetas, int(th.ndim == 2), handles, nstates, int(inverse), trunc_thr,
                                                         max_bond, _APPLY_METHODS[method], out, ranks, dropped, sweeps, status)

        result = _apply_results(lanes, call, plan, method, max_bond, details)
    del keep
    return result


def v_mul_mps_many(circ, thetas, states, trunc_thr: float = 0.0, max_bond: int = 0, *, method: Optional[str] = None, details: bool = False):
    """V(thetas)|state> for one or many states in one call, as ``apply_gates`` applies a program (``v_mul_mps`` of every state up to
    rounding and the order of a layer's decisions).  ``thetas``: 1-D (shared) or ``[states, num_thetas]``; ``method`` and ``details``
    as in ``apply_gates``."""
    return _circuit_many(circ, thetas, states, False, trunc_thr, max_bond, method, details)


def v_dagger_mul_mps_many(circ, thetas, states, trunc_thr: float = 0.0, max_bond: int = 0, *, method: Optional[str] = None, details: bool = False):
    """V(thetas)^H|state> for one or many states in one call; see ``v_mul_mps_many``."""
    return _circuit_many(circ, thetas, states, True, trunc_thr, max_bond, method, details)


# ---- dense vectors into MPS states (aqc_mps_from_vec; rules: csrc/aqc_mps_fromvec_rule.h, kernels: csrc/aqc_mps_fromvec.hip)

FROM_VECTOR_FUSED_CAP = 32                                    # AQC_MPS_FROM_VEC_CAP
_FROM_VECTOR_METHODS = {None: 0, "fused": 1, "host": 2}       # AQC_MPS_FROM_VEC_*
_FROM_VECTOR_ROUTES = {1: "fused", 2: "host"}


def from_vector_route(num_qubits: int, max_bond: int = 0) -> str:
    """The route ``from_vectors`` picks: ``"fused"`` for 2 .. 30 qubits when no bond can pass ``FROM_VECTOR_FUSED_CAP`` (``max_bond`` in
    1 .. 32, or at most 11 qubits), else ``"host"``."""
    return _route_of("aqc_mps_from_vec_route", _FROM_VECTOR_ROUTES, "expects a positive number of qubits and a non-negative max_bond",
                     (int(num_qubits), int(max_bond)))


def _from_vectors_arguments(vecs, trunc_thr, max_bond, method):
    """What is refused before any device call; returns (lanes x 2^n array, single, n, trunc_thr, max_bond, route)."""
    _method_code(method, _FROM_VECTOR_METHODS)
    trunc_thr, max_bond = _truncation(trunc_thr, max_bond)
    if isinstance(vecs, (list, tuple)):
        rows = [np.asarray(v) for v in vecs]
        if not rows or any(v.ndim != 1 for v in rows):
            raise ValueError("expects a vector of 2^n amplitudes, an array [lanes][2^n] or a list of vectors")
        if len({v.size for v in rows}) > 1:
            raise ValueError("the vectors differ in size")
        single, arr = False, np.stack(rows)
    else:
        arr = np.asarray(vecs)
        if arr.ndim not in (1, 2) or arr.size == 0:
            raise ValueError("expects a vector of 2^n amplitudes, an array [lanes][2^n] or a list of vectors")
        single, arr = arr.ndim == 1, np.atleast_2d(arr)
    if arr.dtype.kind not in "fciu":
        raise ValueError("expects numbers")
    size = int(arr.shape[1])
    n = size.bit_length() - 1
    if size != 1 << n or n < 2:
        raise ValueError(f"a vector holds 2^n amplitudes, n >= 2; got {size}")
    arr = np.array(arr, dtype=np.complex128, order="C")   # a copy: the inputs stay untouched
    route = method or from_vector_route(n, max_bond)
    if method == "fused" and from_vector_route(n, max_bond) != "fused":
        raise ValueError(f"the fused route takes 2 .. 30 qubits and bonds up to {FROM_VECTOR_FUSED_CAP}: max_bond in 1 .. {FROM_VECTOR_FUSED_CAP} "
                         f"or at most 11 qubits")
    return arr, single, n, trunc_thr, max_bond, route


def from_vectors(vecs, trunc_thr: float = 0.0, max_bond: int = 0, *, device: Optional[int] = None, method: Optional[str] = None,
                 details: bool = False):
    """New states from dense vectors: ``vecs`` is one vector of 2^n complex amplitudes (index bit q is site q), an array ``[lanes][2^n]``
    or a list of vectors of one size; any norm; they are not modified.  Returns a DeviceMPS for a 1-D input, else a list, in the
    engine's gauge as ``compress`` returns them: every bond cut left to right by the engine's rank rule at ``trunc_thr`` / ``max_bond``
    with the rescaling of a truncating gate, ``discarded_weight`` what the cuts dropped (fused route; ``details["dropped"]`` on both).

    ``method``: ``None`` lets the rule choose (``from_vector_route``).  ``"fused"`` keeps the remainder of every vector on the device: per
    site R-only Householder factors of its tall-skinny matrix, the SVD of R^T, the rank decision and the projection on the matrix
    cores, all lanes together, one synchronisation per call.  ``"host"`` is ``mps_operations.vector_to_canonical_mps`` (a loop of LAPACK
    SVDs) and an upload, vector by vector.  A lane's result does not depend on the other lanes.

    A vector that is zero or not finite, or whose SVD reaches its sweep limit, fails alone: without ``details`` that raises
    ``RuntimeError`` naming the lane and the site; with ``details`` its entry is ``None`` and the second return value
    ``{"route", "bonds", "dropped", "sweeps", "status", "failed_at", "parts"}`` tells why."""
    arr, single, n, trunc_thr, max_bond, route = _from_vectors_arguments(vecs, trunc_thr, max_bond, method)
    lanes = arr.shape[0]
    dev = _default_device() if device is None else int(device)
    bonds, sweeps = np.zeros((lanes, n + 1), dtype=np.int32), np.zeros((lanes, n - 1), dtype=np.int32)
    dropped, status = np.zeros((lanes, n - 1), dtype=np.float64), np.zeros(lanes, dtype=np.int32)
    failed_at, parts = np.full(lanes, -1, dtype=np.int32), np.ones(n - 1, dtype=np.int32)
    if route == "fused":
        out = (c_void_p * lanes)()
        check(_lib.lib().aqc_mps_from_vec(dev, n, lanes, dptr(arr), trunc_thr, max_bond, _FROM_VECTOR_METHODS[method], out, iptr(bonds), dptr(dropped),
                                          iptr(sweeps), iptr(status), iptr(failed_at), iptr(parts)))
        made = _adopt(out)
    else:
        from .mps_operations import _canonical_sweep

        made = []
        for i in range(lanes):
            if not np.all(np.isfinite(arr[i])) or not np.any(arr[i]):
                status[i], failed_at[i] = 2, 0
                bonds[i, 0] = 1
                made.append(None)
                continue
            gam, lam, weights = _canonical_sweep(arr[i], trunc_thr, max_bond)
            made.append(DeviceMPS.from_qiskit((gam, lam), dev, assume_canonical=True))
            bonds[i] = [1] + [v.size for v in lam] + [1]
            dropped[i] = weights
    return _finish(made, status, _COMPRESS_STATUS, lambda lane: f"lane {lane}, site {int(failed_at[lane])}", single, details,
                   {"bonds": bonds, "dropped": dropped, "sweeps": sweeps, "status": status, "failed_at": failed_at}, {"route": route, "parts": parts})


# ---- MPS states into dense vectors and blocks of amplitudes (aqc_mps_to_vec, aqc_mps_amp_blocks; rules: csrc/aqc_mps_tovec_rule.h, kernels:
# csrc/aqc_mps_tovec.hip)

TO_VECTOR_FUSED_CAP = 64                                      # the planes of the fused route
TO_VECTOR_MAX_QUBITS = 30
AMPLITUDE_BLOCK_MAX_LOW = 24
_TO_VECTOR_METHODS = {None: 0, "fused": 1, "gemm": 2}         # AQC_MPS_TO_VEC_*
_TO_VECTOR_ROUTES = {1: "fused", 2: "gemm"}
_AMPLITUDE_BLOCK_METHODS = {None: 0, "fused": 1}


def to_vector_route(bond_dims) -> str:
    """The route ``to_vectors`` picks for a state with these n + 1 bond dimensions: ``"fused"`` when every bond is at most
    ``TO_VECTOR_FUSED_CAP``, else ``"gemm"``.  Host only."""
    d = np.ascontiguousarray(bond_dims, dtype=np.int32)
    return _route_of("aqc_mps_to_vec_route", _TO_VECTOR_ROUTES, _BOND_DIMS_OF_A_STATE, (d.size - 1, iptr(d)) if d.ndim == 1 and d.size >= 2 else None)


def to_vectors(states, *, method: Optional[str] = None, out: Optional[np.ndarray] = None, details: bool = False):
    """The dense vectors of one or many states in one call, the inverse of ``from_vectors``: ``states`` is a DeviceMPS or a list of them
    (one qubit count, 1 <= n <= 30, one device; any gauge, any norm; they are not modified).  Returns complex128 ``[2^n]`` for a single
    state, else ``[states][2^n]``, index bit q being site q.  ``out``: a C-contiguous complex128 array of exactly that shape, filled and
    returned.  A state listed twice is contracted once and delivered twice; a lane's result does not depend on the other states.

    ``method``: ``None`` lets the rule choose per state (``to_vector_route``).  ``"fused"`` (bonds up to ``TO_VECTOR_FUSED_CAP``) grows the
    two halves of every state site by site on the matrix cores, all states in every launch, and writes the amplitudes in one pass;
    ``"gemm"`` (any bond) runs the chain of batched products of the workspace's ``mps_to_vec`` on the states' own tensors.  The states go
    in chunks under a budget of device memory (``aqc_mps_to_vec_budget``), one synchronisation and one download per chunk.

    ``details``: also returns ``{"route", "split", "chunks", "launches"}``, ``route`` per state."""
    code = _method_code(method, _TO_VECTOR_METHODS)
    single, items, n, dims = _call_states(states, device_only=True)
    if n > TO_VECTOR_MAX_QUBITS:
        raise ValueError(f"a dense vector takes at most {TO_VECTOR_MAX_QUBITS} qubits, the states have {n}: amplitude_blocks reads blocks of it")
    if method == "fused":
        for i, d in enumerate(dims):
            if int(d.max()) > TO_VECTOR_FUSED_CAP:
                raise ValueError(f"the fused route takes bond dimensions up to {TO_VECTOR_FUSED_CAP}; state {i} has {int(d.max())}")
    shape = (1 << n,) if single else (len(items), 1 << n)
    if out is not None:
        if not isinstance(out, np.ndarray) or out.dtype != np.complex128 or out.shape != shape or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError(f"out must be a writeable C-contiguous complex128 array of shape {shape}")
    else:
        out = np.empty(shape, dtype=np.complex128)
    count = len(items)
    info = np.zeros(count + 3, dtype=np.int32)
    check(_lib.lib().aqc_mps_to_vec(_handles(items), count, code, dptr(out), iptr(info)))
    if not details:
        return out
    routes = [_TO_VECTOR_ROUTES[int(r)] for r in info[:count]]
    return out, {"route": routes[0] if single else routes, "split": int(info[count]), "chunks": int(info[count + 1]), "launches": int(info[count + 2])}


def amplitude_blocks(states, low_qubits: int, high_bits, *, method: Optional[str] = None) -> np.ndarray:
    """Blocks of amplitudes that share their high bits, at any n >= 2: ``high_bits`` is ``[rows][n - low_qubits]`` of 0 / 1, row r holding
    the bits of the sites low_qubits .. n - 1 (the shape convention of ``mps_sampling.amplitudes``), shared by the states.  Returns
    complex128 ``[rows][2^low_qubits]`` for a single state, else ``[states][rows][2^low_qubits]``: entry l of row r is psi at index
    l + 2^low_qubits (sum_i high_bits[r][i] 2^i).  1 <= low_qubits <= min(n - 1, 24).  A block costs one walk of the high sites
    plus one product, where ``amplitudes`` walks the chain once per number.  Fused route only (``method`` None or ``"fused"``): a bond
    above ``TO_VECTOR_FUSED_CAP`` is refused."""
    code = _method_code(method, _AMPLITUDE_BLOCK_METHODS)
    single, items, n, dims = _call_states(states, device_only=True)
    k = int(low_qubits)
    if n < 2 or k < 1 or k > min(n - 1, AMPLITUDE_BLOCK_MAX_LOW):
        raise ValueError(f"low_qubits must be in 1 .. min(n - 1, {AMPLITUDE_BLOCK_MAX_LOW}) at n >= 2; got {low_qubits} at n = {n}")
    arr = np.asarray(high_bits)
    if arr.ndim != 2 or arr.shape[0] < 1 or not (np.issubdtype(arr.dtype, np.integer) or arr.dtype == np.bool_):
        raise ValueError("high_bits is a non-empty [rows][n - low_qubits] array of bits")
    if arr.shape[1] != n - k:
        raise ValueError(f"a row of high_bits has {arr.shape[1]} bits, the states have {n - k} sites above the low ones")
    if arr.min() < 0 or arr.max() > 1:
        raise ValueError("a bit is 0 or 1")
    for i, d in enumerate(dims):
        if int(d.max()) > TO_VECTOR_FUSED_CAP:
            raise ValueError(f"blocks of amplitudes take bond dimensions up to {TO_VECTOR_FUSED_CAP}; state {i} has a bond of {int(d.max())}")
    arr = np.ascontiguousarray(arr, dtype=np.uint8)
    count, rows = len(items), arr.shape[0]
    out = np.empty((count, rows, 1 << k), dtype=np.complex128)
    check(_lib.lib().aqc_mps_amp_blocks(_handles(items), count, k, rows, arr.ctypes.data_as(POINTER(ctypes.c_uint8)), code, dptr(out)))
    return out[0] if single else out


def fast_dot_gradient_mps(circ, thetas, lvec: DeviceMPS, vh_phi: DeviceMPS, *, trunc_thr: float = 0.0, max_bond: int = 0,
                          block_range: Optional[Tuple[int, int]] = None, front_layer: bool = True, method: Optional[str] = None) -> np.ndarray:
    """Complex gradient of <V lvec|phi> given vh_phi = V^H|phi>, gate by gate on two MPS
    (mps_dot_objective.py:41-242): w <- lvec, z <- vh_phi; every gate is applied to both and each parametrised
    rotation records 0.5j <P w|z>; the CPhase derivative is -1j <P11 w|z> taken before the gate.
    ONE ABI call: the walk, the cached environments behind the inner products and the single download of all of them live on the
    C side -- on one lockstep lane (``aqc_mpsb_gradient_of``) while bonds stay <= 32, on the single-lane engine
    (``aqc_mps_fast_dot_gradient``) otherwise; ``method`` as in ``v_mul_mps``."""
    desc, keep = _describe(circ)
    th = _thetas(circ, thetas)
    lo, hi = _block_range(circ, block_range)
    grad = np.zeros(circ.num_thetas, dtype=np.complex128)
    method = _apply_method(method)
    if method != "single" and _fits_a_lane(circ.num_qubits, max_bond, [lvec, vh_phi]):
        ls = _one_lane("gradient", vh_phi)   # one lockstep lane: the walk is a chain of fused steps instead of ~10 launches per gate
        try:
            ls.set_targets(vh_phi).set_lhs(lvec)
            check(_lib.lib().aqc_mpsb_gradient_of(ls.handle, byref(desc), dptr(th), float(trunc_thr), int(max_bond), lo, hi, int(bool(front_layer)),
                                                  dptr(grad)))
            del keep
            return grad
        except LanesRefused:
            if method == "lockstep":
                raise
    elif method == "lockstep":
        raise LanesRefused("aqc_hip: the operands exceed the lockstep lanes (bonds <= 32)")
    check(_lib.lib().aqc_mps_fast_dot_gradient(byref(desc), lvec.handle, vh_phi.handle, dptr(th), float(trunc_thr), int(max_bond),
                                               lo, hi, int(bool(front_layer)), dptr(grad)))
    del keep
    return grad


def fast_dot_gradient_mps_gatewise(circ, thetas, lvec: DeviceMPS, vh_phi: DeviceMPS, *, trunc_thr: float = 0.0, max_bond: int = 0,
                                   block_range: Optional[Tuple[int, int]] = None, front_layer: bool = True) -> np.ndarray:
    """The same sweep with one ABI call per gate and one full transfer-matrix chain per inner product -- the
    cross-check of the C-side walk used by the tests."""
    n = circ.num_qubits
    th = np.asarray(thetas, dtype=np.float64)
    tpb = 5 if circ.entangler == "cp" else 4
    L = circ.num_blocks
    lo, hi = (0, L) if block_range is None else (int(block_range[0]), int(block_range[1]))
    grad = np.zeros(circ.num_thetas, dtype=np.complex128)
    g1 = grad[: 3 * n].reshape(n, 3)
    g2 = grad[3 * n:].reshape(-1, tpb)
    t1 = th[: 3 * n].reshape(n, 3)
    t2 = th[3 * n:].reshape(-1, tpb)
    w, z = lvec.clone(), vh_phi.clone()
    pauli = {"x": _X, "y": _Y, "z": _Z}

    def both(gate, q):
        w.gate1(gate, q)
        z.gate1(gate, q)

    def dot(p: str, q: int) -> np.complex128:   # 0.5j <P w|z>, P folded into the transfer-matrix chain
        return 0.5j * w.dot_ops(z, [(q, pauli[p])])

    for q in range(n):   # front layer: Rz(t2), Ry(t1), Rz(t0), rightmost first (core_operations.py:921-935)
        for slot, mat, p in ((2, gates.rz_matrix, "z"), (1, gates.ry_matrix, "y"), (0, gates.rz_matrix, "z")):
            both(mat(t1[q, slot]), q)
            if front_layer:
                g1[q, slot] = dot(p, q)
    rs, ps = (gates.rx_matrix, "x") if circ.entangler == "cx" else (gates.rz_matrix, "z")
    trotter, blocks = _blocks_of(circ)
    for i, j, c, t in blocks:
        b = t2[j]
        live = lo <= j < hi
        if trotter and i % 3 == 0:
            both(gates.rz_matrix(-np.pi / 2), c)
        if live and tpb == 5:    # -1j <P11 w|z> before the gate (core_op_matrix.py:430-477)
            g2[j, 4] += -1j * w.dot_ops(z, [(c, _P1), (t, _P1)])
        ent = _ent_matrix(circ.entangler, b[4] if tpb == 5 else 0.0)
        z.gate2(ent, c, t, trunc_thr, max_bond)
        w.gate2(ent, c, t, trunc_thr, max_bond)
        for slot, mat, p, q in ((0, gates.ry_matrix, "y", c), (1, gates.rz_matrix, "z", c), (2, gates.ry_matrix, "y", t), (3, rs, ps, t)):
            both(mat(b[slot]), q)
            if live:
                g2[j, slot] += dot(p, q)
        if trotter and i % 3 == 2:
            both(gates.rz_matrix(np.pi / 2), t)
    w.close()
    z.close()
    return grad


# ---- lanes beyond dense reach ---------------------------------------------------------------------------------------
# Every DeviceMPS owns its stream and every circuit / gradient walk is ONE native call that releases the GIL, so independent
# problems (the seeds / restarts of a horizon, mps_dot_objective.py:41 called once per job in the reference, job_executor.py:141)
# run as lanes on host threads: the walks are chains of small dependent launches with one host decision (the truncation rank) per
# 2-qubit gate, i.e. latency-bound -- concurrent lanes fill the device while one lane waits.

_POOL = None


def _pool(workers: int):
    global _POOL
    from concurrent.futures import ThreadPoolExecutor

    if _POOL is None or _POOL._max_workers < workers:
        if _POOL is not None:
            _POOL.shutdown(wait=True)
        _POOL = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="aqc-mps-lane")
    return _POOL


LOCKSTEP_MAX_BOND = 32   # kLaneCap of csrc/aqc_launch.h


class LockstepLanes:
    """``lanes`` problems on one ansatz evaluated together and device-resident (C ABI ``aqc_mpsb_*``): every step of the gate walk of
    ``mps_dot_objective.fast_dot_gradient`` (:41-242) is one launch for all lanes; a truncated 2-qubit gate is one workgroup per lane
    (two-site tensor, SVD, rank decision, new tensors), the lane's bond dimensions never leave the device and the host enqueues a
    whole evaluation without waiting.  Bonds up to ``LOCKSTEP_MAX_BOND`` per lane; a lane that would grow beyond makes ``evaluate``
    raise (nothing is truncated silently) and ``evaluate_lanes`` repeats the batch lane by lane on the single-lane engine."""

    def __init__(self, num_qubits: int, lanes: int, device: Optional[int] = None):
        h = c_void_p()
        check(_lib.lib().aqc_mpsb_create(_default_device() if device is None else int(device), int(num_qubits), int(lanes), byref(h)))
        self.handle, self.num_qubits, self.lanes = h, int(num_qubits), int(lanes)
        self._targets = self._lhs = self._bank = None

    def gate2_stats(self, enable: Optional[bool] = None, reset: bool = False) -> dict:
        """Work and time of the truncated 2-qubit gates (``aqc_mpsb_gate2_stats``): fp64 flops of the Jacobi rotations that ran, SVDs,
        sweeps, rotations; ``lanes_gate2`` launches timed and their total duration while ``enable`` is on."""
        out = np.zeros(6)
        check(_lib.lib().aqc_mpsb_gate2_stats(self.handle, -1 if enable is None else int(bool(enable)), dptr(out), int(bool(reset))))
        return {"jacobi_flops": float(out[0]), "svds": int(out[1]), "sweeps": int(out[2]), "rotations": int(out[3]),
                "launches_timed": int(out[4]), "launch_ms": float(out[5])}

    def _handles(self, states):
        lst = list(states) if isinstance(states, (list, tuple)) else [states]
        if len(lst) not in (1, self.lanes):
            raise ValueError("one state per lane, or one for all lanes")
        arr = (c_void_p * len(lst))(*[m.handle for m in lst])
        return lst, arr, int(len(lst) == 1)

    def _load(self, slot: str, states, load) -> "LockstepLanes":
        """``load()`` copies ``states`` into the lanes -- unless they hold exactly these states, unchanged since (``DeviceMPS.version``):
        the batches of an optimisation come back every iteration.  The stamp remembered in ``slot`` holds no reference to the states (a
        closed one is not kept alive by its copy), and is dropped before the copy so that a failed one is never taken for the old."""
        stamp = [(m.serial, m.version) for m in states]
        if getattr(self, slot) != stamp:
            setattr(self, slot, None)
            load()
            setattr(self, slot, stamp)
        return self

    def set_targets(self, targets) -> "LockstepLanes":
        """Copies |phi_l> of every lane into the lanes (one state per lane, or one for all).  A call with the very states of the
        previous one, unchanged since, is free.  (``_load`` forgets the remembered states before it copies: after a failed copy the
        lanes hold neither the old nor the new ones, and the next call copies again.)"""
        lst, arr, shared = self._handles(targets)
        return self._load("_targets", lst, lambda: check(_lib.lib().aqc_mpsb_set_targets(self.handle, arr, shared)))

    def set_lhs(self, lhs) -> "LockstepLanes":
        """The same for the left-hand states <lhs_l| (a failed copy is forgotten in the same way)."""
        lst, arr, shared = self._handles(lhs)
        return self._load("_lhs", lst, lambda: check(_lib.lib().aqc_mpsb_set_lhs(self.handle, arr, shared)))

    def _call(self, circ, thetas=None, block_range=None) -> SimpleNamespace:
        """What the calls below hand to the ABI.  Always: ``circ`` (pointer to the descriptor ``desc``, whose block array ``keep``
        lives as long as the returned object) and the block range ``lo``, ``hi``.  With ``thetas`` (every call but ``gradient``):
        ``th``, checked against (lanes, num_thetas) and the lanes' size, and the per-lane outputs such a call fills -- ``disc``
        (discarded weight), ``bonds`` (largest bond of the working state), ``details`` (their two pointers)."""
        c = SimpleNamespace()
        if thetas is not None:
            th = np.ascontiguousarray(thetas, dtype=np.float64)
            if th.shape != (self.lanes, circ.num_thetas):
                raise ValueError("thetas: expects shape (lanes, circ.num_thetas)")
            if circ.num_qubits != self.num_qubits:
                raise ValueError("circuit and lanes differ in the number of qubits")
            c.th = th
            c.disc = np.zeros(self.lanes, dtype=np.float64)
            c.bonds = np.zeros(self.lanes, dtype=np.int32)
            c.details = (dptr(c.disc), iptr(c.bonds))
        c.desc, c.keep = _describe(circ)
        c.circ = byref(c.desc)
        c.lo, c.hi = _block_range(circ, block_range)
        return c

    def evaluate(self, circ, thetas, *, trunc_thr: float = 0.0, max_bond: int = 0, block_range: Optional[Tuple[int, int]] = None,
                 front_layer: bool = True, details: bool = False):
        """(h[lanes], grads[lanes][T]) -- per lane the values of ``v_dagger_mul_mps`` + ``dot`` + ``fast_dot_gradient_mps``;
        with ``details`` also (discarded weight, largest bond) of every lane's V^H|target>."""
        c = self._call(circ, thetas, block_range)
        h = np.zeros(self.lanes, dtype=np.complex128)
        grads = np.zeros((self.lanes, circ.num_thetas), dtype=np.complex128)
        check(_lib.lib().aqc_mpsb_eval(self.handle, c.circ, dptr(c.th), float(trunc_thr), int(max_bond), c.lo, c.hi, int(bool(front_layer)),
                                       dptr(h), dptr(grads), *c.details))
        return (h, grads, c.disc, c.bonds) if details else (h, grads)

    def set_lhs_basis(self, bits) -> "LockstepLanes":
        """lhs state of every lane = the computational-basis state ``bits[lane][qubit]`` (0 / 1), built on the device."""
        arr = np.ascontiguousarray(bits, dtype=np.uint8)
        if arr.shape != (self.lanes, self.num_qubits):
            raise ValueError("bits: expects shape (lanes, num_qubits)")
        check(_lib.lib().aqc_mpsb_set_lhs_basis(self.handle, arr.ctypes.data_as(POINTER(ctypes.c_uint8))))
        self._lhs = None
        return self

    def apply_vh(self, circ, thetas, *, trunc_thr: float = 0.0, max_bond: int = 0, flips: bool = False, half: bool = False, details: bool = False):
        """Phase 1 of ``evaluate``: vh_l = V(thetas[l])^H|target_l> stays in the lanes; returns amps[lanes][1 (+ n)] with
        amps[l][0] = <lhs_l|vh_l> and, with ``flips``, amps[l][1 + q] = <X_q lhs_l|vh_l>.  ``half``: lanes [lanes/2, lanes) repeat targets
        and thetas of the first half -- V^H runs once for both.  ``gradient`` continues from here."""
        c = self._call(circ, thetas)
        na = 1 + self.num_qubits if flips else 1
        amps = np.zeros((self.lanes, na), dtype=np.complex128)
        check(_lib.lib().aqc_mpsb_vh(self.handle, c.circ, dptr(c.th), float(trunc_thr), int(max_bond), int(bool(half)), na, dptr(amps), *c.details))
        return (amps, c.disc, c.bonds) if details else amps

    def set_bank(self, states) -> "LockstepLanes":
        """A bank of K lhs states shared by all lanes (``aqc_mpsb_set_bank``; bonds <= 32): the states S|0>, S X_i|0> of a general
        state preparation, whose amplitudes ``apply_vh_bank`` returns.  Unchanged states since the last call are not copied again."""
        lst = list(states)   # (the count is the library's to refuse: 1 .. 32767)
        return self._load("_bank", lst, lambda: check(_lib.lib().aqc_mpsb_set_bank(self.handle, (c_void_p * len(lst))(*[m.handle for m in lst]), len(lst))))

    def apply_vh_bank(self, circ, thetas, *, trunc_thr: float = 0.0, max_bond: int = 0, half: bool = False, details: bool = False):
        """``apply_vh`` with the bank as the lhs side: vh_l = V(thetas[l])^H|target_l> stays in the lanes; returns amps[lanes][K] with
        amps[l][k] = <bank_k|vh_l> (all K x lanes overlaps in one launch, read back with V^H's results).  ``gradient`` continues from
        here with whatever lhs states are set then."""
        if not self._bank:
            raise RuntimeError("aqc_hip: set the bank of the lanes first (set_bank)")
        c = self._call(circ, thetas)
        na = len(self._bank)
        amps = np.zeros((self.lanes, na), dtype=np.complex128)
        check(_lib.lib().aqc_mpsb_vh_bank(self.handle, c.circ, dptr(c.th), float(trunc_thr), int(max_bond), int(bool(half)), na, dptr(amps), *c.details))
        return (amps, c.disc, c.bonds) if details else amps

    def apply_circuit(self, circ, thetas, *, inverse: bool = False, trunc_thr: float = 0.0, max_bond: int = 0, details: bool = False):
        """The lanes' working state <- V(thetas[l])|target_l> (or V^H with ``inverse``): ``v_mul_mps`` / ``v_dagger_mul_mps`` for every lane,
        the gates of a circuit layer in one launch.  ``export(lane)`` hands a result out; no lhs states needed."""
        c = self._call(circ, thetas)
        check(_lib.lib().aqc_mpsb_apply_circuit(self.handle, c.circ, dptr(c.th), int(bool(inverse)), float(trunc_thr), int(max_bond), *c.details))
        return (c.disc, c.bonds) if details else None

    def export(self, lane: int) -> DeviceMPS:
        """Lane ``lane`` of the working state (after ``apply_circuit`` / ``apply_vh``) as a ``DeviceMPS`` of its own."""
        h = c_void_p()
        check(_lib.lib().aqc_mpsb_export(self.handle, int(lane), byref(h)))
        return DeviceMPS(h)

    def gradient(self, circ, *, block_range: Optional[Tuple[int, int]] = None, front_layer: bool = True) -> np.ndarray:
        """Phase 2: grads[lanes][T] (complex) of <V lhs_l|target_l> from the CURRENT lhs states and the vh of ``apply_vh``."""
        c = self._call(circ, None, block_range)
        grads = np.zeros((self.lanes, circ.num_thetas), dtype=np.complex128)
        check(_lib.lib().aqc_mpsb_grad(self.handle, c.circ, c.lo, c.hi, int(bool(front_layer)), dptr(grads)))
        return grads

    def close(self) -> None:
        if getattr(self, "handle", None):
            _lib.lib().aqc_mpsb_destroy(self.handle)
            self.handle = None
            self._targets = self._lhs = self._bank = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_LOCKSTEP_CACHE: dict = {}   # (device, qubits, lanes) -> LockstepLanes; the batches of a running optimisation come back every iteration
_LOCKSTEP_LOCK = __import__("threading").Lock()


def _lockstep_cached(key, cap: int, make):
    """Look up / create an entry of the shared cache under its lock (the host-thread lanes of ``evaluate_lanes`` arrive here
    together); the evicted object is freed when its last user lets go of it."""
    with _LOCKSTEP_LOCK:
        ls = _LOCKSTEP_CACHE.get(key)
        if ls is None:
            while len(_LOCKSTEP_CACHE) >= cap:
                _LOCKSTEP_CACHE.pop(next(iter(_LOCKSTEP_CACHE)), None)
            ls = _LOCKSTEP_CACHE[key] = make()
        return ls


def _lockstep_for(num_qubits: int, lanes: int, device: int, targets, lhs) -> LockstepLanes:
    key = (device, num_qubits, lanes)
    ls = _lockstep_cached(key, 4, lambda: LockstepLanes(num_qubits, lanes, device))
    # the operands are copied into the lanes; the copies are refreshed when a state was replaced or edited in place (DeviceMPS.version)
    ls.set_targets(targets)
    ls.set_lhs(lhs)
    return ls


def evaluate_lanes(circ, thetas: np.ndarray, targets, lhs, *, trunc_thr: float = 0.0, max_bond: int = 0,
                   block_range: Optional[Tuple[int, int]] = None, front_layer: bool = True, workers: int = 0, method: str = "auto"):
    """One objective+gradient evaluation per lane on the native engine: lane b computes vh_b = V(thetas[b])^H |targets[b]>
    (v_dagger_mul_mps), h_b = <lhs[b]|vh_b> and the complex gradient of <V lhs[b]|targets[b]> (fast_dot_gradient_mps).
    ``targets`` / ``lhs``: one DeviceMPS per lane, or a single one shared by all lanes (operands are only read).
    ``method``: "lockstep" -- all lanes walk the circuit together, one launch per step (``LockstepLanes``; bonds <= 32);
    "threads" -- every lane on the single-lane engine, lanes concurrently on ``workers`` host threads (default: one per lane, at most
    16); "auto" -- lockstep when the operands' bonds allow it (also for one lane), and the thread lanes if a lane outgrows the lockstep bond.
    Returns (h[B] complex, grads[B][T] complex)."""
    th = np.ascontiguousarray(thetas, dtype=np.float64)
    if th.ndim != 2 or th.shape[1] != circ.num_thetas:
        raise ValueError("thetas: expects shape (lanes, circ.num_thetas)")
    if method not in ("auto", "lockstep", "threads"):
        raise ValueError("method: 'auto', 'lockstep' or 'threads'")
    lanes = th.shape[0]
    tg = list(targets) if isinstance(targets, (list, tuple)) else [targets] * lanes
    lh = list(lhs) if isinstance(lhs, (list, tuple)) else [lhs] * lanes
    if len(tg) != lanes or len(lh) != lanes:
        raise ValueError("one target and one lhs state per lane (or one for all)")

    if method != "threads":   # (a single lane as well: its walk is 5x shorter on the lockstep kernels than on the single-lane engine's launch chain)
        distinct = list({id(m): m for m in tg + lh}.values())
        if _fits_a_lane(circ.num_qubits, max_bond, distinct) or method == "lockstep":
            try:
                shared_t = targets if not isinstance(targets, (list, tuple)) else tg
                shared_l = lhs if not isinstance(lhs, (list, tuple)) else lh
                devs = {int(_lib.lib().aqc_mps_device(m.handle)) for m in distinct}   # the lanes live where the operands live
                if len(devs) != 1:
                    raise ValueError(f"the operands of evaluate_lanes live on different devices: {sorted(devs)}")
                ls = _lockstep_for(circ.num_qubits, lanes, devs.pop(), shared_t, shared_l)
                return ls.evaluate(circ, th, trunc_thr=trunc_thr, max_bond=max_bond, block_range=block_range, front_layer=front_layer)
            except LanesRefused:
                if method == "lockstep":
                    raise

    def one(b: int):
        vh = v_dagger_mul_mps(circ, th[b], tg[b], trunc_thr=trunc_thr, max_bond=max_bond, method="single")
        try:
            h = np.conj(vh.dot(lh[b]))   # <lhs|vh> on vh's own scratch and stream: an lhs state shared by the lanes is only read
            g = fast_dot_gradient_mps(circ, th[b], lh[b], vh, trunc_thr=trunc_thr, max_bond=max_bond, block_range=block_range,
                                      front_layer=front_layer, method="single")
        finally:
            vh.close()
        return h, g

    nw = min(lanes, workers if workers > 0 else 16)
    res = [one(0)] if lanes == 1 else list(_pool(nw).map(one, range(lanes)))
    return np.array([r[0] for r in res], dtype=np.complex128), np.stack([r[1] for r in res])
