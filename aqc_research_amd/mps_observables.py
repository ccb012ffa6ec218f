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

Operators on more than two sites, and anything between two different states, are Pauli strings (aqc_mps_pauli; kernels:
csrc/aqc_mps_pauli.hip, rules: csrc/aqc_mps_pauli_rule.h): ``pauli_strings`` gives <phi|P|psi> for many strings and pairs of states in
one call, ``overlaps`` the matrix <phi_a|psi_b>, ``energy`` a weighted sum of expectation values.

Entanglement across the cuts of the chain (aqc_mps_ent_schmidt; kernels: csrc/aqc_mps_ent.hip, rules: csrc/aqc_mps_ent_rule.h):
``schmidt_values`` gives the singular values of every cut of one or many states per call, ``entanglement_entropies`` their entropies
(``entropies_of``: NumPy), ``bond_dims_needed`` the bond dimensions the engine's rank rule would keep at a given ``trunc_thr`` /
``max_bond``.
"""
from ctypes import POINTER, c_uint8, c_void_p
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

    def handles(self):
        """The lanes as the handle array that the native calls take."""
        return (c_void_p * len(self.lanes))(*[m.handle for m in self.lanes])

    def check_fused_cap(self, method, cap: int = FUSED_CAP) -> None:
        """Refuses ``method="fused"`` for a lane beyond the cap, before the native call."""
        if method == "fused":
            for m in self.lanes:
                if int(m.bond_dims.max()) > cap:
                    raise ValueError(f"the fused route takes bond dimensions up to {cap}, not {int(m.bond_dims.max())}")


def _rdms(lanes: _Lanes, arr: np.ndarray, method: Optional[str]) -> np.ndarray:
    if method not in _METHODS:
        raise ValueError(f"method must be None, 'fused' or 'gemm', not {method!r}")
    lanes.check_fused_cap(method)
    out = np.empty((len(lanes.lanes), arr.shape[0], 4, 4), dtype=np.complex128)
    check(_lib.lib().aqc_mps_obs_pairs(lanes.handles(), len(lanes.lanes), arr.shape[0], iptr(arr), _METHODS[method], dptr(out)))
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


# ---- Pauli strings: <phi|P|psi> for many strings and pairs of states per call (aqc_mps_pauli; rules: csrc/aqc_mps_pauli_rule.h)

_PAULI_METHODS = {None: 0, "fused": 1, "gemm": 2}   # AQC_MPS_PAULI_*
_LETTERS = {"I": 0, "X": 1, "Y": 2, "Z": 3}


def pauli_route(bra_dims, ket_dims) -> str:
    """The route the rule picks for a pair with these n + 1 bond dimensions each (``bra_dims`` None: the ket's): ``"fused"`` when every
    bond of both is at most ``FUSED_CAP``, else ``"gemm"``."""
    k = np.ascontiguousarray(ket_dims, dtype=np.int32)
    b = None if bra_dims is None else np.ascontiguousarray(bra_dims, dtype=np.int32)
    if k.ndim != 1 or k.size < 2 or (b is not None and b.shape != k.shape):
        raise ValueError("expects the n + 1 bond dimensions of the bra and of the ket")
    r = _lib.lib().aqc_mps_pauli_route(k.size - 1, None if b is None else iptr(b), iptr(k))
    if r not in (1, 2):
        raise ValueError("expects the n + 1 bond dimensions of the bra and of the ket")
    return "fused" if r == 1 else "gemm"


def _shape_of(states):
    """``(single, count, n)`` of what ``_Lanes`` would take, read on the host: no upload is made for a call that is then refused."""
    single = isinstance(states, DeviceMPS) or _is_tuple_state(states)
    if not single and not isinstance(states, list):
        raise ValueError("states is a DeviceMPS, a QiskitMPS tuple or a list of those")
    items = [states] if single else states
    if not items:
        raise ValueError("expects at least one state")
    ns = set()
    for s in items:
        if isinstance(s, DeviceMPS):
            if not s.handle:
                raise ValueError("a closed DeviceMPS")
            ns.add(s.num_qubits)
        elif _is_tuple_state(s):
            ns.add(len(s[0]))
        else:
            raise ValueError("a state is a DeviceMPS or a QiskitMPS tuple")
    if len(ns) != 1:
        raise ValueError("the states differ in the number of qubits")
    return single, len(items), ns.pop()


def _strings(strings, n: int) -> np.ndarray:
    """uint8 (S, n) of 0, 1, 2, 3 = I, X, Y, Z from an array, a list of ``str`` of length n or a list of sparse ``(letters, qubits)``."""
    if isinstance(strings, np.ndarray):
        arr = strings
        if arr.ndim != 2 or arr.shape[0] < 1 or arr.shape[1] != n or not np.issubdtype(arr.dtype, np.integer):
            raise ValueError(f"expects a non-empty (S, {n}) array of letters 0, 1, 2, 3")
        if arr.min() < 0 or arr.max() > 3:
            raise ValueError("a letter is 0, 1, 2 or 3 (I, X, Y, Z)")
        return np.ascontiguousarray(arr, dtype=np.uint8)
    if not isinstance(strings, (list, tuple)) or len(strings) < 1:
        raise ValueError("expects a non-empty list of Pauli strings")
    arr = np.zeros((len(strings), n), dtype=np.uint8)
    for k, s in enumerate(strings):
        if isinstance(s, str):
            if len(s) != n:
                raise ValueError(f"string {k} has {len(s)} letters for {n} qubits")
            letters, qubits = s, range(n)
        elif isinstance(s, tuple) and len(s) == 2 and isinstance(s[0], str):
            letters, qubits = s[0], tuple(s[1])
            if len(letters) != len(qubits) or len(set(qubits)) != len(qubits):
                raise ValueError(f"string {k}: one letter per listed qubit, every qubit once")
        else:
            raise ValueError(f"string {k} is neither a str over IXYZ nor a (letters, qubits) tuple")
        for ch, q in zip(letters, qubits):
            if ch not in _LETTERS:
                raise ValueError(f"string {k}: {ch!r} is no letter out of IXYZ")
            if not (isinstance(q, (int, np.integer)) and 0 <= q < n):
                raise ValueError(f"string {k}: qubit out of range: {n} qubits")
            arr[k, q] = _LETTERS[ch]
    return arr


def _pauli_call(bras, kets, arr: np.ndarray, method: Optional[str]) -> np.ndarray:
    """``(len(kets), S)``: <bras[p]| P_s |kets[p]> (``bras`` None: expectation mode) for lists of open DeviceMPS."""
    if method not in _PAULI_METHODS:
        raise ValueError(f"method must be None, 'fused' or 'gemm', not {method!r}")
    if method == "fused":
        for m in {id(m): m for m in kets + (bras or [])}.values():   # (a state may be listed many times: overlaps)
            if int(m.bond_dims.max()) > FUSED_CAP:
                raise ValueError(f"the fused route takes bond dimensions up to {FUSED_CAP}, not {int(m.bond_dims.max())}")
    kh = (c_void_p * len(kets))(*[m.handle for m in kets])
    bh = None if bras is None else (c_void_p * len(bras))(*[m.handle for m in bras])
    out = np.empty((len(kets), arr.shape[0]), dtype=np.complex128)
    check(_lib.lib().aqc_mps_pauli(bh, kh, len(kets), arr.shape[0], arr.ctypes.data_as(POINTER(c_uint8)), _PAULI_METHODS[method], dptr(out)))
    return out


def pauli_strings(states, strings, *, bras=None, method: Optional[str] = None) -> np.ndarray:
    """<psi| P_s |psi> for every string: ``(S,)`` complex128 for one state, ``(lanes, S)`` for a list; nothing is normalised.  With
    ``bras`` (a state, or a list as long as ``states``) entry l is <bras[l]| P_s |states[l]>.

    ``strings``: a ``uint8 (S, n)`` array of 0, 1, 2, 3 = I, X, Y, Z, a list of ``str`` over ``IXYZ`` of length n, or a list of sparse
    ``("XZ", (3, 7))`` tuples (X on qubit 3, Z on qubit 7).  Character q of a ``str`` and column q of the array act on qubit q, which is
    index bit q of the dense vector: the project's qubit order, NOT the order in which Qiskit prints a Pauli label (which is reversed).

    Without bras a string is walked over its support only, between the environments of the state, so a local term costs its support and
    not the chain.  ``method``: ``None`` lets the rule choose per pair (``pauli_route``).  A value does not depend on which other
    strings or states are in the call."""
    if method not in _PAULI_METHODS:
        raise ValueError(f"method must be None, 'fused' or 'gemm', not {method!r}")
    single, count, n = _shape_of(states)
    arr = _strings(strings, n)
    if bras is not None and _shape_of(bras) != (single, count, n):
        raise ValueError("bras is one state for one state, or a list as long as states, of the same number of qubits")
    with _Lanes(states) as kets:
        if bras is None:
            out = _pauli_call(None, kets.lanes, arr, method)
        else:
            with _Lanes(bras) as b:
                out = _pauli_call(b.lanes, kets.lanes, arr, method)
    return out[0] if single else out


def overlaps(bras, kets, *, method: Optional[str] = None) -> np.ndarray:
    """The ``(len(bras), len(kets))`` matrix <phi_a|psi_b> in one call (the identity string between all pairs)."""
    if method not in _PAULI_METHODS:
        raise ValueError(f"method must be None, 'fused' or 'gemm', not {method!r}")
    if not isinstance(bras, list) or not isinstance(kets, list):
        raise ValueError("bras and kets are lists of states")
    (_, nb, n), (_, nk, n2) = _shape_of(bras), _shape_of(kets)
    if n != n2:
        raise ValueError("the states differ in the number of qubits")
    with _Lanes(bras) as b, _Lanes(kets) as k:
        pb = [m for m in b.lanes for _ in k.lanes]
        pk = [m for _ in b.lanes for m in k.lanes]
        out = _pauli_call(pb, pk, np.zeros((1, n), dtype=np.uint8), method)
    return out[:, 0].reshape(nb, nk)


def energy(states, terms, *, method: Optional[str] = None) -> np.ndarray:
    """sum_k w_k Re <P_k> for ``terms = [(weight, string), ...]`` (strings as ``pauli_strings`` takes them in a list): ``()`` for one
    state, ``(lanes,)`` for a list."""
    if not isinstance(terms, (list, tuple)) or len(terms) < 1 or any(not (isinstance(t, tuple) and len(t) == 2) for t in terms):
        raise ValueError("terms is a non-empty list of (weight, string)")
    w = np.array([_finite(t[0], "weight") for t in terms], dtype=np.float64)
    strings = [t[1] for t in terms]
    if isinstance(strings[0], np.ndarray):
        strings = np.stack(strings)
    return (pauli_strings(states, strings, method=method).real * w).sum(axis=-1)   # row by row: a state's sum does not depend on the other lanes


def variance(states, op, *, method: Optional[str] = None) -> np.ndarray:
    """<O psi|O psi> / <psi|psi> - |<psi|O psi> / <psi|psi>|^2 for an ``mps_engine.MPO``: ``()`` for one state, ``(lanes,)`` for a list.
    O psi of every state comes from ONE ``mps_engine.apply_operator`` call (exact: nothing is truncated), the three overlaps of every
    state from ``overlaps``.  For a Hermitian operator this is the variance of O in psi; it is zero on an eigenstate up to rounding of
    the size of |O|_2^2.  A state that O annihilates has no O psi: ``RuntimeError``, as ``apply_operator`` raises it."""
    from .mps_engine import MPO, apply_operator

    if not isinstance(op, MPO):
        raise ValueError("an operator is an MPO")
    single, count, n = _shape_of(states)
    if op.num_qubits != n:
        raise ValueError(f"an operator on {op.num_qubits} qubits meets a state of {n}")
    with _Lanes(states) as kets:
        images = apply_operator(op, kets.lanes, method=method)
        try:   # <psi|psi>, <psi|O psi>, <O psi|O psi> of every state: the identity string between 3 x lanes pairs, one call
            g = _pauli_call(kets.lanes + kets.lanes + images, kets.lanes + images + images, np.zeros((1, n), dtype=np.uint8), None)[:, 0].reshape(3, count)
        finally:
            for m in images:
                m.close()
    out = g[2].real / g[0].real - np.abs(g[1] / g[0].real) ** 2
    return out[0] if single else out


# ---- entanglement: the Schmidt spectra of every cut (aqc_mps_ent_schmidt; rules: csrc/aqc_mps_ent_rule.h, kernels: csrc/aqc_mps_ent.hip)

_ENT_METHODS = {None: 0, "fused": 1, "canonical": 2}   # AQC_MPS_ENT_*
_ENT_ROUTES = {1: "fused", 2: "canonical"}
_ENT_SWEEP_LIMIT = 1                                    # status of a cut whose SVD did not converge


def entanglement_route(bond_dims) -> str:
    """The route the rule picks for a state with these n + 1 bond dimensions: ``"fused"`` when every bond is at most ``FUSED_CAP``,
    else ``"canonical"``."""
    d = np.ascontiguousarray(bond_dims, dtype=np.int32)
    if d.ndim != 1 or d.size < 2:
        raise ValueError("expects the n + 1 bond dimensions of a state")
    r = _lib.lib().aqc_mps_ent_route(d.size - 1, iptr(d))
    if r not in _ENT_ROUTES:
        raise ValueError("expects the n + 1 bond dimensions of a state")
    return _ENT_ROUTES[r]


def _ent_method(method):
    if method not in _ENT_METHODS:
        raise ValueError(f"method must be None, 'fused' or 'canonical', not {method!r}")
    return _ENT_METHODS[method]


def _schmidt_call(lanes, method: Optional[str], factors: bool = False):
    """``(values (L, max(n - 1, 1), K), sweeps, status, routes, factors or None)`` for a list of open DeviceMPS."""
    dims = [m.bond_dims for m in lanes]
    n = lanes[0].num_qubits
    routes = [method or entanglement_route(d) for d in dims]
    for d, r in zip(dims, routes):
        if r == "fused" and int(d.max()) > FUSED_CAP:
            raise ValueError(f"the fused route takes bond dimensions up to {FUSED_CAP}, not {int(d.max())}")
        if factors and r != "fused":
            raise ValueError("the factors are those of the fused route")
    kmax = max([1] + [int(d[1:n].max()) for d in dims if n > 1])
    rows = max(n - 1, 1)
    handles = (c_void_p * len(lanes))(*[m.handle for m in lanes])
    s = np.zeros((len(lanes), rows, kmax), dtype=np.float64)
    sweeps, status = np.zeros((len(lanes), rows), dtype=np.int32), np.zeros((len(lanes), rows), dtype=np.int32)
    fac = np.zeros(max(1, sum(2 * int((d[1:n].astype(np.int64) ** 2).sum()) for d in dims)), dtype=np.complex128) if factors else None
    check(_lib.lib().aqc_mps_ent_schmidt(handles, len(lanes), _ENT_METHODS[method], kmax, dptr(s), iptr(sweeps), iptr(status),
                                         None if fac is None else dptr(fac)))
    hit = np.argwhere(status == _ENT_SWEEP_LIMIT)
    if hit.size:
        raise RuntimeError(f"state {int(hit[0, 0])}, cut {int(hit[0, 1]) + 1}: the SVD of the cut reached its sweep limit")
    return s, sweeps, status, routes, fac


def schmidt_values(states, *, method: Optional[str] = None, details: bool = False):
    """The singular values of every cut q = 1 .. n - 1 (qubits 0 .. q-1 | q .. n-1), descending: float64 ``(n - 1, K)`` for one state,
    ``(lanes, n - 1, K)`` for a list, K the largest inner bond dimension of the call; a row is zero beyond its bond dimension.  Nothing
    is normalised: the squares of a row add up to <psi|psi>.  States are taken in whatever gauge they are in and are not modified.

    ``method``: ``None`` lets the rule choose per state (``entanglement_route``): ``"fused"`` takes R factors of the left and right
    halves by QR chains on the device and the singular values of their product for all cuts of all states in one batch, so values far
    below the largest are kept to rounding of the largest; ``"canonical"`` (any bond dimension) runs the engine's identity sweeps on a
    clone and reads the bond vectors, where values below 1e-14 of the largest come back as 0.  A state that is not finite gives NaN
    rows and raises nothing; a cut whose SVD reaches its sweep limit raises ``RuntimeError``.  A state's values do not depend on which
    other states are in the call.  ``details``: ``(values, {"sweeps", "status", "route"})``."""
    _ent_method(method)
    _shape_of(states)
    with _Lanes(states) as lanes:
        n = lanes.lanes[0].num_qubits
        s, sweeps, status, routes, _ = _schmidt_call(lanes.lanes, method)
        cut = slice(0, n - 1)
        s, sweeps, status = s[:, cut], sweeps[:, cut], status[:, cut]
        if lanes.single:
            s, sweeps, status, routes = s[0], sweeps[0], status[0], routes[0]
        return (s, {"sweeps": sweeps, "status": status, "route": routes}) if details else s


def schmidt_factors(state):
    """``(values, C, D)`` of one state on the fused route: lists of the left factors C_q and the right factors D_q of the bonds
    q = 1 .. n - 1 (chi_q x chi_q, upper triangular): C_q^H C_q is the left environment of bond q, D_q^H D_q the conjugate of the right
    one, and the values of cut q are the singular values of C_q D_q^T."""
    single, _, _ = _shape_of(state)
    if not single:
        raise ValueError("expects one state")
    with _Lanes(state) as lanes:
        m = lanes.lanes[0]
        n, d = m.num_qubits, m.bond_dims
        s, _, _, _, fac = _schmidt_call(lanes.lanes, "fused", factors=True)
        block = int((d[1:n].astype(np.int64) ** 2).sum())
        out = []
        for base in (0, block):
            at, mats = base, []
            for q in range(1, n):
                mats.append(fac[at:at + int(d[q]) ** 2].reshape(int(d[q]), int(d[q])).copy())
                at += int(d[q]) ** 2
            out.append(mats)
        return s[0, :n - 1], out[0], out[1]


def entropies_of(values, alpha: float = 1.0) -> np.ndarray:
    """Entanglement entropies of Schmidt values (last axis), natural logarithm, of p = s^2 / sum s^2 with 0 ln 0 = 0: von Neumann at
    ``alpha`` = 1, Renyi otherwise, ``np.inf`` the min-entropy.  Pure NumPy."""
    alpha = float(alpha)
    if not alpha >= 0.0:
        raise ValueError("alpha must be a non-negative number or np.inf")
    s = np.asarray(values, dtype=np.float64)
    w = s * s
    with np.errstate(divide="ignore", invalid="ignore"):
        p = w / w.sum(axis=-1, keepdims=True)
        if alpha == 1.0:
            return -np.where(p > 0.0, p * np.log(np.where(p > 0.0, p, 1.0)), p * 0.0).sum(axis=-1)
        if np.isinf(alpha):
            return -np.log(p.max(axis=-1))
        if alpha == 0.0:   # the logarithm of the rank
            return np.log(np.where(np.isnan(p).any(axis=-1), np.nan, (p > 0.0).sum(axis=-1)))
        return np.log((p ** alpha).sum(axis=-1)) / (1.0 - alpha)


def entanglement_entropies(states, alpha: float = 1.0, *, method: Optional[str] = None) -> np.ndarray:
    """``entropies_of(schmidt_values(states, method=method), alpha)``: ``(n - 1,)`` or ``(lanes, n - 1)``."""
    return entropies_of(schmidt_values(states, method=method), alpha)


def rank_rule(values, trunc_thr: float = 0.0, max_bond: int = 0):
    """``(rank, dropped weight)`` of one descending spectrum by the engine's rank decision (aqc_mps_rank_rule; no device needed): the
    floor 1e-14 s_max, then ``max_bond`` (> 0), then the tail dropped while its weight stays below ``trunc_thr``."""
    s = np.ascontiguousarray(values, dtype=np.float64)
    if s.ndim != 1 or s.size < 1:
        raise ValueError("expects a flat, non-empty spectrum")
    rank, dropped = np.zeros(1, np.int32), np.zeros(1, np.float64)
    check(_lib.lib().aqc_mps_rank_rule(s.size, dptr(s), float(trunc_thr), int(max_bond), iptr(rank), dptr(dropped)))
    return int(rank[0]), float(dropped[0])


def bond_dims_needed(states, trunc_thr: float = 0.0, max_bond: int = 0, *, method: Optional[str] = None):
    """``(ranks, dropped)`` per cut: the bond dimension the engine's rank rule keeps of each cut's spectrum at ``trunc_thr`` /
    ``max_bond`` and the weight it drops: int ``(n - 1,)`` and float64 ``(n - 1,)``, with a leading lanes axis for a list."""
    trunc_thr = _finite(trunc_thr, "trunc_thr")
    if trunc_thr < 0.0 or int(max_bond) < 0:
        raise ValueError("trunc_thr and max_bond must be non-negative")
    _ent_method(method)
    single, _, _ = _shape_of(states)
    with _Lanes(states) as lanes:
        dims = [m.bond_dims for m in lanes.lanes]
        s = schmidt_values(lanes.lanes, method=method)
    ranks, dropped = np.zeros(s.shape[:2], dtype=np.int64), np.zeros(s.shape[:2], dtype=np.float64)
    for lane in range(s.shape[0]):
        for cut in range(s.shape[1]):
            ranks[lane, cut], dropped[lane, cut] = rank_rule(s[lane, cut, :int(dims[lane][cut + 1])], trunc_thr, max_bond)
    return (ranks[0], dropped[0]) if single else (ranks, dropped)
