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

General operators (``mps_engine.MPO``) between states are a walk that carries the operator's bond (aqc_mps_melem; kernels:
csrc/aqc_mps_melem.hip, rules: csrc/aqc_mps_melem_rule.h): ``operator_elements`` gives <phi|O|psi> for many (bra, operator, ket) jobs in
one call without forming O psi, ``operator_matrix`` an operator in a basis of states, ``expectations`` and ``variance_by_walk`` what
their names say.

Entanglement across the cuts of the chain (aqc_mps_ent_schmidt; kernels: csrc/aqc_mps_ent.hip, rules: csrc/aqc_mps_ent_rule.h):
``schmidt_values`` gives the singular values of every cut of one or many states per call, ``entanglement_entropies`` their entropies
(``entropies_of``: NumPy), ``bond_dims_needed`` the bond dimensions the engine's rank rule would keep at a given ``trunc_thr`` /
``max_bond``.
"""
from ctypes import POINTER, c_int64, c_uint8
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check, dptr, iptr
from .mps_engine import (MPO, _BOND_DIMS_OF_A_STATE, _call_states, _handles, _Lanes, _method_code, _packed_ops, _route_of, _truncation,
                         _within_fused_cap, apply_operator)
from .observables import (_bond_energies_of, _bond_pairs, _correlation_letters, _correlation_of, _correlation_pairs, _magnetisation_of,
                          _magnetisation_pairs, _single_axis, pauli_expectation, pauli_matrix)  # noqa: F401  (the last two: for callers)
from .xxz import _finite

FUSED_CAP = 64   # AQC_MPS_OBS_FUSED_CAP of include/aqc_hip.h
_METHODS = {None: 0, "fused": 1, "gemm": 2}   # AQC_MPS_OBS_*
_ROUTES = {1: "fused", 2: "gemm"}


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
    return _route_of("aqc_mps_obs_route", _ROUTES, _BOND_DIMS_OF_A_STATE, (d.size - 1, iptr(d)))


def _two_qubits(n: int) -> None:
    if n < 2:
        raise ValueError("pair density matrices need at least 2 qubits")


def _rdms(states, pairs_of, method: Optional[str]):
    """``(rho, lanes)``: the matrices of the pairs ``pairs_of(n)`` of every state of the call; everything is refused before an upload."""
    code = _method_code(method, _METHODS)
    lanes = _Lanes(states)
    arr = _pairs(pairs_of(lanes.n), lanes.n)
    _within_fused_cap(method, lanes.dims, FUSED_CAP)
    out = np.empty((len(lanes.items), arr.shape[0], 4, 4), dtype=np.complex128)
    with lanes:
        check(_lib.lib().aqc_mps_obs_pairs(lanes.handles(), len(lanes.lanes), arr.shape[0], iptr(arr), code, dptr(out)))
    return (out[0] if lanes.single else out), lanes


def pair_density_matrices(states, pairs=None, *, method: Optional[str] = None) -> np.ndarray:
    """The two-qubit reduced density matrices of ``pairs`` (``None``: all i < j in lexicographic order): ``(P, 4, 4)`` for one state,
    ``(lanes, P, 4, 4)`` for a list."""
    def wanted(n):
        _two_qubits(n)
        return _correlation_pairs(n) if pairs is None else pairs

    return _rdms(states, wanted, method)[0]


def reduced_density_matrix(states, qubits: Sequence[int], *, method: Optional[str] = None) -> np.ndarray:
    """The reduced density matrix of 1 or 2 listed qubits: ``(2^k, 2^k)`` for one state, ``(lanes, 2^k, 2^k)`` for a list.  One qubit
    is read from the pair with a neighbour, whose other qubit is traced out."""
    qs = np.asarray(qubits)
    if qs.ndim != 1 or qs.size not in (1, 2) or not np.issubdtype(qs.dtype, np.integer):
        raise ValueError("expects a flat list of 1 or 2 qubit numbers")
    q = int(qs[0])

    def pair(n):
        _two_qubits(n)
        if qs.size == 2:
            return qs[None, :]
        if not 0 <= q < n:
            raise ValueError(f"qubit out of range: {n} qubits")
        return [(q, q + 1 if q + 1 < n else q - 1)]

    rho, lanes = _rdms(states, pair, method)
    rho = rho[0] if lanes.single else rho[:, 0]
    if qs.size == 2:
        return rho
    r = rho.reshape(rho.shape[:-2] + (2, 2, 2, 2))   # [other][q][other'][q']
    return r[..., 0, :, 0, :] + r[..., 1, :, 1, :]


def magnetisation(states, axis: str = "z", *, method: Optional[str] = None) -> np.ndarray:
    """<sigma_i> along ``axis`` for every qubit: ``(n,)`` or ``(lanes, n)``.  Read from the ceil(n / 2) pairs (0, 1), (2, 3), ...
    (the last qubit of an odd chain with its left neighbour).  Not divided by <psi|psi>."""
    a = _single_axis(axis)
    rho, lanes = _rdms(states, _magnetisation_pairs, method)
    return _magnetisation_of(rho, lanes.n, a)


def correlation_matrix(states, letters: str = "zz", connected: bool = False, *, method: Optional[str] = None) -> np.ndarray:
    """C[i][j] = <a_i b_j> for ``letters = "ab"`` out of x, y, z, over all pairs: ``(n, n)`` or ``(lanes, n, n)``.  The diagonal is 1
    for equal letters and 0 otherwise, as in ``observables.correlation_matrix``.  ``connected``: minus <a_i><b_j>."""
    a, b = _correlation_letters(letters)
    rho, lanes = _rdms(states, _correlation_pairs, method)
    return _correlation_of(rho, lanes.n, a, b, connected)


def bond_energies(states, delta: float, *, method: Optional[str] = None) -> np.ndarray:
    """-1/4 tr rho_{i,i+1} (XX + YY + delta ZZ) for the n - 1 bonds of the open XXZ chain: ``(n - 1,)`` or ``(lanes, n - 1)``."""
    delta = _finite(delta, "delta")
    rho, _ = _rdms(states, _bond_pairs, method)
    return _bond_energies_of(rho, delta)


# ---- Pauli strings: <phi|P|psi> for many strings and pairs of states per call (aqc_mps_pauli; rules: csrc/aqc_mps_pauli_rule.h)

_PAULI_METHODS = {None: 0, "fused": 1, "gemm": 2}   # AQC_MPS_PAULI_*
_LETTERS = {"I": 0, "X": 1, "Y": 2, "Z": 3}


def pauli_route(bra_dims, ket_dims) -> str:
    """The route the rule picks for a pair with these n + 1 bond dimensions each (``bra_dims`` None: the ket's): ``"fused"`` when every
    bond of both is at most ``FUSED_CAP``, else ``"gemm"``."""
    k = np.ascontiguousarray(ket_dims, dtype=np.int32)
    b = None if bra_dims is None else np.ascontiguousarray(bra_dims, dtype=np.int32)
    fits = k.ndim == 1 and k.size >= 2 and (b is None or b.shape == k.shape)
    return _route_of("aqc_mps_pauli_route", _ROUTES, "expects the n + 1 bond dimensions of the bra and of the ket",
                     (k.size - 1, None if b is None else iptr(b), iptr(k)) if fits else None)


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


def _pauli_call(bras, kets, arr: np.ndarray, code: int) -> np.ndarray:
    """``(len(kets), S)``: <bras[p]| P_s |kets[p]> (``bras`` None: expectation mode) for lists of open DeviceMPS."""
    out = np.empty((len(kets), arr.shape[0]), dtype=np.complex128)
    check(_lib.lib().aqc_mps_pauli(None if bras is None else _handles(bras), _handles(kets), len(kets), arr.shape[0],
                                   arr.ctypes.data_as(POINTER(c_uint8)), code, dptr(out)))
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
    code = _method_code(method, _PAULI_METHODS)
    kets = _Lanes(states)
    arr = _strings(strings, kets.n)
    b = None if bras is None else _Lanes(bras)
    if b is not None and (b.single, len(b.items), b.n) != (kets.single, len(kets.items), kets.n):
        raise ValueError("bras is one state for one state, or a list as long as states, of the same number of qubits")
    _within_fused_cap(method, kets.dims + ([] if b is None else b.dims), FUSED_CAP)
    with kets:
        if b is None:
            out = _pauli_call(None, kets.lanes, arr, code)
        else:
            with b:
                out = _pauli_call(b.lanes, kets.lanes, arr, code)
    return out[0] if kets.single else out


def overlaps(bras, kets, *, method: Optional[str] = None) -> np.ndarray:
    """The ``(len(bras), len(kets))`` matrix <phi_a|psi_b> in one call (the identity string between all pairs)."""
    code = _method_code(method, _PAULI_METHODS)
    if not isinstance(bras, list) or not isinstance(kets, list):
        raise ValueError("bras and kets are lists of states")
    b, k = _Lanes(bras), _Lanes(kets)
    if b.n != k.n:
        raise ValueError("the states differ in the number of qubits")
    _within_fused_cap(method, k.dims + b.dims, FUSED_CAP)
    with b, k:
        pb = [m for m in b.lanes for _ in k.lanes]
        pk = [m for _ in b.lanes for m in k.lanes]
        out = _pauli_call(pb, pk, np.zeros((1, k.n), dtype=np.uint8), code)
    return out[:, 0].reshape(len(b.lanes), len(k.lanes))


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
    if not isinstance(op, MPO):
        raise ValueError("an operator is an MPO")
    kets = _Lanes(states)
    count, n = len(kets.items), kets.n
    if op.num_qubits != n:
        raise ValueError(f"an operator on {op.num_qubits} qubits meets a state of {n}")
    with kets:
        images = apply_operator(op, kets.lanes, method=method)
        try:   # <psi|psi>, <psi|O psi>, <O psi|O psi> of every state: the identity string between 3 x lanes pairs, one call
            g = _pauli_call(kets.lanes + kets.lanes + images, kets.lanes + images + images, np.zeros((1, n), dtype=np.uint8),
                            _PAULI_METHODS[None])[:, 0].reshape(3, count)
        finally:
            for m in images:
                m.close()
    out = g[2].real / g[0].real - np.abs(g[1] / g[0].real) ** 2
    return out[0] if kets.single else out


# ---- matrix elements of operators: <phi|O|psi> for many (bra, operator, ket) jobs per call, by a walk that carries the operator's bond
# (aqc_mps_melem; rules: csrc/aqc_mps_melem_rule.h, kernels: csrc/aqc_mps_melem.hip)

MELEM_OP_CAP = 32                                   # AQC_MPS_MELEM_OP_CAP
_MELEM_METHODS = {None: 0, "fused": 1, "gemm": 2}   # AQC_MPS_MELEM_*


def melem_route(bra_dims, ket_dims, op_dims) -> str:
    """The route the rule picks for a job with these n + 1 bond dimensions each (``bra_dims`` None: the ket's, ``op_dims`` None: the
    identity): ``"fused"`` when every bond of bra and ket is at most ``FUSED_CAP`` and every operator bond at most ``MELEM_OP_CAP``, else
    ``"gemm"``."""
    k = np.ascontiguousarray(ket_dims, dtype=np.int32)
    b = None if bra_dims is None else np.ascontiguousarray(bra_dims, dtype=np.int32)
    o = None if op_dims is None else np.ascontiguousarray(op_dims, dtype=np.int32)
    fits = k.ndim == 1 and k.size >= 2 and (b is None or b.shape == k.shape) and (o is None or o.shape == k.shape)
    return _route_of("aqc_mps_melem_route", _ROUTES, "expects the n + 1 bond dimensions of the bra, of the ket and of the operator",
                     (k.size - 1, None if b is None else iptr(b), iptr(k), None if o is None else iptr(o)) if fits else None)


def operator_elements(jobs, *, method: Optional[str] = None) -> np.ndarray:
    """<phi|O|psi> for every job of ``jobs = [(bra, op_or_None, ket), ...]``: ``(J,)`` complex128, nothing normalised.  ``op`` is an
    ``mps_engine.MPO`` (``None``: the identity, the overlap), bra and ket a DeviceMPS or a QiskitMPS tuple of the operator's qubit
    count, any gauge.  States and operators that are the same object are uploaded once.  O psi is never formed: there is no SVD, no
    truncation and no intermediate state, and the cost of a job is 2 (D_q + D_{q+1}) matrix products per site for an operator whose
    sites are as sparse as those of ``MPO.xxz``.  Errors are of the size of rounding relative to ``|phi| |O|_2 |psi|``.

    ``method``: ``None`` lets the rule choose per job (``melem_route``).  A job's value does not depend on which other jobs are in the
    call; non-finite entries are data and spoil their own jobs only."""
    code = _method_code(method, _MELEM_METHODS)
    if not isinstance(jobs, list) or not jobs or any(not (isinstance(j, tuple) and len(j) == 3) for j in jobs):
        raise ValueError("jobs is a non-empty list of (bra, op_or_None, ket)")
    states, ops, state_at, op_at, n = [], [], {}, {}, None
    job_bra, job_op, job_ket = [], [], []
    for j, (bra, op, ket) in enumerate(jobs):
        if op is not None and not isinstance(op, MPO):
            raise ValueError(f"job {j}: an operator is an MPO or None")
        dims = []
        for state in (bra, ket):
            d = _call_states([state])[3][0]   # (a job takes one state each side: a list in its place is refused as no state)
            n = d.size - 1 if n is None else n
            if d.size - 1 != n:
                raise ValueError("the states differ in the number of qubits")
            dims.append(d)
        if op is not None and op.num_qubits != n:
            raise ValueError(f"job {j}: an operator on {op.num_qubits} qubits meets a state of {n}")
        if method == "fused" and melem_route(dims[0], dims[1], None if op is None else op.bond_dims) != "fused":
            raise ValueError(f"the fused route takes bond dimensions up to {FUSED_CAP} and operator bond dimensions up to {MELEM_OP_CAP} (job {j})")
        for state, column in ((bra, job_bra), (ket, job_ket)):
            if id(state) not in state_at:
                state_at[id(state)] = len(states)
                states.append(state)
            column.append(state_at[id(state)])
        if op is not None and id(op) not in op_at:
            op_at[id(op)] = len(ops)
            ops.append(op)
        job_op.append(-1 if op is None else op_at[id(op)])
    job_bra, job_op, job_ket = (np.array(a, dtype=np.int32) for a in (job_bra, job_op, job_ket))
    op_dims, op_off, op_data = _packed_ops(ops, n)
    out = np.empty(len(jobs), dtype=np.complex128)
    with _Lanes(states) as lanes:
        check(_lib.lib().aqc_mps_melem(lanes.handles(), len(lanes.lanes), len(ops), iptr(op_dims) if ops else None,
                                       op_off.ctypes.data_as(POINTER(c_int64)) if ops else None, dptr(op_data) if ops else None, len(jobs),
                                       iptr(job_bra), iptr(job_op), iptr(job_ket), code, dptr(out)))
    return out


def _state_list(states, what: str):
    if not isinstance(states, list) or not states:
        raise ValueError(f"{what} is a non-empty list of states")
    return states


def operator_matrix(op, kets, bras=None, *, method: Optional[str] = None) -> np.ndarray:
    """The ``(len(bras), len(kets))`` matrix <phi_a|O|psi_b> in one call (``bras`` None: the kets): a Hamiltonian in a basis of MPS
    states, or with ``op`` None their Gram matrix."""
    kets = _state_list(kets, "kets")
    bras = kets if bras is None else _state_list(bras, "bras")
    return operator_elements([(b, op, k) for b in bras for k in kets], method=method).reshape(len(bras), len(kets))


def expectations(states, ops, *, method: Optional[str] = None) -> np.ndarray:
    """<psi|O_k|psi> for every state and every operator of the list ``ops`` in one call: ``(nops,)`` complex128 for one state,
    ``(lanes, nops)`` for a list; not divided by <psi|psi>."""
    if not isinstance(ops, (list, tuple)) or not ops:
        raise ValueError("ops is a non-empty list of operators")
    single, items, _, _ = _call_states(states)
    out = operator_elements([(s, o, s) for s in items for o in ops], method=method).reshape(len(items), len(ops))
    return out[0] if single else out


def variance_by_walk(states, op, *, method: Optional[str] = None) -> np.ndarray:
    """<psi|O^H O|psi> / <psi|psi> - |<psi|O|psi> / <psi|psi>|^2 as ``variance`` gives it, from ONE ``operator_elements`` call with three
    jobs per state (the identity, O, and ``op.adjoint().times(op)`` with bonds D^2): O psi is never formed, so nothing is compressed and
    a state that O annihilates simply has variance 0.  ``()`` for one state, ``(lanes,)`` for a list."""
    if not isinstance(op, MPO):
        raise ValueError("an operator is an MPO")
    single, items, n, _ = _call_states(states)
    if op.num_qubits != n:
        raise ValueError(f"an operator on {op.num_qubits} qubits meets a state of {n}")
    square = op.adjoint().times(op)
    g = operator_elements([(s, o, s) for s in items for o in (None, op, square)], method=method).reshape(len(items), 3)
    out = g[:, 2].real / g[:, 0].real - np.abs(g[:, 1] / g[:, 0].real) ** 2
    return out[0] if single else out


# ---- entanglement: the Schmidt spectra of every cut (aqc_mps_ent_schmidt; rules: csrc/aqc_mps_ent_rule.h, kernels: csrc/aqc_mps_ent.hip)

_ENT_METHODS = {None: 0, "fused": 1, "canonical": 2}   # AQC_MPS_ENT_*
_ENT_ROUTES = {1: "fused", 2: "canonical"}
_ENT_SWEEP_LIMIT = 1                                    # status of a cut whose SVD did not converge


def entanglement_route(bond_dims) -> str:
    """The route the rule picks for a state with these n + 1 bond dimensions: ``"fused"`` when every bond is at most ``FUSED_CAP``,
    else ``"canonical"``."""
    d = np.ascontiguousarray(bond_dims, dtype=np.int32)
    return _route_of("aqc_mps_ent_route", _ENT_ROUTES, _BOND_DIMS_OF_A_STATE, (d.size - 1, iptr(d)) if d.ndim == 1 and d.size >= 2 else None)


def _schmidt_call(lanes: _Lanes, method: Optional[str], factors: bool = False):
    """``(values (L, max(n - 1, 1), K), sweeps, status, routes, factors or None)`` of the states of a call, which it uploads for itself;
    ``factors`` go with ``method="fused"``."""
    code = _method_code(method, _ENT_METHODS)
    dims, n, count = lanes.dims, lanes.n, len(lanes.items)
    routes = [method or entanglement_route(d) for d in dims]
    _within_fused_cap(method, dims, FUSED_CAP)
    kmax = max([1] + [int(d[1:n].max()) for d in dims if n > 1])
    rows = max(n - 1, 1)
    s = np.zeros((count, rows, kmax), dtype=np.float64)
    sweeps, status = np.zeros((count, rows), dtype=np.int32), np.zeros((count, rows), dtype=np.int32)
    fac = np.zeros(max(1, sum(2 * int((d[1:n].astype(np.int64) ** 2).sum()) for d in dims)), dtype=np.complex128) if factors else None
    with lanes:
        check(_lib.lib().aqc_mps_ent_schmidt(lanes.handles(), count, code, kmax, dptr(s), iptr(sweeps), iptr(status), None if fac is None else dptr(fac)))
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
    lanes = _Lanes(states)
    s, sweeps, status, routes, _ = _schmidt_call(lanes, method)
    cut = slice(0, lanes.n - 1)
    s, sweeps, status = s[:, cut], sweeps[:, cut], status[:, cut]
    if lanes.single:
        s, sweeps, status, routes = s[0], sweeps[0], status[0], routes[0]
    return (s, {"sweeps": sweeps, "status": status, "route": routes}) if details else s


def schmidt_factors(state):
    """``(values, C, D)`` of one state on the fused route: lists of the left factors C_q and the right factors D_q of the bonds
    q = 1 .. n - 1 (chi_q x chi_q, upper triangular): C_q^H C_q is the left environment of bond q, D_q^H D_q the conjugate of the right
    one, and the values of cut q are the singular values of C_q D_q^T."""
    lanes = _Lanes(state)
    if not lanes.single:
        raise ValueError("expects one state")
    n, d = lanes.n, lanes.dims[0]
    s, _, _, _, fac = _schmidt_call(lanes, "fused", factors=True)
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
    trunc_thr, max_bond = _truncation(_finite(trunc_thr, "trunc_thr"), max_bond)
    lanes = _Lanes(states)
    s = _schmidt_call(lanes, method)[0][:, :lanes.n - 1]
    ranks, dropped = np.zeros(s.shape[:2], dtype=np.int64), np.zeros(s.shape[:2], dtype=np.float64)
    for lane in range(s.shape[0]):
        for cut in range(s.shape[1]):
            ranks[lane, cut], dropped[lane, cut] = rank_rule(s[lane, cut, :int(lanes.dims[lane][cut + 1])], trunc_thr, max_bond)
    return (ranks[0], dropped[0]) if lanes.single else (ranks, dropped)
