"""GPU: every batched entry point held to its lanes' own results, bit for bit (DESIGN 6s;the checks are tests/lane_contract.py, which
tests/test_lane_contract_host.py holds to planted faults).

For a fixed call shape a lane's outputs are a function of that lane's inputs alone and the same call gives the same bits: R (repeat),
P (position), F (other finite neighbours), N (NaN neighbours) and, for the three launches that clamp a grid dimension at 65535, G (a
count of 65538).  Nothing is compared between different batch sizes.  Lane 0 (for G: every probe lane) is compared once with the
reference and tolerance of the feature's own test; everything else is np.array_equal.

Every case that names a route or a kernel family asserts through the workspace's or the module's introspection that it ran."""
import functools

import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests import mps_obs_ref, mps_pauli_ref, obs_ref, xxz_ref
from tests.helpers import FAMILY_ENV, TOL
from tests.lane_contract import check_lanes, nan_filled
from tests.test_hip_observables import RDM_TOL
from tests.test_hip_xxz import STATE_TOL

pytestmark = pytest.mark.gpu

PAST_THE_GRID = 65535 + 3
GRID_PROBES = (0, 65534, 65535, 65536, 65537)

# every switch a case of this module may set: unset unless the case says otherwise, whatever the caller's environment holds
_SWITCHES = ("AQC_KERNEL_FAMILY", "AQC_KERNEL_V2", "AQC_SPARSE_SWEEP", "AQC_SPARSE_MIN_ITEMS", "AQC_LAZY_Z", "AQC_PROJECTED", "AQC_PROJECTED_VDAG",
             "AQC_PROJECTED_VDAG_MIN_ELEMS", "AQC_PROJECTED_FUSED", "AQC_PROJECTED_FUSED_MAX_SHARES", "AQC_PROJECTED_PAIRS", "AQC_APPLY_PERSIST",
             "AQC_SWEEP_GRID", "AQC_GRAPH", "AQC_TILE_BITS_APPLY", "AQC_TILE_BITS_SWEEP", "AQC_THREADS", "AQC_LOW_BITS")


def _set_switches(monkeypatch, env):
    for name in _SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ======== state vectors: the XXZ Hamiltonian and the pair density matrices ===============================================================
@functools.lru_cache(maxsize=None)
def _vectors(n, lanes, seed):
    return _frozen(xxz_ref.random_states(n, lanes, seed))[0]


def _other_vectors(n, lanes, seed):
    """Data of another kind: not normalised, six orders of magnitude larger."""
    return 1.0e6 * _vectors(n, lanes, seed + 1)


@pytest.mark.parametrize("n", (3, 12))
@pytest.mark.parametrize("op", ("mul_vec", "energy"))
def test_xxz_mul_vec_and_energy(op, n):
    from aqc_research_amd.xxz import xxz_energy, xxz_mul_vec

    delta, lanes = -0.7, 5
    states = _vectors(n, lanes, 9100 + n)
    if op == "mul_vec":
        run = lambda s: xxz_mul_vec(s, delta)
        ref = lambda s, l: xxz_ref.mul_vec(s[l], delta)
    else:
        run = lambda s: xxz_energy(s, delta)
        ref = lambda s, l: np.vdot(s[l], xxz_ref.mul_vec(s[l], delta)).real
    check_lanes(run, states, other=_other_vectors(n, lanes, 9100 + n), reference=ref, tol=STATE_TOL)


@pytest.mark.parametrize("shared", (False, True), ids=("lanes", "shared-source"))
@pytest.mark.parametrize("n", (3, 12))
def test_xxz_evolve(n, shared):
    """Per-lane times.  F: the neighbours evolve ten times longer, so the probe lanes run the extra steps of the longer series with zero
    coefficients.  The times are validated by the call (a NaN is refused for the whole call), so N poisons the states alone; with the
    shared source there is no state per lane to poison and N does not apply."""
    from aqc_research_amd.xxz import xxz_evolve

    delta, lanes = 1.0, 5
    times = np.array([0.3, 1.2, -1.2, 2.9, 0.7])
    states = _vectors(n, lanes, 9200 + n)

    def run_lanes(inputs):
        out, info = xxz_evolve(inputs[0], delta, inputs[1], details=True)
        return {"state": out, "terms": info["terms"]}

    def run_shared(t):
        out, info = xxz_evolve(states[0], delta, t, details=True)
        return {"state": out, "terms": info["terms"]}

    longer = 10.0 * times[::-1]
    length = lambda t: xxz_ref.series_length(xxz_ref.radius(n, delta) * t)
    assert min(length(longer[l]) for l in (1, 3)) > max(length(times[l]) for l in (0, 2, 4)), "the neighbours' series are the longer ones"
    if shared:
        check_lanes(run_shared, times, checks="RPF", other=longer, tol=STATE_TOL,
                    reference=lambda t, l: {"state": xxz_ref.evolve_lanes(states[0], delta, [t[l]])[0]})
    else:
        check_lanes(run_lanes, (states, times), other=(_other_vectors(n, lanes, 9200 + n), longer), tol=STATE_TOL,
                    poison=lambda inputs, others: (nan_filled(inputs[0], others), inputs[1]),
                    reference=lambda inputs, l: {"state": xxz_ref.evolve_lanes(inputs[0][l], delta, [inputs[1][l]])[0]})


@pytest.mark.parametrize("n", (4, 12))
def test_state_vector_pair_density_matrices(n):
    from aqc_research_amd.observables import pair_density_matrices

    lanes = 5
    states = _vectors(n, lanes, 9300 + n)
    pairs = obs_ref.all_pairs(n)
    check_lanes(pair_density_matrices, states, other=_other_vectors(n, lanes, 9300 + n), tol=RDM_TOL,
                reference=lambda s, l: obs_ref.pair_rdms(s[l], pairs))


@pytest.mark.parametrize("op", ("mul_vec", "energy", "evolve", "pair_density_matrices"))
def test_state_vector_counts_past_the_grid(op):
    """65538 lanes of 2 qubits: the lane loops of xxz_step_kernel, xxz_energy_final, obs_pass_kernel and obs_final_kernel run their
    second round (lanes 65535 .. 65537 in workgroups 0 .. 2 behind lanes 0 .. 2), R and P on the probe lanes, which are also held to
    the NumPy statement."""
    from aqc_research_amd.observables import pair_density_matrices
    from aqc_research_amd.xxz import xxz_energy, xxz_evolve, xxz_mul_vec

    n, delta = 2, -0.7
    states = _vectors(n, PAST_THE_GRID, 9400)
    kw = dict(checks="RP", probes=GRID_PROBES, compare_lanes=GRID_PROBES, reference_lanes=GRID_PROBES)
    if op == "mul_vec":
        check_lanes(lambda s: xxz_mul_vec(s, delta), states, tol=STATE_TOL, reference=lambda s, l: xxz_ref.mul_vec(s[l], delta), **kw)
    elif op == "energy":
        check_lanes(lambda s: xxz_energy(s, delta), states, tol=STATE_TOL,
                    reference=lambda s, l: np.vdot(s[l], xxz_ref.mul_vec(s[l], delta)).real, **kw)
    elif op == "evolve":
        times = np.linspace(-2.0, 2.0, PAST_THE_GRID)
        check_lanes(lambda inputs: xxz_evolve(inputs[0], delta, inputs[1]), (states, times), tol=STATE_TOL,
                    reference=lambda inputs, l: xxz_ref.evolve_lanes(inputs[0][l], delta, [inputs[1][l]])[0], **kw)
    else:
        check_lanes(pair_density_matrices, states, tol=RDM_TOL, reference=lambda s, l: obs_ref.pair_rdms(s[l], [(0, 1)]), **kw)


# ======== matrix-product states: observables, Pauli strings, overlaps =====================================================================
# n = 7; A: bonds that are no multiple of 4 or 16, up to the fused cap itself; D: beyond the cap (the rule picks gemm)
_MPS_N = 7
_BONDS = {"A": [1, 2, 3, 7, 64, 37, 5, 1], "A2": [1, 2, 4, 13, 33, 64, 2, 1], "D": [1, 2, 4, 65, 96, 40, 2, 1], "D2": [1, 2, 3, 17, 65, 72, 2, 1]}


@functools.lru_cache(maxsize=None)
def _mps(profile, seed):
    return mps_obs_ref.hand_made(_BONDS[profile], seed)


@functools.lru_cache(maxsize=None)
def _mps_dense(profile, seed):
    return _frozen(mps_obs_ref.dense(_mps(profile, seed)))[0]


def _nan_mps(profile, seed):
    """The state with a NaN in every tensor."""
    gam, lam = _mps(profile, seed)
    return [(g0 * np.nan, g1 * np.nan) for g0, g1 in gam], lam


class _Devices:
    """DeviceMPS handles of QiskitMPS tuples, uploaded once and closed at the end of the case."""

    def __init__(self):
        self.made = {}

    def __call__(self, profile, seed, nan=False):
        from aqc_research_amd.mps_engine import DeviceMPS

        key = (profile, seed, nan)
        if key not in self.made:
            self.made[key] = DeviceMPS.from_qiskit(_nan_mps(profile, seed) if nan else _mps(profile, seed), assume_canonical=True)
        return self.made[key]

    def close(self):
        for m in self.made.values():
            m.close()


@pytest.fixture
def devices():
    d = _Devices()
    yield d
    d.close()


def _route_profiles(method):
    """(the probes' profile, the neighbours' profile under F): the other profile wherever the route stays the same."""
    return {"fused": ("A", "A2"), "gemm": ("D", "D2"), "gemm-forced": ("A", "D")}[method]


@pytest.mark.parametrize("method", ("fused", "gemm", "gemm-forced"))
def test_mps_pair_density_matrices(method, devices):
    """Four states per call.  fused / gemm: the rule's choice for profiles A / D, the neighbours of F with other bonds of the same
    route; gemm-forced: profile A with method="gemm", the neighbours of F get profile D's bonds."""
    from aqc_research_amd.mps_observables import pair_density_matrices, route

    mine, theirs = _route_profiles(method)
    states = [devices(mine, 700 + l) for l in range(4)]
    other = [devices(theirs, 720 + l) for l in range(4)]
    want = "gemm" if method != "fused" else "fused"
    arg = None if method != "gemm-forced" else "gemm"
    if arg is None:
        assert all(route(m.bond_dims) == want for m in states + other)
    pairs = obs_ref.all_pairs(_MPS_N)
    check_lanes(lambda s: pair_density_matrices(s, method=arg), states, checks="RPF", probes=(0, 3), other=other, tol=TOL,
                reference=lambda s, l: obs_ref.pair_rdms(_mps_dense(mine, 700 + l), pairs))


_STRINGS = ["IIIIIII", "ZIIIIII", "IIXYIII", "XIIIIIZ", "IYZXZYI", "ZZZZZZZ"]     # six supports: none, one site, inside, the ends, all


@pytest.mark.parametrize("mode", ("expectation", "bra-ket"))
@pytest.mark.parametrize("method", ("fused", "gemm"))
def test_mps_pauli_strings(method, mode, devices):
    """Four pairs, six strings.  F: neighbours with other bonds of the same route; N: every neighbour state holds NaN tensors."""
    from aqc_research_amd.mps_observables import _strings, pauli_route, pauli_strings

    mine, theirs = _route_profiles(method)
    kets = [devices(mine, 740 + l) for l in range(4)]
    bras = [devices(mine, 750 + l) for l in range(4)]
    arr = _strings(_STRINGS, _MPS_N)
    for k, b in zip(kets, bras):
        assert pauli_route(None if mode == "expectation" else b.bond_dims, k.bond_dims) == method
    if mode == "expectation":
        check_lanes(lambda s: pauli_strings(s, _STRINGS, method=None), kets, probes=(0, 3), tol=TOL,
                    other=[devices(theirs, 760 + l) for l in range(4)], poison=[devices(mine, 740 + l, nan=True) for l in range(4)],
                    reference=lambda s, l: mps_pauli_ref.by_dense(_mps(mine, 740 + l), _mps(mine, 740 + l), arr, _mps_dense(mine, 740 + l),
                                                                  _mps_dense(mine, 740 + l)))
    else:
        check_lanes(lambda s: pauli_strings(s[0], _STRINGS, bras=s[1], method=None), (kets, bras), probes=(0, 3), tol=TOL,
                    other=([devices(theirs, 760 + l) for l in range(4)], [devices(theirs, 770 + l) for l in range(4)]),
                    poison=([devices(mine, 740 + l, nan=True) for l in range(4)], [devices(mine, 750 + l, nan=True) for l in range(4)]),
                    reference=lambda s, l: mps_pauli_ref.by_dense(_mps(mine, 750 + l), _mps(mine, 740 + l), arr, _mps_dense(mine, 750 + l),
                                                                  _mps_dense(mine, 740 + l)))


@pytest.mark.parametrize("method", ("fused", "gemm"))
def test_mps_overlaps(method, devices):
    """The 4 x 4 matrix <phi_a|psi_b>: a lane is a ket (a column), the bras are shared, so a poisoned ket must leave the other columns."""
    from aqc_research_amd.mps_observables import overlaps, pauli_route

    mine, theirs = _route_profiles(method)
    kets = [devices(mine, 780 + l) for l in range(4)]
    bras = [devices(mine, 790 + l) for l in range(4)]
    assert all(pauli_route(b.bond_dims, k.bond_dims) == method for b in bras for k in kets)
    check_lanes(lambda s: overlaps(bras, s).T.copy(), kets, probes=(0, 3), tol=TOL,
                other=[devices(theirs, 800 + l) for l in range(4)], poison=[devices(mine, 780 + l, nan=True) for l in range(4)],
                reference=lambda s, l: np.array([np.vdot(_mps_dense(mine, 790 + a), _mps_dense(mine, 780 + l)) for a in range(4)]))


def test_mps_pauli_strings_past_the_grid():
    """65538 pairs in expectation mode that name three bond-1 states of two qubits, one string: the fused route's second launch (pairs
    65535 .. 65537).  Pair l names state (l + l // 65535) mod 3, so a wrapped pair differs from its predecessor and from the pair of
    the first launch that had its workgroup."""
    from aqc_research_amd.mps_engine import DeviceMPS
    from aqc_research_amd.mps_observables import pauli_route, pauli_strings

    tuples = [mps_obs_ref.hand_made([1, 1, 1], 810 + k) for k in range(3)]
    dense = [mps_obs_ref.dense(t) for t in tuples]
    three = [DeviceMPS.from_qiskit(t, assume_canonical=True) for t in tuples]
    try:
        assert pauli_route(None, three[0].bond_dims) == "fused"
        which = [(l + l // 65535) % 3 for l in range(PAST_THE_GRID)]
        lanes = [three[k] for k in which]
        arr = np.array([[1, 3]], dtype=np.uint8)                               # X on qubit 0, Z on qubit 1
        assert len({which[l] for l in (65534, 65535, 65537)}) == 3 and all(which[a] != which[b] for a, b in zip(GRID_PROBES, GRID_PROBES[1:]))
        out = check_lanes(lambda s: pauli_strings(s, arr), lanes, checks="RP", probes=(65534, 65535, 65537), compare_lanes=GRID_PROBES, tol=TOL,
                          reference_lanes=GRID_PROBES,
                          reference=lambda s, l: mps_pauli_ref.by_dense(tuples[which[l]], tuples[which[l]], arr, dense[which[l]], dense[which[l]]))
        for k in range(3):                                                     # every pair of the call: its state's value
            rows = out["out"][np.array(which) == k]
            assert np.all(rows == rows[0])
    finally:
        for m in three:
            m.close()


# ======== the workspace: V, V^H, one-call evaluations =====================================================================================
@functools.lru_cache(maxsize=None)
def _circuit(n, kind, depth):
    from aqc_research_amd import ParametricCircuit, TrotterAnsatz
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    if kind == "trotter2":
        return TrotterAnsatz(n, orc.trotter_blocks(n, depth), second_order=True)
    if kind == "spin":
        return ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", depth))
    rng = np.random.default_rng(100 * n + depth)
    blocks = np.stack([rng.permutation(n)[:2] for _ in range(depth)], axis=1).astype(np.int64)
    blocks[:, 0] = (0, n - 1)                                                  # a long-range block
    return ParametricCircuit(n, kind, blocks)


@functools.lru_cache(maxsize=None)
def _dense_inputs(n, kind, depth, lanes, seed, scale=1.0):
    circ = _circuit(n, kind, depth)
    rng = np.random.default_rng(seed)
    th = rng.uniform(-np.pi, np.pi, size=(lanes, circ.num_thetas)) * (1.0 if scale == 1.0 else 3.0)
    x = rng.standard_normal((lanes, 1 << n)) + 1j * rng.standard_normal((lanes, 1 << n))
    y = rng.standard_normal((lanes, 1 << n)) + 1j * rng.standard_normal((lanes, 1 << n))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    y /= np.linalg.norm(y, axis=1, keepdims=True) / scale
    return _frozen(th, x, y)


class _DenseCalls:
    """apply (V^H, then V), eval(vdag, gather, grad) and eval over a partial block range on dense lhs states: on one workspace with
    everything uploaded again per call, and on a fresh workspace per call."""

    def __init__(self, circ, lanes):
        from aqc_research_amd.engine import HipContext

        self.circ, self.lanes, self.ctx = circ, lanes, HipContext(circ)
        self.flips = np.array([0] + [1 << q for q in range(circ.num_qubits)], dtype=np.int64)
        self.ws = self._create()

    def _create(self):
        from aqc_research_amd.engine import Workspace

        return Workspace(self.ctx, batch=self.lanes)

    def on(self, ws, inputs):
        from aqc_research_amd.engine import BUF_X, BUF_Y, BUF_Z

        th, x, y = inputs
        out = {}
        ws.set_thetas(th)
        ws.upload(BUF_Y, y)
        ws.upload(BUF_X, x)
        ws.apply(True, BUF_Y, BUF_Z)
        out["vdag_y"] = ws.download(BUF_Z)
        ws.apply(False, BUF_X, BUF_Z)
        out["v_x"] = ws.download(BUF_Z)
        ws.gather_setup(self.flips)
        out["amps"], out["grads"] = ws.eval(th, vdag=True, gather=True, grad=True)
        _, out["grads_part"] = ws.eval(th, vdag=False, gather=False, grad=True, block_range=(1, self.circ.num_blocks - 1), front_layer=False)
        out["amps_only"], _ = ws.eval(None, vdag=True, gather=True, grad=False)
        return out

    def same(self, inputs):
        return self.on(self.ws, inputs)

    def fresh(self, inputs):
        ws = self._create()
        try:
            return self.on(ws, inputs)
        finally:
            ws.close()

    def reference(self, inputs, lane):
        th, x, y = (a[lane] for a in inputs)
        z = orc.v_dagger_mul_vec(self.circ, th, y)
        return {"vdag_y": z, "v_x": orc.v_mul_vec(self.circ, th, x), "amps": z[self.flips], "amps_only": z[self.flips],
                "grads": orc.grad_of_dot_product(self.circ, th, x, z),
                "grads_part": orc.grad_of_dot_product(self.circ, th, x, z, (1, self.circ.num_blocks - 1), False)}


# (qubits, circuit, depth, family or None for the shape's own, lanes)
_DENSE_CASES = [
    (6, "cx", 10, "per-group", 3), (6, "cp", 10, "per-group", 65), (6, "cp", 10, "register-blocked", 3), (6, "trotter2", 2, "register-blocked", 65),
    (6, "trotter2", 2, "mfma", 3), (6, "cx", 10, "mfma", 65), (8, "cp", 12, None, 3), (8, "cx", 12, None, 65), (8, "trotter2", 2, None, 65),
    (12, "cx", 14, None, 257),
]


@pytest.mark.parametrize("n,kind,depth,family,lanes", _DENSE_CASES)
def test_workspace_dense_calls(n, kind, depth, family, lanes, monkeypatch):
    _set_switches(monkeypatch, {} if family is None else {"AQC_KERNEL_FAMILY": FAMILY_ENV[family]})
    circ = _circuit(n, kind, depth)
    calls = _DenseCalls(circ, lanes)
    try:
        # the matrix-core kernels run from 2^8 amplitudes per lane: by default, and below that size not even on request (family 1 instead)
        want = 3 if family is None else int(FAMILY_ENV[family])
        if family is not None:
            assert calls.ws.switch("AQC_KERNEL_FAMILY") == want
        want = 1 if (want == 3 and n < 8) else want
        assert calls.ws.kernel_family(1) == want and calls.ws.kernel_family(0) == want
        if n == 12:
            assert calls.ws.plan_info(1)[1] == 12 and calls.ws.plan_info(0)[1] == 12, "the persistent kernels run on 2^12 tiles"
        inputs = _dense_inputs(n, kind, depth, lanes, 4000 + n)
        check_lanes(calls.same, inputs, also=(calls.fresh,), other=_dense_inputs(n, kind, depth, lanes, 4500 + n, 1024.0), tol=TOL,
                    reference=calls.reference)
        assert calls.ws.sparse_counts() == (-1, -1, -1), "dense lhs states take the dense route"
    finally:
        calls.ws.close()


@functools.lru_cache(maxsize=None)
def _basis_inputs(n, depth, tile, lanes, seed, scale=1.0):
    circ = _circuit(n, "spin", depth)
    rng = np.random.default_rng(seed)
    th = rng.uniform(-np.pi, np.pi, size=(2, lanes, circ.num_thetas)).transpose(1, 0, 2).copy()        # two theta sets per lane
    y = rng.standard_normal((lanes, 1 << n)) + 1j * rng.standard_normal((lanes, 1 << n))
    y /= np.linalg.norm(y, axis=1, keepdims=True) / scale
    high = 1 << (n - tile)
    basis = np.array([5 | (((3 * b + (seed % 2)) % high) << tile) for b in range(lanes)], dtype=np.int64)  # the same low bits, other tiles
    return _frozen(th, y, basis)


class _BasisCalls:
    """One basis state per lane: eval(th, gather=True) twice (the second call replays the captured graph with new thetas), then
    objective_launch with the second thetas resident."""

    def __init__(self, circ, lanes, tile):
        from aqc_research_amd.engine import HipContext

        self.circ, self.lanes, self.tile, self.ctx = circ, lanes, tile, HipContext(circ)
        n = circ.num_qubits
        self.gather = np.array([5 | (f << tile) for f in range(1 << (n - tile))], dtype=np.int64)
        self.ws = self._create()

    def _create(self):
        from aqc_research_amd.engine import Workspace

        return Workspace(self.ctx, batch=self.lanes, tile_bits_apply=self.tile, tile_bits_sweep=self.tile)

    def on(self, ws, inputs):
        from aqc_research_amd.engine import BUF_X, BUF_Y

        th, y, basis = inputs
        out = {}
        ws.upload(BUF_Y, y)
        ws.set_basis(BUF_X, basis)
        ws.gather_setup(self.gather)
        out["amps0"], out["grads0"] = ws.eval(np.ascontiguousarray(th[:, 0]), gather=True)
        out["amps1"], out["grads1"] = ws.eval(np.ascontiguousarray(th[:, 1]), gather=True)
        ws.set_thetas(np.ascontiguousarray(th[:, 0]))
        ws.objective_launch(BUF_X)
        out["amps_launch"], out["grads_launch"] = ws.gather_fetch(), ws.get_grads()
        return out

    def same(self, inputs):
        return self.on(self.ws, inputs)

    def fresh(self, inputs):
        ws = self._create()
        try:
            return self.on(ws, inputs)
        finally:
            ws.close()

    def reference(self, inputs, lane):
        th, y, basis = (a[lane] for a in inputs)
        x = np.zeros(1 << self.circ.num_qubits, complex)
        x[basis] = 1.0
        out = {}
        for k in (0, 1):
            z = orc.v_dagger_mul_vec(self.circ, th[k], y)
            out[f"amps{k}"], out[f"grads{k}"] = z[self.gather], orc.grad_of_dot_product(self.circ, th[k], x, z)
        out["amps_launch"], out["grads_launch"] = out["amps0"], out["grads0"]
        return out

    def virtual_passes(self, inputs):
        """Applications of the virtual plan in one objective_launch: the objective by projection makes at least two, V^H by its stages none."""
        from aqc_research_amd._lib import K_APPLY_VIRTUAL
        from aqc_research_amd.engine import BUF_X

        self.on(self.ws, inputs)
        self.ws.profile(True)
        self.ws.objective_launch(BUF_X)
        self.ws.sync()
        count = self.ws.profile_get(K_APPLY_VIRTUAL)[0]
        self.ws.profile(False)
        return count


_SMALL = {"AQC_SPARSE_MIN_ITEMS": "1", "AQC_PROJECTED_VDAG_MIN_ELEMS": "1"}
# (qubits, depth, tile, lanes, switches): shapes whose plan has a projected route (test_hip_round5._ROUTE_SHAPES, found on the host)
_BASIS_CASES = {
    "default-shares": (12, 19, 10, 5, _SMALL),
    "one-share": (12, 19, 10, 5, dict(_SMALL, AQC_PROJECTED_FUSED_MAX_SHARES="1")),
    "no-pair-launches": (12, 19, 10, 5, dict(_SMALL, AQC_PROJECTED_PAIRS="0")),
    "unforced-2^24": (16, 40, 12, 256, {}),
}


@pytest.mark.parametrize("case", sorted(_BASIS_CASES))
def test_workspace_basis_state_calls(case, monkeypatch):
    """The sparse-lhs route and the objective by projection.  N poisons the thetas and the target of the other lanes; a basis index
    cannot be poisoned."""
    n, depth, tile, lanes, env = _BASIS_CASES[case]
    _set_switches(monkeypatch, env)
    circ = _circuit(n, "spin", depth)
    calls = _BasisCalls(circ, lanes, tile)
    try:
        for name, val in env.items():
            assert calls.ws.switch(name) == int(val)
        assert calls.ws.projected_info(), "the shape was chosen for the route by projection"
        inputs = _basis_inputs(n, depth, tile, lanes, 5000 + n)
        assert len(set((inputs[2] >> tile).tolist())) > 1, "the basis states lie in different tiles"
        check_lanes(calls.same, inputs, also=(calls.fresh,), other=_basis_inputs(n, depth, tile, lanes, 5501 + n, 1024.0), tol=TOL,
                    reference=calls.reference)
        assert calls.ws.sparse_counts()[0] > 0, "the sparse route did not run"
        assert calls.virtual_passes(inputs) >= 2, "the objective by projection did not run"
    finally:
        calls.ws.close()


# ======== the workspace: surrogate evaluations and the device optimisers ==================================================================
@functools.lru_cache(maxsize=None)
def _surrogate_inputs(n, depth, lanes, seed, kind="clean"):
    """Per lane: four theta sets, a target, the objective's weight and leading state.  Odd lanes lean towards a flipped basis state, so
    that some lanes lead with a flip state.  kind "other": larger angles, targets of norm 8, other weights."""
    circ = _circuit(n, "spin", depth)
    rng = np.random.default_rng(seed)
    th = rng.uniform(-np.pi, np.pi, size=(lanes, 4, circ.num_thetas)) * (3.0 if kind == "other" else 1.0)
    y = 0.3 * (rng.standard_normal((lanes, 1 << n)) + 1j * rng.standard_normal((lanes, 1 << n)))
    for b in range(1, lanes, 2):
        y[b, 1 << (b % n)] += 4.0
    y /= np.linalg.norm(y, axis=1, keepdims=True) / (8.0 if kind == "other" else 1.0)
    weight = rng.uniform(0.2, 0.9, size=lanes) if kind == "other" else np.ones(lanes)
    return _frozen(th, y, weight)


class _SurrogateCalls:
    """surrogate_eval four times: three with the objective's state frozen and new thetas each (the first call captures the graph, the
    next two replay it), then one that updates the state."""

    def __init__(self, circ, lanes):
        from aqc_research_amd.engine import HipContext

        self.circ, self.lanes, self.ctx = circ, lanes, HipContext(circ)
        self.flips = np.array([0] + [1 << q for q in range(circ.num_qubits)], dtype=np.int64)
        self.ws = self._create()

    def _create(self):
        from aqc_research_amd.engine import Workspace

        return Workspace(self.ctx, batch=self.lanes)

    def on(self, ws, inputs):
        from aqc_research_amd.engine import BUF_X, BUF_Y

        th, y, weight = inputs
        ws.upload(BUF_Y, y)
        ws.set_basis(BUF_X, 0)
        ws.gather_setup(self.flips)
        out = {}
        w, mx = np.array(weight), np.zeros(self.lanes, dtype=np.int64)
        for k in range(3):
            out[f"f{k}"], _, out[f"hs{k}"], out[f"g{k}"] = ws.surrogate_eval(np.ascontiguousarray(th[:, k]), w, mx, update_state=False)
        assert np.array_equal(w, weight, equal_nan=True) and not mx.any(), "a frozen state was written"
        out["g0_real"] = out["g0"].real.copy()                                 # (the surrogate's gradient: what the reference states)
        out["f3"], out["fid3"], out["hs3"], out["g3"] = ws.surrogate_eval(np.ascontiguousarray(th[:, 3]), w, mx, update_state=True)
        out["weight"], out["leading"] = w, mx
        return out

    def same(self, inputs):
        return self.on(self.ws, inputs)

    def fresh(self, inputs):
        ws = self._create()
        try:
            return self.on(ws, inputs)
        finally:
            ws.close()

    def reference(self, inputs, lane):
        """Weight 1, |state_0> leading, nothing updated: f = 1 - |h_0|^2 and the gradient Re(-2 conj(h_0) g_0)
        (test_hip_batched_optimizer.test_first_evaluation_equals_single_lane_objective states the same through the objective class)."""
        th, y, weight = (a[lane] for a in inputs)
        assert weight == 1.0
        z = orc.v_dagger_mul_vec(self.circ, th[0], y)
        x = np.zeros(1 << self.circ.num_qubits, complex)
        x[0] = 1.0
        g0 = orc.grad_of_dot_product(self.circ, th[0], x, z)
        return {"hs0": z[self.flips], "f0": 1.0 - abs(z[0]) ** 2, "g0_real": (g0 * (-2.0 * np.conj(z[0]))).real}


@pytest.mark.parametrize("lanes", (3, 65))
def test_workspace_surrogate_eval(lanes, monkeypatch):
    _set_switches(monkeypatch, {})
    n, depth = 8, 10
    calls = _SurrogateCalls(_circuit(n, "spin", depth), lanes)
    try:
        assert calls.ws.switch("AQC_GRAPH") == 1, "the evaluations replay a captured graph"
        base = check_lanes(calls.same, _surrogate_inputs(n, depth, lanes, 6000 + lanes), also=(calls.fresh,), tol=TOL, reference=calls.reference,
                           other=_surrogate_inputs(n, depth, lanes, 6100 + lanes, "other"))
        assert base["leading"].any(), "no lane leads with a flip state: the second kind of lhs state did not run"
    finally:
        calls.ws.close()


@functools.lru_cache(maxsize=None)
def _lbfgs_inputs(n, depth, lanes, seed, kind="clean"):
    """Starts and targets.  kind "other": every second lane's target is V(start)|0> itself (the lane stops at once), the others are
    far from anything the ansatz reaches from a start three times as wide (they run to the iteration limit)."""
    circ = _circuit(n, "spin", depth)
    rng = np.random.default_rng(seed)
    starts = (0.06 if kind == "other" else 0.02) * rng.standard_normal((lanes, circ.num_thetas))
    y = 0.05 * (rng.standard_normal((lanes, 1 << n)) + 1j * rng.standard_normal((lanes, 1 << n)))
    x0 = np.zeros(1 << n, complex)
    x0[0] = 1.0
    for b in range(lanes):
        if kind == "other" and b % 2 == 0:
            y[b] = orc.v_mul_vec(circ, starts[b], x0)
        elif kind == "other":
            y[b] *= 20.0
        else:
            y[b, 1 << (b % n) if b % 3 == 1 else 0] += 1.0                     # (every third lane: a flip state leads)
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    return _frozen(starts, y)


@pytest.mark.parametrize("lanes", (3, 65))
def test_device_lbfgs(lanes, monkeypatch):
    """BatchedSurrogateObjective.minimize_on_device, four iterations.  F: the neighbours' targets make them stop at once or run to the
    limit.  A lane with a non-finite value is not documented to leave the call standing, so N is not asked for."""
    from aqc_research_amd.batched_optimizer import BatchedSurrogateObjective

    _set_switches(monkeypatch, {})
    n, depth = 8, 10
    circ = _circuit(n, "spin", depth)
    nits = []

    def run(inputs):
        bo = BatchedSurrogateObjective(circ, inputs[1])
        try:
            res = bo.minimize_on_device(inputs[0], maxiter=4)
            nits.append(res["nit"].copy())
            return {"x": res["x"], "fun": res["fun"], "fidelity": res["fidelity"], "nit": res["nit"], "weight": bo.weight, "leading": bo.max_no}
        finally:
            bo.close()

    inputs = _lbfgs_inputs(n, depth, lanes, 6200 + lanes)
    base = check_lanes(run, inputs, checks="RPF", other=_lbfgs_inputs(n, depth, lanes, 6300 + lanes, "other"))
    x0 = np.zeros(1 << n, complex)
    x0[0] = 1.0
    fid = abs(np.vdot(orc.v_mul_vec(circ, base["x"][0], x0), inputs[1][0])) ** 2
    assert abs(fid - base["fidelity"][0]) < 1e-9, "lane 0: the reported point does not have the reported fidelity"
    assert base["nit"][0] == 4
    others = [l for l in range(lanes) if l not in ((0, lanes // 2, lanes - 1) if lanes > 3 else (0, lanes - 1))]
    print(f"iterations of the clean call {nits[0].tolist()}, of the call with other neighbours {nits[-1].tolist()}")
    assert {int(v) for v in nits[-1][others]} >= ({0, 4} if lanes > 3 else {4}), "the neighbours of F stop early and late"


@functools.lru_cache(maxsize=None)
def _cd_inputs(n, lanes, seed, scale=1.0):
    circ = _circuit(n, "cx", 10)
    rng = np.random.default_rng(seed)
    d = 1 << n
    th = scale * np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(lanes)])
    us = np.stack([np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0] for _ in range(lanes)])
    return _frozen(th, np.ascontiguousarray(us))


@pytest.mark.parametrize("n,route", [(4, "persistent"), (7, "wide")])
def test_workspace_cd_minimize(n, route, monkeypatch):
    """Two sweeps on five lanes: the one-launch kernel with its operands in LDS, and the wide walk.  Lane 0 follows the oracle's two
    consecutive sweeps within the bounds of tests/test_hip_cd_driver.py (1e-8 on the first value, 1e-7 on the second and on the thetas)."""
    from aqc_research_amd.engine import BUF_Y, HipContext, Workspace

    _set_switches(monkeypatch, {})
    lanes = 5
    circ = _circuit(n, "cx", 10)
    ctx = HipContext(circ)

    def on(ws, inputs):
        ws.upload(BUF_Y, inputs[1])
        res = ws.cd_minimize(inputs[0], 2, route=route, chunk=2, fobj_thr=0.0, dtheta_thr=0.0)
        return {k: res[k] for k in ("thetas", "cost", "nit", "status", "profile")}

    ws = Workspace(ctx, batch=lanes, ncols=1 << n)

    def fresh(inputs):
        other = Workspace(ctx, batch=lanes, ncols=1 << n)
        try:
            return on(other, inputs)
        finally:
            other.close()

    try:
        inputs = _cd_inputs(n, lanes, 6400 + n)
        base = check_lanes(lambda i: on(ws, i), inputs, checks="RPF", also=(fresh,), other=_cd_inputs(n, lanes, 6500 + n, 3.0))
    finally:
        ws.close()
    t1, f1 = orc.coord_descent_single_sweep(circ, inputs[0][0], inputs[1][0])
    t2, f2 = orc.coord_descent_single_sweep(circ, t1, inputs[1][0])
    assert abs(base["profile"][0, 0] - f1) < 1e-8 and abs(base["profile"][0, 1] - f2) < 1e-7 and np.max(np.abs(base["thetas"][0] - t2)) < 1e-7
    assert np.all(base["nit"] == 2) and np.all(base["status"] == 1)


def test_workspace_sketch_adam_with_rand_vectors(monkeypatch):
    """n = 5, k = 4, three lanes, three iterations.  The lane number is part of the Philox counter of a lane's sketching vectors
    (tests/sketch_ref.plane_uniforms), so a lane moved to another position draws other vectors: P does not apply, and F keeps the
    probe lanes where they are.  Lane 0 follows the CPU walk of optimizer._adam under the same draws within the 1e-9 of
    tests/test_hip_sketched.py."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.engine import HipContext, Workspace
    from tests import sketch_ref as sk

    _set_switches(monkeypatch, {})
    n, k, lanes, niter, lr, seed = 5, 4, 3, 3, 0.1, 2024
    d = 1 << n
    circ = ParametricCircuit(n, "cx", orc.spin_blocks(n, 12))
    ctx = HipContext(circ)

    def data(s, scale):
        rng = np.random.default_rng(s)
        us = np.stack([np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0] for _ in range(lanes)])
        return scale * np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(lanes)]), np.ascontiguousarray(us)

    def on(ws, inputs):
        ws.sketch_target(inputs[1])
        res = ws.sketch_adam("rand", inputs[0], niter, lr, seed=seed, reset=1)
        return {key: res[key] for key in ("x", "profile", "nit", "cost", "best_f", "best_x", "status")}

    ws = Workspace(ctx, batch=lanes, ncols=k)

    def fresh(inputs):
        other = Workspace(ctx, batch=lanes, ncols=k)
        try:
            return on(other, inputs)
        finally:
            other.close()

    try:
        inputs = data(6600, 1.0)
        base = check_lanes(lambda i: on(ws, i), inputs, checks="RF", also=(fresh,), other=data(6601, 3.0))
    finally:
        ws.close()
    assert not base["status"].any()

    def fun_grad(x, s):
        xm, ym = sk.generate(sk.SKETCH_RAND, inputs[1][0], k, om=sk.omega(sk.SKETCH_RAND, seed, s, 0, d, k))      # (evaluation s runs under sketch number iter0 + s)
        return orc.sketching_objective_and_gradient(circ, x, xm, ym)

    x_ref, prof_ref, nit_ref, _ = sk.adam_walk(fun_grad, inputs[0][0], niter, lr)
    print("lane 0: |profile - CPU walk|", np.abs(base["profile"][0] - prof_ref), "|x - x_ref|", np.max(np.abs(base["x"][0] - x_ref)))
    assert int(base["nit"][0]) == nit_ref == niter
    assert np.max(np.abs(base["profile"][0] - prof_ref)) < 1e-9 and np.max(np.abs(base["x"][0] - x_ref)) < 1e-9


# ======== the batched SVD =================================================================================================================
def test_svd_batch_with_ragged_sizes():
    """Seven matrices of 24 x 17, active in ragged leading corners.  R and P; test_hip_svd_batch.py poisons a matrix already.  Matrix
    0 is held to the bounds of that file: 8 k eps s_0 on the reconstruction, 8 k eps on the orthonormality."""
    from aqc_research_amd.mps_engine import svd_batch

    rng = np.random.default_rng(6700)
    count, m, n = 7, 24, 17
    a = rng.standard_normal((count, m, n)) + 1j * rng.standard_normal((count, m, n))
    rows = np.array([24, 17, 5, 24, 1, 16, 23], dtype=np.int32)
    cols = np.array([17, 9, 17, 1, 17, 16, 3], dtype=np.int32)

    def run(inputs):
        u, s, vh, sweeps, status = svd_batch(inputs[0], rows=inputs[1], cols=inputs[2])
        return {"u": u, "s": s, "vh": vh, "sweeps": sweeps, "status": status}

    base = check_lanes(run, (a, rows, cols), checks="RP")
    assert not base["status"].any()
    eps, k = 2.0**-52, min(m, n)
    u, s, vh = base["u"][0], base["s"][0], base["vh"][0]
    assert np.max(np.abs((u * s) @ vh - a[0])) <= 8 * k * eps * s[0]
    assert np.max(np.abs(np.conj(u.T) @ u - np.eye(k))) <= 8 * k * eps and np.max(np.abs(vh @ np.conj(vh.T) - np.eye(k))) <= 8 * k * eps
    for i in range(count):                                                      # zero outside the active corners
        ki = min(rows[i], cols[i])
        assert not base["u"][i][rows[i]:].any() and not base["u"][i][:, ki:].any() and not base["s"][i][ki:].any()
        assert not base["vh"][i][ki:].any() and not base["vh"][i][:, cols[i]:].any()


# ======== matrix-product states: measurement ==============================================================================================
@pytest.mark.parametrize("method", ("fused", "gemm"))
def test_mps_amplitudes(method, devices):
    """Three states, 70 bit strings: two workgroups of shots on the fused route."""
    from aqc_research_amd.mps_sampling import amplitudes, route

    mine, theirs = _route_profiles(method)
    states = [devices(mine, 820 + l) for l in range(3)]
    assert all(route(m.bond_dims) == method for m in states)
    bits = np.random.default_rng(6800).integers(0, 2, size=(70, _MPS_N)).astype(np.uint8)
    index = (bits.astype(np.int64) << np.arange(_MPS_N)[None, :]).sum(axis=1)
    check_lanes(lambda s: amplitudes(s, bits), states, checks="RPF", other=[devices(theirs, 830 + l) for l in range(3)], tol=TOL,
                reference=lambda s, l: _mps_dense(mine, 820 + l)[index])


@pytest.mark.parametrize("method", ("fused", "gemm"))
def test_mps_sample(method, devices):
    """Three states, 70 shots.  The lane number is part of the Philox counter, so a state moved to another lane draws other shots: P
    does not apply and is not asserted; F keeps the probe states at their positions.  Lane 0 gives the bits of the NumPy rule on every
    shot whose margin is at least tests/mps_sample_ref.MARGIN, and the amplitudes of the dense vector."""
    from aqc_research_amd.mps_sampling import route, sample
    from tests import mps_sample_ref as ref

    mine, theirs = _route_profiles(method)
    states = [devices(mine, 840 + l) for l in range(3)]
    assert all(route(m.bond_dims) == method for m in states)

    def run(s):
        got = sample(s, 70, seed=ref.PHILOX_SEED, details=True)
        return {key: got[key] for key in ("bits", "amplitudes", "probabilities", "norm2")}

    base = check_lanes(run, states, checks="RF", other=[devices(theirs, 850 + l) for l in range(3)])
    want_bits, want_amps, margin = ref.sample(_mps(mine, 840), 70, seed=ref.PHILOX_SEED)
    keep = margin >= ref.MARGIN
    assert np.count_nonzero(keep) >= 69
    assert np.array_equal(base["bits"][0][keep], want_bits[keep])
    assert np.max(np.abs(base["amplitudes"][0][keep] - want_amps[keep])) <= TOL
    assert np.max(np.abs(base["amplitudes"][0] - _mps_dense(mine, 840)[ref.indices(base["bits"][0])])) <= TOL


# ======== matrix-product states: the lockstep lanes =======================================================================================
_LOCKSTEP_BLOCKS = np.array([[0, 2, 4, 1, 3], [1, 3, 5, 2, 4]])                        # one brick layer: every bond is crossed once


@functools.lru_cache(maxsize=None)
def _lockstep_tuples(lanes, seed, low, high):
    """One random state of 6 qubits per lane, the bond caps cycling through low .. high."""
    rng = np.random.default_rng(seed)
    return tuple(orc.random_mps(6, low + b % (high - low + 1), rng) for b in range(lanes))


@pytest.mark.parametrize("truncating", (False, True), ids=("exact", "truncating"))
@pytest.mark.parametrize("lanes", (3, 129))
def test_mps_lockstep_lanes(lanes, truncating):
    """evaluate_lanes(method="lockstep") and LockstepLanes.evaluate / apply_vh / gradient on one object that is used again and again,
    as an optimisation does.

    exact: targets and lhs states are product states, whose gates produce bonds of 2, so after the first call the launches are sized
    for bonds up to 4 (8 x 4^2 elements of LDS).  F: one neighbour's target has bonds of 4; its middle gate produces a bond of 8 and
    the gradient walk's gate on sites of bonds (4, 8, 4) needs 192 elements: the lane raises kLaneLdsShort and the evaluation is
    repeated at full size.  That is seen in the count of SVDs, which is one per gate, lane and pass whatever the data.
    truncating (max_bond = 4, trunc_thr = 1e-8): targets with bonds up to 4, so the cap really truncates on the probe lanes; with the
    cap no bond outgrows a launch, the neighbours of F only differ.
    The discarded weight is a sum by atomics over the gates of a layer: it is held to (two-qubit gates) x 2^-52 relative, everything
    else exactly."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd import mps_engine as me

    n = 6
    circ = ParametricCircuit(n, entangler="cx", blocks=_LOCKSTEP_BLOCKS)
    kw = dict(trunc_thr=1e-8, max_bond=4) if truncating else {}
    rng = np.random.default_rng(6900 + lanes)
    th = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(lanes)])
    th_other = 3.0 * np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(lanes)])
    made = []

    def device(tuples):
        out = [me.DeviceMPS.from_qiskit(t) for t in tuples]
        made.extend(out)
        return out

    t_tuples = _lockstep_tuples(lanes, 6901, 2, 4) if truncating else _lockstep_tuples(lanes, 6901, 1, 1)
    l_tuples = _lockstep_tuples(lanes, 6902, 1, 2) if truncating else _lockstep_tuples(lanes, 6902, 1, 1)
    targets, lhs = device(t_tuples), device(l_tuples)
    big = lanes // 2 + 1 if lanes > 3 else 1                                   # a neighbour, never a probe
    other_t = device(_lockstep_tuples(lanes, 6903, 1, 2))
    other_t[big] = device([orc.random_mps(n, 4, np.random.default_rng(6904))])[0]
    assert int(other_t[big].bond_dims.max()) == 4 and (truncating or max(int(m.bond_dims.max()) for m in targets + lhs) == 1)
    other_l = device(_lockstep_tuples(lanes, 6905, 1, 2))
    ls = me.LockstepLanes(n, lanes)
    svds = []

    def run(inputs):
        thetas, tg, lh = inputs
        ls.set_targets(tg).set_lhs(lh)
        ls.gate2_stats(enable=True, reset=True)
        h, g, disc, bonds = ls.evaluate(circ, thetas, details=True, **kw)
        svds.append(ls.gate2_stats(enable=False)["svds"])
        amps, disc_vh, bonds_vh = ls.apply_vh(circ, thetas, flips=True, details=True, **kw)
        g_vh = ls.gradient(circ)
        hp, gp = ls.evaluate(circ, thetas, block_range=(1, 4), front_layer=False, **kw)
        he, ge = me.evaluate_lanes(circ, thetas, tg, lh, method="lockstep", **kw)
        return {"h": h, "grads": g, "discarded": disc, "bonds": bonds, "amps": amps, "discarded_vh": disc_vh, "bonds_vh": bonds_vh,
                "grads_vh": g_vh, "h_part": hp, "grads_part": gp, "h_lanes": he, "grads_lanes": ge}

    def reference(inputs, l):
        """Exact arithmetic: the dense oracle at TOL.  Truncating: the single-lane engine under the same rule at 1e-12, the reference
        and bound of test_hip_round4.test_lockstep_lanes_truncate_like_the_single_lane_engine."""
        if truncating:
            from tests.test_hip_round4 import _single_lane_reference

            h1, g1, *_ = _single_lane_reference(me, circ, inputs[0][l], inputs[1][l], inputs[2][l], **kw)
            return {"h": h1, "grads": g1, "h_lanes": h1, "grads_lanes": g1}
        x = orc.mps_to_vector(l_tuples[l])
        z = orc.v_dagger_mul_vec(circ, inputs[0][l], orc.mps_to_vector(t_tuples[l]))
        g = orc.grad_of_dot_product(circ, inputs[0][l], x, z)
        return {"h": np.vdot(x, z), "grads": g, "h_lanes": np.vdot(x, z), "grads_lanes": g}

    bound = circ.num_blocks * 2.0**-52
    try:
        base = check_lanes(run, (th, targets, lhs), checks="RPF", other=(th_other, other_t, other_l), tol=1e-12 if truncating else TOL,
                           reference=reference, rel_tol={"discarded": bound, "discarded_vh": bound},
                           distinct=("h", "grads", "amps", "grads_vh", "h_part", "grads_part"))
    finally:
        ls.close()
        for m in made:
            m.close()
    print(f"SVDs of the first evaluate per call (clean, repeat, permuted, other neighbours): {svds}")
    assert len(svds) == 4 and svds[0] == svds[1] == svds[2] > 0, svds         # clean, repeat, permuted: one pass each
    if truncating:
        assert base["bonds"].max() == 4 and base["discarded"].max() > 0.0, "the cap did not truncate"
    else:
        assert svds[3] >= svds[0] + (lanes - 1) * circ.num_blocks, f"the evaluation with the large neighbour was not repeated at full size: {svds}"
