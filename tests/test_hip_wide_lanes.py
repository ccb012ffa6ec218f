"""GPU: every batched entry point at the lane counts it accepts (the checks are tests/wide_lanes.py, which
tests/test_wide_lanes_host.py holds to planted faults).

A workspace takes 1 .. 65535 lanes, the lockstep lanes and their bank 1 .. 32767, svd_batch any count.  Every case runs its route at
the top of its range on the smallest shape that has the route, with lane l = pool member l mod 7: lanes 0 .. 6 against the feature's own
reference at its own tolerance, every other lane np.array_equal to lane l mod 7 of the same call, the call twice with the same bits.
The call objects are those of tests/test_hip_lane_contract.py; every case asserts through the workspace's introspection that the
route it names ran.  Nothing is compared between different batch sizes."""
import time

import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests.helpers import FAMILY_ENV, TOL
from tests.test_hip_lane_contract import (_SMALL, _BasisCalls, _DenseCalls, _SurrogateCalls, _basis_inputs, _cd_inputs, _circuit, _dense_inputs,
                                          _frozen, _lbfgs_inputs, _set_switches, _surrogate_inputs)
from tests.wide_lanes import POOL, Wide, check_wide, probe_lanes

pytestmark = pytest.mark.gpu

WS_MAX = 65535           # aqc_ws_create: batch in [1, 65535]
LOCKSTEP_MAX = 32767     # aqc_mpsb_create, aqc_mpsb_set_bank: lanes / count in [1, 32767]
PAST_THE_GRID = 65538
EPS = 2.0**-52


def _live():
    from aqc_research_amd.engine import live_buffers

    return live_buffers()


def _device_memory():
    """Free bytes of the current device, from the HIP runtime the library is linked to."""
    import ctypes

    from aqc_research_amd import _lib

    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    fn = _lib.lib().hipMemGetInfo
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    assert fn(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


class _Clock:
    def __init__(self, what):
        self.what, self.t0 = what, time.perf_counter()

    def done(self, extra=""):
        print(f"{self.what}: {time.perf_counter() - self.t0:.1f} s{extra}")


# ======== a. dense routes at 65535 lanes ==================================================================================================
@pytest.mark.parametrize("n,kind,depth,family", [(6, "cp", 10, "per-group"), (6, "trotter2", 2, "register-blocked"), (8, "cx", 12, None)])
def test_workspace_dense_calls_at_65535_lanes(n, kind, depth, family, monkeypatch):
    """The whole _DenseCalls.on sequence, every output of every lane (the largest buffer: 65535 x 2^8 x 16 B = 268 MB)."""
    _set_switches(monkeypatch, {} if family is None else {"AQC_KERNEL_FAMILY": FAMILY_ENV[family]})
    clock = _Clock(f"dense calls, {n} qubits {kind} {family}, {WS_MAX} lanes")
    calls = _DenseCalls(_circuit(n, kind, depth), WS_MAX)
    try:
        want = 3 if family is None else int(FAMILY_ENV[family])
        if family is not None:
            assert calls.ws.switch("AQC_KERNEL_FAMILY") == want
        assert calls.ws.kernel_family(1) == want and calls.ws.kernel_family(0) == want
        check_wide(lambda wide: calls.same(wide.full()), WS_MAX, _dense_inputs(n, kind, depth, POOL, 7000 + n), reference=calls.reference, tol=TOL)
        assert calls.ws.sparse_counts() == (-1, -1, -1), "dense lhs states take the dense route"
    finally:
        calls.ws.close()
    clock.done()


# ======== b. the projected route where 2 x lanes passes 65536 =============================================================================
class _BroadcastBasisCalls(_BasisCalls):
    """_BasisCalls with one target for all lanes, handed in by broadcast (13 qubits at these counts: 4 GiB per buffer); the lanes differ
    in their thetas and in the tile of their basis state.  The inputs keep the structure of _BasisCalls, the target column only read
    at its first lane."""

    def on(self, ws, inputs):
        from aqc_research_amd.engine import BUF_X, BUF_Y

        th, y, basis = inputs
        out = {}
        ws.broadcast(BUF_Y, y[0])
        ws.set_basis(BUF_X, basis)
        ws.gather_setup(self.gather)
        out["amps0"], out["grads0"] = ws.eval(np.ascontiguousarray(th[:, 0]), gather=True)
        out["amps1"], out["grads1"] = ws.eval(np.ascontiguousarray(th[:, 1]), gather=True)
        ws.set_thetas(np.ascontiguousarray(th[:, 0]))
        ws.objective_launch(BUF_X)
        out["amps_launch"], out["grads_launch"] = ws.gather_fetch(), ws.get_grads()
        return out


def _launch_counts(calls, inputs):
    """Launches of one objective_launch by kind, from the workspace's profile: (projection passes, virtual sweep stages, applications of
    the virtual plan).  The objective by projection applies the virtual plan at least twice and V^H by its stages never; a projection
    pass is the fused pass (one per evaluation), its two-launch form (two), or the sweep's projection of the checkpoint (one)."""
    from aqc_research_amd._lib import K_APPLY_VIRTUAL, K_PROJECT, K_SWEEP_VIRTUAL
    from aqc_research_amd.engine import BUF_X

    calls.on(calls.ws, inputs)
    calls.ws.profile(True)
    calls.ws.objective_launch(BUF_X)
    calls.ws.sync()
    counts = tuple(calls.ws.profile_get(kind)[0] for kind in (K_PROJECT, K_SWEEP_VIRTUAL, K_APPLY_VIRTUAL))
    calls.ws.profile(False)
    return counts


# The launches of the route that carry two items per lane (aqc_project.hip), and the case that reaches each.  The fused pass has its
# items in grid.x; project_staged_kernel, project_kernel, project_sum_kernel and project_csum_kernel take theirs from grid.y, one launch
# per 65535 items: at 32768 lanes the second launch has one item, at 32769 three.
#   (qubits, depth, tile, switches beside _SMALL, what the plan must say, projection passes per objective_launch, objective by projection)
_DOUBLING_CASES = {
    # the fused pass alone (summed_bits 8: one part; more than 512 lanes: one share)
    "fused": (12, 19, 10, {}, {"summed_bits": 8}, 1, True),
    "fused-no-pair-launches": (12, 19, 10, {"AQC_PROJECTED_PAIRS": "0"}, {"summed_bits": 8}, 1, True),
    # both products as launches of their own: project_staged_kernel (the projection) and project_kernel (the lhs tile)
    "two-launches": (12, 19, 10, {"AQC_PROJECTED_FUSED": "0"}, {"summed_bits": 8}, 2, True),
    # V^H by its stages: the sweep projects the checkpoint itself (run_projected_stages: project_staged_kernel)
    "sweep-alone": (12, 19, 10, {"AQC_PROJECTED_VDAG": "0"}, {"summed_bits": 8}, 1, False),
    # 2^9 summed values: the fused pass leaves two partial projections per item, project_sum_kernel adds them
    "fused-two-parts": (13, 11, 10, {}, {"summed_bits": 9}, 1, True),
    # five touched qubits and a workgroup target above the batch: the fused pass splits its walk in two shares (proj_alloc: the
    # largest power of two with 2 shares <= 2^(touched - 4)), project_csum_kernel adds them
    "fused-two-shares": (13, 19, 10, {"AQC_PROJECTED_FUSED_WGS": "70000"}, {"summed_bits": 8, "touched_qubits": 5}, 1, True),
}


@pytest.mark.parametrize("case", sorted(_DOUBLING_CASES))
@pytest.mark.parametrize("lanes", (32768, 32769))
def test_workspace_projected_route_at_the_doubling(lanes, case, monkeypatch):
    """The route's launches carry 2 x lanes items, 65536 and 65538 here.  Two evaluations, the second replaying the captured graph,
    then objective_launch; amplitudes and gradients of all lanes.  The 13-qubit shapes take one broadcast target (4 GiB per buffer).
    Which launches ran: the switches as the workspace read them, the plan's sizes (they decide the parts and the shares, see
    _DOUBLING_CASES), and the profile of one objective_launch."""
    n, depth, tile, extra, plan, passes, by_projection = _DOUBLING_CASES[case]
    env = dict(_SMALL, **extra)
    _set_switches(monkeypatch, {})
    monkeypatch.delenv("AQC_PROJECTED_FUSED_WGS", raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    need, free = 48 << 30, _device_memory()                                   # (13 qubits: six buffers of 4 GiB, the virtual registers, the shares)
    if n > 12 and free < need:
        pytest.skip(f"{need / 2**30:.1f} GiB of device memory needed, {free / 2**30:.1f} GiB free")
    clock = _Clock(f"projected route, {case}, {lanes} lanes")
    calls = (_BasisCalls if n == 12 else _BroadcastBasisCalls)(_circuit(n, "spin", depth), lanes, tile)
    try:
        for name, val in env.items():
            assert calls.ws.switch(name) == int(val)
        assert calls.ws.switch("AQC_PROJECTED_FUSED_MAX_SHARES") >= 2 and (case == "fused-two-shares" or calls.ws.switch("AQC_PROJECTED_FUSED_WGS") < lanes)
        info = calls.ws.projected_info()
        assert info, "the shape was chosen for the route by projection"
        assert all(info[key] == val for key, val in plan.items()) and info["shared_with_first_stage"] <= 4, info
        pool = _basis_inputs(n, depth, tile, POOL, 7100 + n)
        if n > 12:
            pool = (pool[0], np.repeat(pool[1][:1], POOL, axis=0), pool[2])
        assert len(set((pool[2] >> tile).tolist())) > 1, "the basis states lie in different tiles"
        wide = Wide(lanes, pool)
        full = _frozen(*wide.full()) if n == 12 else _frozen(wide.column(0), pool[1], wide.column(2))   # (12 qubits: 2 GB of targets, built once)
        check_wide(lambda _: calls.same(full), lanes, pool, reference=calls.reference, tol=TOL)
        assert calls.ws.sparse_counts()[0] > 0, "the sparse route did not run"
        projections, virtual_sweeps, virtual_applies = _launch_counts(calls, full)
        assert projections == passes, (projections, virtual_sweeps, virtual_applies)
        assert (virtual_applies >= 2) if by_projection else (virtual_applies == 0), "objective by projection / V^H by its stages"
    finally:
        calls.ws.close()
    clock.done(f"; (projection passes, virtual sweep stages, virtual applications) = {(projections, virtual_sweeps, virtual_applies)}")


# ======== c, e. the persistent 2^12 kernels at 65535 lanes; a buffer past 4 GiB ===========================================================
class _LeanDenseCalls:
    """The sequence of _DenseCalls.on where a full array of states cannot exist on the host: the target and the lhs state go in by
    broadcast of one state plus upload_lane on the probe lanes, whole states come back from the probe lanes only (download of a lane),
    and every lane is read through gathered amplitudes and gradients.  The pooled lanes differ in their thetas."""

    def __init__(self, circ, lanes):
        from aqc_research_amd.engine import HipContext, Workspace

        self.circ, self.lanes = circ, lanes
        n = circ.num_qubits
        self.flips = np.array([0] + [1 << q for q in range(n)] + [(1 << n) - 1], dtype=np.int64)
        before = _device_memory()
        self.ws = Workspace(HipContext(circ), batch=lanes)
        self.bytes = before - _device_memory()

    def on(self, wide, x0, y0):
        from aqc_research_amd.engine import BUF_X, BUF_Y, BUF_Z

        ws = self.ws
        th = wide.column(0)
        ws.set_thetas(th)
        ws.broadcast(BUF_Y, y0)
        ws.broadcast(BUF_X, x0)
        for j, l in enumerate(wide.probe_lanes):
            ws.upload(BUF_X, wide.probe_inputs[1][j], lane=l)
            ws.upload(BUF_Y, wide.probe_inputs[2][j], lane=l)
        out = {}
        ws.apply(True, BUF_Y, BUF_Z)
        out["vdag_amps"] = ws.gather(BUF_Z, self.flips)
        out["probe:vdag_y"] = np.stack([ws.download(BUF_Z, lane=l) for l in wide.probe_lanes])
        ws.apply(False, BUF_X, BUF_Z)
        out["v_amps"] = ws.gather(BUF_Z, self.flips)
        out["probe:v_x"] = np.stack([ws.download(BUF_Z, lane=l) for l in wide.probe_lanes])
        ws.gather_setup(self.flips)
        out["amps"], out["grads"] = ws.eval(th, vdag=True, gather=True, grad=True)
        _, out["grads_part"] = ws.eval(th, vdag=False, gather=False, grad=True, block_range=(1, self.circ.num_blocks - 1), front_layer=False)
        out["amps_only"], _ = ws.eval(None, vdag=True, gather=True, grad=False)
        return out

    def reference(self, inputs, lane):
        th, x, y = (a[lane] for a in inputs)
        z, vx = orc.v_dagger_mul_vec(self.circ, th, y), orc.v_mul_vec(self.circ, th, x)
        return {"probe:vdag_y": z, "probe:v_x": vx, "vdag_amps": z[self.flips], "v_amps": vx[self.flips], "amps": z[self.flips],
                "amps_only": z[self.flips], "grads": orc.grad_of_dot_product(self.circ, th, x, z),
                "grads_part": orc.grad_of_dot_product(self.circ, th, x, z, (1, self.circ.num_blocks - 1), False)}


# (qubits, lanes, device memory the case asks for: the workspace measured 33 783 021 568 and 32 235 323 392 bytes, rounded up to a GiB)
_LEAN_CASES = {"2^12-at-65535": (12, WS_MAX, 32 << 30), "buffer-past-4GiB": (13, 32769, 31 << 30)}


@pytest.mark.parametrize("case", sorted(_LEAN_CASES))
def test_workspace_dense_calls_on_large_buffers(case, monkeypatch):
    """2^12-at-65535: the persistent 2^12-tile kernels at the largest batch, buffers of 4 GiB - 64 KiB.  buffer-past-4GiB: 13 qubits at
    32769 lanes, 4 GiB + 128 KiB per buffer, the smallest shape and count beyond 4 GiB: the byte offsets of lanes 32767 and 32768
    pass 2^32.  cx, depth 14.  The probe lanes 0, 1, 32766 .. 32769 and the last two carry states and thetas of their own and are
    held to the oracle with their whole states; every other lane has the broadcast state and the thetas of pool member l mod 7."""
    n, lanes, need = _LEAN_CASES[case]
    kind, depth = "cx", 14
    _set_switches(monkeypatch, {})
    free = _device_memory()
    if free < need:
        pytest.skip(f"{need / 2**30:.1f} GiB of device memory needed, {free / 2**30:.1f} GiB free")
    clock = _Clock(f"dense calls on large buffers, {n} qubits, {lanes} lanes")
    circ = _circuit(n, kind, depth)
    calls = _LeanDenseCalls(circ, lanes)
    try:
        assert calls.bytes <= need, f"the workspace took {calls.bytes} bytes, the test asks for {need} free"
        assert calls.ws.kernel_family(1) == 3 and calls.ws.kernel_family(0) == 3
        plans = calls.ws.plan_info(1), calls.ws.plan_info(0)
        assert plans[0][1] == 12 and plans[1][1] == 12, "the persistent kernels run on 2^12 tiles"
        assert (plans[0][0] > 1) == (n > 12), "13 qubits need more than one stage of 2^12 tiles"
        buffer_bytes = lanes * (16 << n)
        assert (buffer_bytes > 1 << 32) == (n == 13) and abs(buffer_bytes - (1 << 32)) <= 128 << 10
        where = probe_lanes(lanes)
        pool = _dense_inputs(n, kind, depth, POOL, 7200 + n)
        pool = (pool[0], np.repeat(pool[1][:1], POOL, axis=0), np.repeat(pool[2][:1], POOL, axis=0))   # one state, seven theta draws
        own = _dense_inputs(n, kind, depth, len(where), 7300 + n)
        check_wide(lambda wide: calls.on(wide, pool[1][0], pool[2][0]), lanes, pool, probes=(where, own), reference=calls.reference, tol=TOL)
        assert calls.ws.sparse_counts() == (-1, -1, -1), "dense lhs states take the dense route"
    finally:
        calls.ws.close()
    clock.done(f"; workspace {calls.bytes / 2**30:.2f} GiB ({calls.bytes} bytes), plans (stages, tile bits, ..) {plans}")


# ======== d. the callers that ride on the workspace batch =================================================================================
def test_workspace_surrogate_eval_at_65535_lanes(monkeypatch):
    _set_switches(monkeypatch, {})
    n, depth = 8, 10
    clock = _Clock(f"surrogate_eval, {WS_MAX} lanes")
    calls = _SurrogateCalls(_circuit(n, "spin", depth), WS_MAX)
    try:
        assert calls.ws.switch("AQC_GRAPH") == 1, "the evaluations replay a captured graph"
        assert calls.ws.kernel_family(1) == 3
        base = check_wide(lambda wide: calls.same(wide.full()), WS_MAX, _surrogate_inputs(n, depth, POOL, 7400), reference=calls.reference, tol=TOL,
                          distinct=[f"{k}{i}" for k in ("f", "hs", "g") for i in range(4)])
        assert base["leading"].any(), "no lane leads with a flip state: the second kind of lhs state did not run"
    finally:
        calls.ws.close()
    clock.done()


def test_device_lbfgs_at_65535_lanes(monkeypatch):
    """BatchedSurrogateObjective.minimize_on_device, three iterations; lanes 0 .. 6: the reported point has the reported fidelity."""
    from aqc_research_amd.batched_optimizer import BatchedSurrogateObjective

    _set_switches(monkeypatch, {})
    n, depth = 8, 10
    circ = _circuit(n, "spin", depth)
    clock = _Clock(f"device L-BFGS, {WS_MAX} lanes")

    def run(wide):
        starts, y = wide.full()
        bo = BatchedSurrogateObjective(circ, y)
        try:
            assert bo.ws.batch == WS_MAX and bo.ws.kernel_family(1) == 3
            res = bo.minimize_on_device(starts, maxiter=3)
            return {"x": res["x"], "fun": res["fun"], "fidelity": res["fidelity"], "nit": res["nit"], "weight": bo.weight, "leading": bo.max_no}
        finally:
            bo.close()

    pool = _lbfgs_inputs(n, depth, POOL, 7500)
    base = check_wide(run, WS_MAX, pool, distinct=("x", "fun", "fidelity"))
    x0 = np.zeros(1 << n, complex)
    x0[0] = 1.0
    for k in range(POOL):
        fid = abs(np.vdot(orc.v_mul_vec(circ, base["x"][k], x0), pool[1][k])) ** 2
        assert abs(fid - base["fidelity"][k]) < 1e-9, f"lane {k}: the reported point does not have the reported fidelity"
    assert base["nit"][0] == 3
    clock.done()


def test_workspace_cd_minimize_at_65535_lanes(monkeypatch):
    """The one-launch kernel with its operands in LDS at 3 qubits (ncols = 8), two sweeps; lanes 0 .. 6 follow the oracle's two
    consecutive sweeps within the bounds of tests/test_hip_cd_driver.py (1e-8 on the first value, 1e-7 on the second and the thetas).
    The route is an argument of the call (route="persistent" is refused where it cannot run); there is nothing to introspect."""
    from aqc_research_amd.engine import BUF_Y, HipContext, Workspace

    _set_switches(monkeypatch, {})
    n = 3
    circ = _circuit(n, "cx", 10)
    clock = _Clock(f"cd_minimize (persistent), {WS_MAX} lanes")
    ws = Workspace(HipContext(circ), batch=WS_MAX, ncols=1 << n)

    def run(wide):
        th, us = wide.full()
        ws.upload(BUF_Y, us)
        res = ws.cd_minimize(th, 2, route="persistent", chunk=2, fobj_thr=0.0, dtheta_thr=0.0)
        return {"thetas": res["thetas"], "cost": res["cost"], "nit": res["nit"], "status": res["status"], "f1": res["profile"][:, 0],
                "f2": res["profile"][:, 1]}

    def reference(inputs, k):
        t1, f1 = orc.coord_descent_single_sweep(circ, inputs[0][k], inputs[1][k])
        t2, f2 = orc.coord_descent_single_sweep(circ, t1, inputs[1][k])
        return {"f1": f1, "f2": f2, "thetas": t2}

    try:
        base = check_wide(run, WS_MAX, _cd_inputs(n, POOL, 7600), reference=reference, tol={"f1": 1e-8, "f2": 1e-7, "thetas": 1e-7})
    finally:
        ws.close()
    assert np.all(base["nit"] == 2) and np.all(base["status"] == 1)
    clock.done()


def test_workspace_sketch_adam_at_65535_lanes(monkeypatch):
    """(n, k) = (3, 2), cz, depth 6 (tests/test_hip_sketched.ADAM_CASES["n3"]), three iterations under the alt sketch, whose index
    sequence is an input of the lane (the rand sketch draws from the lane number, so its lanes differ by design).  Lanes 0 .. 6
    follow the CPU walk of optimizer._adam under the same sketches within the 1e-9 of that file.  sketch_adam has one route, named by
    the kind of sketch in the call; the workspace's introspection has nothing on it."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.engine import HipContext, Workspace
    from tests import sketch_ref as sk

    _set_switches(monkeypatch, {})
    n, k, niter, lr = 3, 2, 3, 0.1
    d = 1 << n
    circ = ParametricCircuit(n, "cz", orc.spin_blocks(n, 6))
    rng = np.random.default_rng(7700)
    us = np.stack([np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0] for _ in range(POOL)])
    th = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(POOL)])
    idx = np.stack([np.stack([rng.permutation(d)[:k] for _ in range(niter + 1)]) for _ in range(POOL)]).astype(np.int32)      # [lane][evaluation][k]
    clock = _Clock(f"sketch_adam, {WS_MAX} lanes")
    ws = Workspace(HipContext(circ), batch=WS_MAX, ncols=k)

    def run(wide):
        x0, targets, index = wide.full()
        ws.sketch_target(targets)
        res = ws.sketch_adam("alt", x0, niter, lr, alt_idx=np.ascontiguousarray(index.transpose(1, 0, 2)), reset=1)
        return {key: res[key] for key in ("x", "profile", "nit", "cost", "best_f", "best_x", "status")}

    def reference(inputs, lane):
        def fun_grad(x, s):
            xm, ym = sk.generate(sk.SKETCH_ALT, inputs[1][lane], k, idx=inputs[2][lane][s - 1])
            return orc.sketching_objective_and_gradient(circ, x, xm, ym)

        x_ref, prof_ref, nit_ref, _ = sk.adam_walk(fun_grad, inputs[0][lane], niter, lr)
        assert nit_ref == niter
        return {"x": x_ref, "profile": prof_ref}

    try:
        base = check_wide(run, WS_MAX, (th, np.ascontiguousarray(us), idx), reference=reference, tol=1e-9)
    finally:
        ws.close()
    assert not base["status"].any() and np.all(base["nit"] == niter)
    clock.done()


# ======== f. the lockstep lanes and their bank ============================================================================================
_LOCKSTEP_BLOCKS = np.array([[0, 1, 0], [1, 2, 1]])                                    # 3 qubits: every bond is crossed, one of them twice


def test_mps_lockstep_lanes_at_32767_lanes():
    """LockstepLanes on 3 qubits at its largest lane count, in exact arithmetic (product states in, bonds of 2 at the most): the gates
    (evaluate), V^H with the flip amplitudes, the gradient, a partial block range, and export of the working state on the lanes at
    both ends and on either side of 16384 and 32766.  Lanes 0 .. 6 against the dense oracle at TOL.  The lockstep lanes are one
    route, chosen by constructing LockstepLanes; the bonds reported (at most 2) say that no lane left it for the full-size repeat."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd import mps_engine as me

    n, lanes = 3, LOCKSTEP_MAX
    circ = ParametricCircuit(n, entangler="cx", blocks=_LOCKSTEP_BLOCKS)
    rng = np.random.default_rng(7800)
    th = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(POOL)])
    t_tuples = [orc.random_mps(n, 1, rng) for _ in range(POOL)]
    l_tuples = [orc.random_mps(n, 1, rng) for _ in range(POOL)]
    targets, lhs = [me.DeviceMPS.from_qiskit(t) for t in t_tuples], [me.DeviceMPS.from_qiskit(t) for t in l_tuples]
    exported = (0, 1, 2, 3, 4, 5, 6, 16383, 16384, lanes - 2, lanes - 1)
    clock = _Clock(f"lockstep lanes, {lanes} lanes")
    ls = me.LockstepLanes(n, lanes)

    def run(wide):
        thetas, tg, lh = wide.full()
        ls.set_targets(tg).set_lhs(lh)
        h, g, disc, bonds = ls.evaluate(circ, thetas, details=True)
        amps, disc_vh, bonds_vh = ls.apply_vh(circ, thetas, flips=True, details=True)
        g_vh = ls.gradient(circ)
        hp, gp = ls.evaluate(circ, thetas, block_range=(1, 2), front_layer=False)
        ls.apply_circuit(circ, thetas, inverse=True)
        out = {"h": h, "grads": g, "discarded": disc, "bonds": bonds, "amps": amps, "discarded_vh": disc_vh, "bonds_vh": bonds_vh,
               "grads_vh": g_vh, "h_part": hp, "grads_part": gp}
        states = []
        for l in exported:
            m = ls.export(l)
            try:
                states.append(np.asarray(m.to_vector()).reshape(-1))
            finally:
                m.close()
        return out, np.stack(states)

    def reference(inputs, l):
        x = orc.mps_to_vector(l_tuples[l])
        z = orc.v_dagger_mul_vec(circ, inputs[0][l], orc.mps_to_vector(t_tuples[l]))
        g = orc.grad_of_dot_product(circ, inputs[0][l], x, z)
        flips = [np.vdot(x[np.arange(1 << n) ^ (1 << q)], z) for q in range(n)]          # <X_q lhs|V^H target>: index bit q <-> site q
        return {"h": np.vdot(x, z), "grads": g, "grads_vh": g, "amps": np.array([np.vdot(x, z)] + flips),
                "grads_part": orc.grad_of_dot_product(circ, inputs[0][l], x, z, (1, 2), False)}

    states = []

    def all_lanes(wide):
        out, st = run(wide)
        states.append(st)
        return out

    bound = circ.num_blocks * EPS
    try:
        check_wide(all_lanes, lanes, (th, targets, lhs), reference=reference, tol=TOL, rel_tol={"discarded": bound, "discarded_vh": bound},
                   distinct=("h", "grads", "amps", "grads_vh", "h_part", "grads_part"))
    finally:
        ls.close()
        for m in targets + lhs:
            m.close()
    assert np.array_equal(states[0], states[1]), "the exported states of the two calls differ"
    for i, l in enumerate(exported):
        k = l % POOL
        if l >= POOL:
            assert np.array_equal(states[0][i], states[0][k]), f"export of lane {l} differs from lane {k}"
        else:
            z = orc.v_dagger_mul_vec(circ, th[k], orc.mps_to_vector(t_tuples[k]))
            assert np.max(np.abs(states[0][i] - z)) <= TOL, f"export of lane {l}"
    clock.done()


@pytest.mark.parametrize("count,lanes", [(LOCKSTEP_MAX, 1), (2, LOCKSTEP_MAX)])
def test_mps_lockstep_bank(count, lanes):
    """apply_vh_bank: a bank of 32767 states against one lane (the bank states are the pooled axis), and a bank of two states against
    32767 lanes.  amps[l][k] = <bank_k|V^H target_l> against the dense oracle at TOL on the first seven of the pooled axis.  One route,
    named by the call."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd import mps_engine as me

    n = 3
    circ = ParametricCircuit(n, entangler="cx", blocks=_LOCKSTEP_BLOCKS)
    rng = np.random.default_rng(7900 + lanes)
    th = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(POOL)])
    t_tuples = [orc.random_mps(n, 1, rng) for _ in range(POOL)]
    b_tuples = [orc.random_mps(n, 2, rng) for _ in range(POOL)]
    targets, bank = [me.DeviceMPS.from_qiskit(t) for t in t_tuples], [me.DeviceMPS.from_qiskit(t) for t in b_tuples]
    t_vec, b_vec = [orc.mps_to_vector(t) for t in t_tuples], [orc.mps_to_vector(t) for t in b_tuples]
    clock = _Clock(f"lockstep bank of {count} states, {lanes} lanes")
    live = _live()
    ls = me.LockstepLanes(n, lanes)

    def run_bank(wide):                                                        # one lane (target 0, thetas 0), the bank pooled
        ls.set_targets([targets[0]]).set_bank(wide.column(0))
        return {"amps": ls.apply_vh_bank(circ, th[:1])[0]}

    def run_lanes(wide):                                                       # the lanes pooled, bank states 0 and 1
        thetas, tg = wide.full()
        ls.set_targets(tg).set_bank(bank[:2])
        amps, disc, bonds = ls.apply_vh_bank(circ, thetas, details=True)
        return {"amps": amps, "grads": ls.set_lhs(tg).gradient(circ), "bonds": bonds}

    try:
        if lanes == 1:
            z0 = orc.v_dagger_mul_vec(circ, th[0], t_vec[0])
            check_wide(run_bank, count, [bank], reference=lambda inputs, k: {"amps": np.vdot(b_vec[k], z0)}, tol=TOL)
        else:
            def reference(inputs, l):
                z = orc.v_dagger_mul_vec(circ, inputs[0][l], t_vec[l])
                return {"amps": np.array([np.vdot(b_vec[0], z), np.vdot(b_vec[1], z)]), "grads": orc.grad_of_dot_product(circ, inputs[0][l], t_vec[l], z)}

            check_wide(run_lanes, lanes, (th, targets), reference=reference, tol=TOL)
    finally:
        ls.close()
        assert _live() == live
        for m in targets + bank:
            m.close()
    clock.done()


# ======== g. counts without a stated limit ================================================================================================
def test_svd_batch_past_the_grid():
    """65538 matrices in a store of 3 x 2, active in ragged corners from 1 x 1 to 3 x 2.  The first seven against numpy.linalg.svd
    within the bounds of tests/test_hip_svd_batch.py: 8 k eps s_0 on the spectrum and on the reconstruction, 8 k eps on the
    orthonormality (k = 2, the store's)."""
    from aqc_research_amd.mps_engine import svd_batch

    rng = np.random.default_rng(8000)
    m, n, k = 3, 2, 2
    a = rng.standard_normal((POOL, m, n)) + 1j * rng.standard_normal((POOL, m, n))
    rows = np.array([3, 1, 2, 3, 1, 2, 3], dtype=np.int32)
    cols = np.array([2, 1, 2, 1, 2, 1, 2], dtype=np.int32)
    clock = _Clock(f"svd_batch, {PAST_THE_GRID} matrices")

    def run(wide):
        store, r, c = wide.full()
        u, s, vh, sweeps, status = svd_batch(store, rows=r, cols=c)
        return {"u": u, "s": s, "vh": vh, "sweeps": sweeps, "status": status}

    base = check_wide(run, PAST_THE_GRID, (a, rows, cols), distinct=("u", "s"))            # (vh of a one-column matrix is 1 whatever the column)
    assert not base["status"].any()
    for i in range(POOL):
        r, c = rows[i], cols[i]
        ki = min(r, c)
        u, s, vh = base["u"][i], base["s"][i], base["vh"][i]
        s_ref = np.linalg.svd(a[i, :r, :c], compute_uv=False)
        bound = 8 * k * EPS * s_ref[0]
        assert np.all(np.diff(s[:ki]) <= 0) and np.max(np.abs(s[:ki] - s_ref)) <= bound, i
        assert np.max(np.abs((u[:r, :ki] * s[:ki]) @ vh[:ki, :c] - a[i, :r, :c])) <= bound, i
        assert np.max(np.abs(np.conj(u[:r, :ki].T) @ u[:r, :ki] - np.eye(ki))) <= 8 * k * EPS, i
        assert np.max(np.abs(vh[:ki, :c] @ np.conj(vh[:ki, :c].T) - np.eye(ki))) <= 8 * k * EPS, i
        assert not u[r:].any() and not u[:, ki:].any() and not s[ki:].any() and not vh[ki:].any() and not vh[:, c:].any(), i
    clock.done()


# ======== h. refusals =====================================================================================================================
@pytest.mark.parametrize("batch", (0, WS_MAX + 1))
def test_workspace_refuses_a_batch_outside_its_range(batch):
    from aqc_research_amd.engine import HipContext, Workspace

    ctx = HipContext(_circuit(6, "cx", 10))
    live = _live()
    with pytest.raises(RuntimeError, match=r"\[1, 65535\]"):
        Workspace(ctx, batch=batch)
    assert _live() == live


def test_lockstep_lanes_refuse_counts_outside_their_range():
    from aqc_research_amd import mps_engine as me

    live = _live()
    for lanes in (0, LOCKSTEP_MAX + 1):
        with pytest.raises(RuntimeError, match=r"\[1, 32767\]"):
            me.LockstepLanes(3, lanes)
        assert _live() == live
    state = me.DeviceMPS.from_qiskit(orc.random_mps(3, 1, np.random.default_rng(8100)))
    ls = me.LockstepLanes(3, 1)
    try:
        held = _live()
        for count in (0, LOCKSTEP_MAX + 1):
            with pytest.raises(RuntimeError, match=r"bank: count must be in \[1, 32767\]"):
                ls.set_bank([state] * count)
            assert _live() == held
    finally:
        ls.close()
        state.close()
    assert _live() == live
