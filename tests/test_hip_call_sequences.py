"""GPU: call sequences on one long-lived workspace, checked against the shadow model of tests/ws_model.py.

The skipping the workspace does (partial Z, the checkpoint in ZW, the tile lists of the sparse route, the projected route's
virtual pattern, the graph cache) is decided from host-side bookkeeping that lives across calls.  The tests below interleave
the call kinds of include/aqc_hip.h the way the objectives, the device L-BFGS and the drivers do, and compare every read
with the oracle (1e-10) and, read for read, across route configurations (1e-12).
"""
import numpy as np
import pytest

from oracle import aqc_oracle as orc
from tests import ws_model as wm
from tests.ws_model import BUF_X, BUF_X2, BUF_Y, BUF_Z, BUF_ZW

pytestmark = pytest.mark.gpu

SWITCHES = ("AQC_SPARSE_MIN_ITEMS", "AQC_PROJECTED_VDAG_MIN_ELEMS", "AQC_PROJECTED", "AQC_LAZY_Z", "AQC_SPARSE_SWEEP",
            "AQC_KERNEL_FAMILY", "AQC_PROJECTED_VDAG")
FORCED = {"AQC_SPARSE_MIN_ITEMS": "1", "AQC_PROJECTED_VDAG_MIN_ELEMS": "1"}
CONFIGS = {
    "default": {},
    "forced": FORCED,
    "forced_noproj": dict(FORCED, AQC_PROJECTED="0"),
    "forced_nolazy": dict(FORCED, AQC_LAZY_Z="0"),
    "dense_sweep": dict(FORCED, AQC_SPARSE_SWEEP="0"),
}


def _pc(n, ent, depth):
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    return ParametricCircuit(n, ent, create_ansatz_structure(n, "spin", "full", depth))


def _trotter(n, layers):
    from aqc_research_amd import TrotterAnsatz
    from aqc_research_amd.circuit_structures import make_trotter_like_circuit

    return TrotterAnsatz(n, make_trotter_like_circuit(n, layers), second_order=True)


# name -> (circuit, tile bits, lanes): sweep plans of 2 and >= 3 stages, a 2nd-order Trotter ansatz, projected plans with one
# and with two virtual stages (HipContext.plan_projected)
SHAPES = {
    "cx12_t10": (lambda: _pc(12, "cx", 18), 10, 3),
    "cz13_t8": (lambda: _pc(13, "cz", 20), 8, 4),
    "trotter13_t10": (lambda: _trotter(13, 1), 10, 4),
    "cp14_t9": (lambda: _pc(14, "cp", 22), 9, 5),
    "cx16_t9": (lambda: _pc(16, "cx", 24), 9, 3),
}
_CACHE = {}


def _shape(name):
    if name not in _CACHE:
        from aqc_research_amd.engine import HipContext

        make, tile, batch = SHAPES[name]
        circ = make()
        _CACHE[name] = (circ, HipContext(circ), tile, batch, wm.Oracle(circ))
    return _CACHE[name]


def _configure(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _maker(ctx, batch, tile):
    from aqc_research_amd.engine import Workspace

    return lambda: Workspace(ctx, batch=batch, tile_bits_apply=tile, tile_bits_sweep=tile)


def _run(monkeypatch, shape, env, ops):
    circ, ctx, tile, batch, oracle = _shape(shape)
    _configure(monkeypatch, env)
    return wm.run_sequence(_maker(ctx, batch, tile), circ, batch, ops, oracle)


def _opening(circ, batch, rng, x_idx, gather):
    th = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(batch)])
    return [("upload", {"buf": BUF_Y, "data": np.stack([orc.rand_state(circ.num_qubits, rng) for _ in range(batch)])}),
            ("set_basis", {"buf": BUF_X, "idx": x_idx}),
            ("gather_setup", {"idx": gather}),
            ("set_thetas", {"th": th})]


def _launch():
    return [("objective_launch", {"x": BUF_X, "br": None, "front": True}), ("results", {"kind": "async"})]


# ---- regression sequences ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("replay", ["surrogate_eval", "eval"])
@pytest.mark.parametrize("projected", ["1", "0"])
def test_replay_between_objective_launches_leaves_no_stale_list(monkeypatch, replay, projected):
    """aqc_ws_sweep.cpp run_vdag_restricted (vd_key) and aqc_ws_project.cpp ensure_pattern (proj.init_buf): a replayed graph
    rebuilds V^H's last-stage tile list and the virtual pattern on the device; the next objective_launch must not take them
    as built for its own lhs state.  The lhs state sits in a tile outside the gather set's."""
    circ, _, tile, batch, _ = _shape("cx12_t10")
    rng = np.random.default_rng(701)
    ops = _opening(circ, batch, rng, [(3 << tile) | (5 + b) for b in range(batch)], [0, 1 << tile])
    ops.append(("set_basis", {"buf": BUF_X2, "idx": [7] * batch}))

    def other():
        if replay == "surrogate_eval":
            return ("surrogate_eval", {"th": np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(batch)]), "update": 1,
                                       "real_only": False, "weight": np.full(batch, 0.3), "max_no": np.zeros(batch, np.int64),
                                       "br": None, "front": True})
        return ("eval", {"th": np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(batch)]), "vdag": True,
                         "gather": True, "grad": True, "x": BUF_X2, "br": None, "front": True})

    ops += _launch() + [other()] + _launch() + [other()] + _launch() + [("download", {"buf": BUF_Z, "lane": None})]
    _run(monkeypatch, "cx12_t10", dict(FORCED, AQC_PROJECTED=projected, AQC_PROJECTED_VDAG="0"), ops)


def test_apply_into_zw_completes_a_partial_z_first(monkeypatch):
    """aqc_ws_sweep.cpp run_apply: V x into ZW overwrites V^H's checkpoint; a partial Z left by objective_launch is completed
    from it before the first stage runs, not after."""
    circ, _, tile, batch, _ = _shape("cz13_t8")
    rng = np.random.default_rng(702)
    ops = _opening(circ, batch, rng, [0] * batch, [0, 1 << (tile + 1)])
    ops += _launch() + [("apply", {"inverse": False, "src": BUF_X, "dst": BUF_ZW}), ("download", {"buf": BUF_Z, "lane": None}),
                        ("download", {"buf": BUF_ZW, "lane": None})]
    _run(monkeypatch, "cz13_t8", dict(FORCED, AQC_PROJECTED_VDAG="0"), ops)


@pytest.mark.parametrize("writer", ["upload_lane", "copy_lane"])
def test_lane_writer_of_a_stale_partial_z_refuses(monkeypatch, writer):
    """aqc_api.cpp aqc_ws_upload_lane / aqc_ws_copy_lane (and aqc_ws_extra.cpp mps_to_vec): with the thetas changed since the
    evaluation that left Z partial, a write of one lane cannot complete the others; it refuses with the readers' message and
    leaves Z as it was.  With one lane the write covers the buffer and is taken."""
    from aqc_research_amd.engine import Workspace

    circ, ctx, tile, batch, _ = _shape("cz13_t8")
    rng = np.random.default_rng(703)
    _configure(monkeypatch, dict(FORCED, AQC_PROJECTED_VDAG="0"))
    n = circ.num_qubits
    for B in (batch, 1):
        ws = Workspace(ctx, batch=B, tile_bits_apply=tile, tile_bits_sweep=tile)
        src = Workspace(ctx, batch=B, tile_bits_apply=tile, tile_bits_sweep=tile)
        tg = np.stack([orc.rand_state(n, rng) for _ in range(B)])
        th = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(B)])
        v = orc.rand_state(n, rng)
        src.upload(BUF_Y, np.stack([v] * B))
        ws.upload(BUF_Y, tg)
        ws.set_basis(BUF_X, 0)
        ws.gather_setup([0])
        ws.set_thetas(th)
        ws.objective_launch(BUF_X)
        ws.set_thetas(th[::-1].copy())

        def write():
            if writer == "upload_lane":
                ws.upload(BUF_Z, v, lane=0)
            else:
                ws.copy_lane_from(src, BUF_Y, 0, BUF_Z, 0)
        if B > 1:
            with pytest.raises(RuntimeError, match="BUF_Z holds"):
                write()
            with pytest.raises(RuntimeError, match="BUF_Z holds"):
                ws.download(BUF_Z)
            ws.apply(True, BUF_Y, BUF_Z)   # a whole-buffer writer takes Z over; then lane writes are plain writes
            write()
            z = ws.download(BUF_Z)
            assert wm.maxdiff(z[0], v) == 0.0
            for b in range(1, B):
                assert wm.maxdiff(z[b], orc.v_dagger_mul_vec(circ, th[B - 1 - b], tg[b])) < wm.TOL
        else:
            write()
            assert wm.maxdiff(ws.download(BUF_Z)[0], v) == 0.0
        ws.close()
        src.close()


def test_refused_identity_leaves_a_partial_z_known_as_partial(monkeypatch):
    """aqc_api.cpp aqc_ws_set_identity: a state-vector workspace is no square one, so the call is refused -- after it had announced
    its write, which marked a Z that objective_launch left partial as complete.  The readers of Z must still complete it."""
    from aqc_research_amd.engine import Workspace

    circ, ctx, tile, batch, oracle = _shape("cz13_t8")
    rng = np.random.default_rng(708)
    _configure(monkeypatch, dict(FORCED, AQC_PROJECTED_VDAG="0"))
    tg = np.stack([orc.rand_state(circ.num_qubits, rng) for _ in range(batch)])
    th = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(batch)])
    ws = Workspace(ctx, batch=batch, tile_bits_apply=tile, tile_bits_sweep=tile)
    try:
        ws.upload(BUF_Y, tg)
        ws.set_basis(BUF_X, 0)
        ws.gather_setup([0])
        ws.set_thetas(th)
        ws.objective_launch(BUF_X)
        with pytest.raises(RuntimeError, match="square"):
            ws.set_identity(BUF_Z)
        z = ws.download(BUF_Z)
    finally:
        ws.close()
    for b in range(batch):
        assert wm.maxdiff(z[b], oracle.vdag(th[b], tg[b])) < wm.TOL, b


@pytest.mark.parametrize("call", ["objective_launch", "eval", "surrogate_eval"])
def test_refused_block_range_enqueues_nothing(monkeypatch, call):
    """aqc_ws_sweep.cpp aqc_ws_objective_launch / aqc_ws_eval, aqc_ws_optim.cpp aqc_ws_surrogate_eval: a block_range the ABI
    rejects is rejected before V^H and the gather are enqueued -- Z and the gathered amplitudes stay as they were."""
    circ, _, tile, batch, _ = _shape("cx12_t10")
    rng = np.random.default_rng(704)
    nb = circ.num_blocks
    ops = _opening(circ, batch, rng, [1] * batch, [1, 2])
    ops += _launch()
    ops.append(("upload", {"buf": BUF_Z, "data": np.stack([orc.rand_state(circ.num_qubits, rng) for _ in range(batch)])}))
    th = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(batch)])
    ops.append({"objective_launch": ("objective_launch", {"x": BUF_X, "br": (nb, nb + 1), "front": True, "bad": True}),
                "eval": ("eval", {"th": th, "vdag": True, "gather": True, "grad": True, "x": BUF_X, "br": (3, 2), "front": True,
                                  "bad": True}),
                "surrogate_eval": ("surrogate_eval", {"th": th, "update": 1, "real_only": False, "weight": np.full(batch, 0.5),
                                                      "max_no": np.zeros(batch, np.int64), "br": (0, nb + 1), "front": True,
                                                      "bad": True})}[call])
    ops += [("download", {"buf": BUF_Z, "lane": None}), ("results", {"kind": "gather_fetch"}),
            ("grad", {"x": BUF_X, "br": None, "front": True}), ("results", {"kind": "get_grads"})]
    _run(monkeypatch, "cx12_t10", FORCED, ops)


def test_refused_gather_setup_keeps_the_registered_set(monkeypatch):
    """engine.py Workspace.gather_setup: the wrapper sized every later fetch by the count of a set-up the ABI had refused
    (found by the random sequences: a fetch of 6 amplitudes per lane into room for 2)."""
    circ, _, tile, batch, _ = _shape("cx12_t10")
    rng = np.random.default_rng(705)
    gather = [0, 1, 2, 3, 1 << tile, 2 << tile]
    ops = _opening(circ, batch, rng, [1] * batch, gather) + _launch()
    ops += [("gather_setup", {"idx": [0, 1 << circ.num_qubits]}), ("results", {"kind": "async"}),
            ("results", {"kind": "gather_fetch"}), ("gather_launch", {"buf": BUF_Z})]
    _run(monkeypatch, "cx12_t10", FORCED, ops)


def test_coordinate_descent_wide_walk_leaves_no_stale_checkpoint(monkeypatch):
    """aqc_ws_extra.cpp aqc_ws_cd_sweep: beyond 6 qubits the sweep is the wide walk, launches that rewrite X and Z in place
    after its V^H (run_apply) has left the checkpoint of the old Z in ZW.  A gradient from a basis state afterwards must read Z
    as the walk left it: the sparse route (z of the second stage from the checkpoint) agrees with the dense one."""
    from aqc_research_amd import _lib
    from aqc_research_amd._lib import check, dptr
    from aqc_research_amd.engine import HipContext, Workspace

    n = 7
    circ = _pc(n, "cx", 6)
    ctx = HipContext(circ)
    dim = 1 << n
    rng = np.random.default_rng(706)
    target, _ = np.linalg.qr(rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim)))
    th0 = orc.rand_thetas(circ.num_thetas, rng)
    out = {}
    for cfg in ("forced", "dense_sweep"):
        _configure(monkeypatch, CONFIGS[cfg])
        ws = Workspace(ctx, batch=1, ncols=dim, tile_bits_apply=8, tile_bits_sweep=8)   # (two stages: V^H keeps a checkpoint)
        assert not _lib.lib().aqc_ws_cd_fits_one_launch(ws.handle)
        ws.upload(BUF_Y, target[None])
        th, fobj = th0.copy(), np.zeros(1)
        check(_lib.lib().aqc_ws_cd_sweep(ws.handle, dptr(th), dptr(fobj)))
        ws.set_basis(BUF_X, [5])
        ws.grad()
        out[cfg] = (th, fobj, ws.get_grads()[0])
        ws.close()
    for a, b in zip(out["forced"], out["dense_sweep"]):
        assert wm.maxdiff(a, b) < 1e-12


def test_device_lbfgs_in_every_configuration(monkeypatch):
    """aqc_ws_optim.cpp aqc_ws_lbfgs (maxiter=2): its evaluate step decides its route like the one-call evaluations do, and picks
    the lhs state on the device between V^H and the sweep.  Under every configuration the point it reports has the reported
    fidelity and surrogate value (oracle, 1e-10), an objective_launch from another lhs state afterwards reads nothing stale (Z,
    amplitudes, gradient: oracle, 1e-10), and all of it agrees across the configurations (1e-12).  Lane 1's target sits on a flip
    state in another first-stage tile: that lane leads with it, so the support of the combined lhs state moves."""
    import ctypes

    from aqc_research_amd import _lib

    circ, ctx, tile, batch, oracle = _shape("cx12_t10")
    n, T = circ.num_qubits, circ.num_thetas
    rng = np.random.default_rng(707)
    idx = np.array([5, 5 ^ (1 << tile), 5 ^ 2, 5 ^ (1 << (n - 1))], np.int64)
    basis = np.eye(1 << n, dtype=complex)
    x0 = 0.05 * np.stack([orc.rand_thetas(T, rng) for _ in range(batch)])
    near = x0 + 0.01 * np.stack([orc.rand_thetas(T, rng) for _ in range(batch)])   # targets a short way from the start
    tg = np.stack([orc.v_mul_vec(circ, near[0], basis[idx[0]]), orc.v_mul_vec(circ, near[1], basis[idx[1]]), orc.rand_state(n, rng)])
    th = np.stack([orc.rand_thetas(T, rng) for _ in range(batch)])
    x_late = [(3 << tile) | (7 + b) for b in range(batch)]
    i64 = ctypes.POINTER(ctypes.c_int64)
    results = {}
    for cfg, env in CONFIGS.items():
        _configure(monkeypatch, env)
        ws = _maker(ctx, batch, tile)()
        ws.upload(BUF_Y, tg)
        ws.set_basis(BUF_X, int(idx[0]))
        ws.gather_setup(idx)
        x, f, fid, w = np.empty_like(x0), np.empty(batch), np.empty(batch), np.empty(batch)
        nit, lead, nfev = np.zeros(batch, np.int64), np.zeros(batch, np.int64), ctypes.c_int64()
        _lib.check(ws._L.aqc_ws_lbfgs(ws.handle, _lib.dptr(x0.copy()), 2, 5, 1e-7, 1e-12, 0.0, 12, -1, -1, 1, _lib.dptr(x), _lib.dptr(f),
                                      _lib.dptr(fid), nit.ctypes.data_as(i64), ctypes.byref(nfev), _lib.dptr(w), lead.ctypes.data_as(i64)))
        ws.set_basis(BUF_X, x_late)
        ws.set_thetas(th)
        ws.objective_launch(BUF_X)
        hs, g, z = ws.gather_fetch(), ws.get_grads(), ws.download(BUF_Z)
        ws.close()
        assert lead[1] == 1 and nfev.value >= 3, (lead, nfev.value)   # the case this test is about really occurs
        reads = [("x", x), ("f", f), ("fidelity", fid), ("weight", w), ("leading", lead.astype(float)), ("nit", nit.astype(float)),
                 ("nfev", np.array([float(nfev.value)])), ("launch.hs", hs), ("launch.grads", g), ("launch.z", z)]
        for b in range(batch):
            h2 = np.abs(oracle.vdag(x[b], tg[b])[idx]) ** 2
            f_ref = 1.0 - (1.0 - w[b]) * h2[0] - w[b] * h2[lead[b]]
            vh = oracle.vdag(th[b], tg[b])
            print(f"{cfg} lane {b}: f = {f[b]:.6f}, leading state {lead[b]}, nit {nit[b]}; |fidelity - oracle| = {abs(fid[b] - h2[0]):.3g}, "
                  f"|f - oracle| = {abs(f[b] - f_ref):.3g}, |Z - oracle| = {wm.maxdiff(z[b], vh):.3g}")
            assert abs(fid[b] - h2[0]) < wm.TOL and abs(f[b] - f_ref) < wm.TOL
            assert wm.maxdiff(z[b], vh) < wm.TOL and wm.maxdiff(hs[b], vh[idx]) < wm.TOL
            assert wm.maxdiff(g[b], oracle.grad(th[b], basis[x_late[b]], vh)) < wm.TOL
        results[cfg] = [(0, label, np.array(got)) for label, got in reads]
    _cross_check(results)


# ---- random sequences ------------------------------------------------------------------------------------------------------

CASES = [(s, seed) for s in ("cx12_t10", "cz13_t8", "trotter13_t10", "cp14_t9") for seed in (1, 2, 3)] + [("cx16_t9", 4), ("cx16_t9", 5)]


def _sequence(shape, seed):
    circ, _, tile, batch, _ = _shape(shape)
    return wm.Gen(seed, circ.num_qubits, batch, circ.num_thetas, circ.num_blocks, tile).sequence(25 + seed % 3 * 6)


def _cross_check(results):
    """The same sequence must read the same numbers under every configuration (where both completed the read)."""
    keyed = {}
    for cfg, reads in results.items():
        seen = {}
        for step, label, got in reads:
            k = (step, label, seen.setdefault((step, label), 0))
            seen[(step, label)] += 1
            keyed.setdefault(k, []).append((cfg, got))
    worst = (0.0, None)
    for k, vals in keyed.items():
        for cfg, got in vals[1:]:
            d = wm.maxdiff(got, vals[0][1])
            if d > worst[0]:
                worst = (d, f"{k} {vals[0][0]} vs {cfg}")
    assert worst[0] < 1e-12, f"configurations disagree by {worst[0]:.3g} at {worst[1]}"


@pytest.mark.parametrize("shape,seed", CASES)
def test_random_sequence_matches_the_model_in_every_configuration(monkeypatch, shape, seed):
    ops = _sequence(shape, seed)
    results = {cfg: _run(monkeypatch, shape, env, ops) for cfg, env in CONFIGS.items()}
    _cross_check(results)


@pytest.mark.parametrize("family", ["1", "2"])
def test_random_sequence_on_the_valu_kernel_families(monkeypatch, family):
    ops = _sequence("cx12_t10", 1)
    results = {"mfma": _run(monkeypatch, "cx12_t10", {}, ops),
               "family": _run(monkeypatch, "cx12_t10", {"AQC_KERNEL_FAMILY": family}, ops)}
    _cross_check(results)
