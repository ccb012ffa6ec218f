"""Shadow model of a matrix workspace (ncols = k > 1), its sequence generator and the oracle's rendering of the workspace; the
runner, the digest memo and `describe` are those of tests/ws_model.py (run_sequence(..., kit=MatKit)).

Lanes hold [2^n][k] matrices.  The W, ZW and Z rules of the header's buffer paragraph stand as in the state-vector model.  What
this one adds is the side-effect sentence of every long-running matrix call of include/aqc_hip.h:

  call              unspecified afterwards   kept     thetas in use at exit
  lbfgs_mat         Z W ZW                   X Y X2   x_out
  cd_sweep(s)       X Z W ZW                 Y X2     thetas_io as returned
  cd_minimize       X Z W ZW                 Y X2     best_thetas, on every route
  sketch_generate   W ZW (X, Y: the result)  Z X2     unchanged (read by `eigen`)
  sketch_adam       X Y Z W ZW               X2       x_out; reset = 0 resumes from the run's own last point

The thetas in use are tracked as a value.  After a long-running call they are the thetas the call itself returned -- never the
reference's -- so an optimiser's tolerance does not leak into a 1e-10 read; the call's outputs are held to its reference
(tests/lbfgs_ref.py, the coordinate-descent restatements of oracle/, tests/sketch_ref.py) at the bounds the isolated tests of
that call use.  An unspecified buffer is never read until a writer takes it over.  A refused call changes nothing.
"""
import numpy as np

from oracle import aqc_oracle as aorc
from oracle import aqc_ref as cref
from tests import sketch_ref as sk
from tests import ws_model as wm
from tests.lbfgs_ref import lbfgs_ref
from tests.ws_model import BUF_W, BUF_X, BUF_X2, BUF_Y, BUF_Z, BUF_ZW, NAMES, TOL

# bounds of the isolated tests: test_hip_full_aqc_device (trajectory: fun 1e-6, x 1e-5), test_hip_cd_driver / test_hip_round4 (whole
# sweeps: 1e-8 on the first value, 1e-7 on the second and on the thetas), test_hip_sketched (ADAM walk 1e-9, orthonormality 1e-12)
LBFGS_F, LBFGS_X = 1e-6, 1e-5
CD_F, CD_TH = (1e-8, 1e-7), 1e-7
ADAM = 1e-9
ORTH = 1e-12
SKETCH_CODE = {"rand": sk.SKETCH_RAND, "alt": sk.SKETCH_ALT, "eigen": sk.SKETCH_EIGEN}
LONG = ("lbfgs_mat", "cd_sweeps", "cd_sweep", "cd_minimize", "sketch_generate", "sketch_adam")
ADAM_KW = dict(beta1=0.9, beta2=0.99, eps=1e-8)


class MatOracle(wm.Oracle):
    """V, V^H and the gradient on [2^n][k] matrices (oracle/aqc_ref.py), memoised like the state-vector ones."""

    def vdag(self, th, y):
        return self._get("vhm", lambda: cref.v_dagger_mul_mat(self.circ, th, y), th, y)

    def v(self, th, y):
        return self._get("vm", lambda: cref.v_mul_mat(self.circ, th, y), th, y)

    def grad(self, th, x, z, block_range=None, front=True):
        assert block_range is None and front, "the matrix gradient walks every block"
        return self._get("gm", lambda: cref.grad_of_matrix_dot_product(self.circ, th, x, z), th, x, z)

    def objective(self, th, x, y):
        """f = 1 - Re tr(X^H V^H Y) / k and its gradient (sk_core.py:167-194): (f, g[T])."""
        z = self.vdag(th, y)
        return 1.0 - float(np.real(np.vdot(x, z))) / x.shape[1], -np.real(self.grad(th, x, z)) / x.shape[1]


# ---- references of the long-running calls, on the oracle -----------------------------------------------------------------

def lbfgs_reference(orc, x, y, x0, maxiter, memory, max_backtracks):
    def fun(th):
        res = [orc.objective(th[b], x[b], y[b]) for b in range(len(th))]
        return np.array([r[0] for r in res]), np.stack([r[1] for r in res])
    ref = lbfgs_ref(fun, x0, maxiter=maxiter, memory=memory, gtol=0.0, ftol=0.0, max_backtracks=max_backtracks)
    ref["memory"] = memory
    ref["points"] = [np.array(x0, float)] + [it["x"] for it in ref["trace"]]
    ref["grads"] = [fun(p)[1] for p in ref["points"]]      # (memoised: the walk has been at every one of them)
    return ref


def lbfgs_margins(ref):
    """Relative margins of the Armijo tests the reference took: |ft - bound| / max(1, |f|)."""
    out = []
    for it in ref["trace"]:
        for m in it["margins"]:
            out += list(np.abs(m[~np.isnan(m)]) / np.maximum(1.0, np.abs(it["f_in"][~np.isnan(m)])))
    return out


def lbfgs_branch_margins(ref):
    """Relative margins of the reference's other branches, on the lanes they decide for, from its trace and the gradients at its
    points: the descent test slope >= 0 as |<g, d>| / (|g| |d|) -- where it fired the direction is -g and the two-loop slope is not
    on record: margin 0 --, the curvature test sy > 1e-12 yy as |sy - 1e-12 yy| / (|s| |y|), the relative-decrease test
    |f - f_acc| <= ftol max(1, |f|) (ftol = 0: a tie is an unchanged value) as |f - f_acc| / max(1, |f|)."""
    out = {"descent": [], "curvature": [], "decrease": []}
    norm = lambda a: np.sqrt(np.einsum("bt,bt->b", a, a))   # noqa: E731
    for k, it in enumerate(ref["trace"]):
        g, g_new = ref["grads"][k], ref["grads"][k + 1]
        s, y = ref["points"][k + 1] - ref["points"][k], g_new - g
        on = it["active_in"]
        mv = on & (it["step"] > 0) & (s != 0).any(axis=1)
        # (d = -g is also what the two-loop gives a lane none of whose pairs on record was taken: slope = -<g, g>, margin 1)
        pairs = [t["good"] for t in ref["trace"][max(0, k - ref["memory"]):k]]
        empty = ~np.any(pairs, axis=0) if pairs else np.ones(len(g), bool)
        fired = np.array([not empty[b] and np.array_equal(it["d"][b], -g[b]) for b in range(len(g))])
        out["descent"] += list(np.where(fired, 0.0, np.abs(it["slope"]) / (norm(g) * norm(it["d"])))[on])
        sy, yy = np.einsum("bt,bt->b", s, y), np.einsum("bt,bt->b", y, y)
        out["curvature"] += list((np.abs(sy - 1e-12 * yy) / np.maximum(norm(s) * norm(y), 1e-300))[mv])
        out["decrease"] += list((np.abs(it["f"] - it["f_in"]) / np.maximum(1.0, np.abs(it["f_in"])))[mv])
    return out


def cd_reference(circ, th0, y, nsweeps, max_steps):
    """(thetas after every sweep [nsweeps][B][T], fobj [B][nsweeps]): whole sweeps by the compiled restatement, cut ones
    (max_steps >= 0) by the oracle's sweep."""
    th = np.array(th0, float)
    B = th.shape[0]
    ths, fobj = [], np.zeros((B, nsweeps))
    for s in range(nsweeps):
        if max_steps < 0:
            th, f = cref.coord_descent_sweeps(circ, th, y, 1)
            fobj[:, s] = f[:, 0]
        else:
            nxt = []
            for b in range(B):
                t, f = aorc.coord_descent_single_sweep(circ, th[b].copy(), y[b], max_steps=max_steps)
                nxt.append(t)
                fobj[b, s] = f
            th = np.stack(nxt)
        ths.append(th.copy())
    return np.stack(ths), fobj


def cd_best(ths, fobj):
    """The rule of csrc/aqc_cd_rule.h with its thresholds off: a sweep's value below the best so far is recorded with the
    sweep's thetas.  Returns (best thetas [B][T], best f [B], index of the best sweep [B])."""
    B = fobj.shape[0]
    best = np.array([int(np.argmin(fobj[b])) for b in range(B)])   # (the first of equal values: `below`, not `at most`)
    return np.stack([ths[best[b], b] for b in range(B)]), fobj[np.arange(B), best], best


def cd_margins(fobj):
    """Relative margins of the best-so-far decisions: consecutive running minima against the next value."""
    out = []
    for row in fobj:
        best = np.inf
        for f in row:
            if np.isfinite(best):
                out.append(abs(f - best) / max(1.0, abs(best)))
            best = min(best, f)
    return out


def sketch_pair(orc, kind, u, k, th, om, idx):
    """(X, Y = U X) of one lane by tests/sketch_ref.py, V^H from the oracle."""
    return sk.generate(SKETCH_CODE[kind], u, k, om=om, idx=idx, vh_mul=None if th is None else (lambda m: orc.vdag(th, m)))


def adam_lane(orc, kind, u, k, lane, state, niter, lr, seed, iter0, alt_idx):
    """One lane of aqc_ws_sketch_adam from `state` (m, v, t, x, best_f, best_x, flag), as sk_adam_kernel walks it: evaluation e
    under sketch iter0 + e + 1, a step after each but the last.  Returns (new state, profile [niter + 1], nit)."""
    d = u.shape[0]
    st = {key: (np.array(val, float) if isinstance(val, np.ndarray) else val) for key, val in state.items()}
    prof, nit = np.zeros(niter + 1), 0
    code = SKETCH_CODE[kind]
    for e in range(niter + 1):
        om = None if kind == "alt" else sk.omega(code, seed, iter0 + e + 1, lane, d, k)
        xm, ym = sketch_pair(orc, kind, u, k, st["x"] if kind == "eigen" else None, om, None if alt_idx is None else alt_idx[e][lane])
        f, g = orc.objective(st["x"], xm, ym)
        prof[e] = f
        if st["flag"] < 2 and f < st["best_f"]:
            st["best_f"], st["best_x"] = f, st["x"].copy()
        if st["flag"] == 1:
            st["flag"] = 2
        if st["flag"] != 0 or e == niter:
            continue
        t = st["t"] + 1
        m = ADAM_KW["beta1"] * st["m"] + (1 - ADAM_KW["beta1"]) * g
        v = ADAM_KW["beta2"] * st["v"] + (1 - ADAM_KW["beta2"]) * g * g
        step = lr * np.sqrt(1 - ADAM_KW["beta2"] ** t) / (1 - ADAM_KW["beta1"] ** t) * m / (np.sqrt(v) + ADAM_KW["eps"])
        st.update(m=m, v=v, t=t, x=st["x"] - step)
        nit += 1
    return st, prof, nit


def adam_margins(profiles):
    return cd_margins(profiles)


# ---- the model -----------------------------------------------------------------------------------------------------------

class MatModel:
    """Logical content of one matrix workspace (see the module docstring).  bufs[b] is None while b is unspecified."""

    def __init__(self, orc, batch, circ, ncols):
        self.orc, self.circ, self.B, self.dim, self.k = orc, circ, batch, 1 << circ.num_qubits, ncols
        self.T = circ.num_thetas
        self.bufs = {b: None for b in NAMES}
        self.thetas = None            # the thetas in use, as a value
        self.bank = None
        self.grads = None
        self.pending = None           # what results_async took a copy of
        self.target = None            # sketch_target: [B][d][d]
        self.adam = None              # per lane: m, v, t, x, best_f, best_x, flag
        self.rewritten = set()

    def write(self, buf, value, lanes=None):
        self.rewritten.add(buf)
        if lanes is None:
            self.bufs[buf] = None if value is None else np.array(value, complex)
            return
        cur = self.bufs[buf]
        if cur is None and len(lanes) < self.B:
            return                                  # a lane of an unspecified buffer leaves it unspecified
        cur = np.zeros((self.B, self.dim, self.k), complex) if cur is None else cur.copy()
        for lane, v in zip(lanes, value):
            cur[lane] = v
        self.bufs[buf] = cur

    def scribbled(self, *bufs):
        for b in bufs:
            self.write(b, None)

    def per_lane(self, fn, *arrays):
        return np.stack([fn(self.thetas[b], *[a[b] for a in arrays]) for b in range(self.B)])

    def vdag_into_z(self):
        self.write(BUF_Z, self.per_lane(self.orc.vdag, self.bufs[BUF_Y]))
        self.scribbled(BUF_ZW)                      # the mirrored V^H keeps its checkpoint there

    def sweep(self, x_buf):
        self.grads = self.per_lane(self.orc.grad, self.bufs[x_buf], self.bufs[BUF_Z])
        self.scribbled(BUF_W, BUF_ZW)
        return self.grads

    def returned_thetas(self, th):
        """A long-running call has returned `th`: they are the thetas in use."""
        self.thetas = np.array(th, float)


def _refused(fn, what):
    try:
        fn()
    except (RuntimeError, ValueError, NotImplementedError):
        return []
    raise AssertionError(f"{what}: the call was expected to be refused")


def apply_op(ws, m: MatModel, op, ws2=None, m2=None):
    """Run `op` on `ws` and on the model; returns the reads (label, got, expected[, own bound])."""
    name, a = op
    reads = []
    B, k, dim = m.B, m.k, m.dim
    if a.get("bad"):
        return _refused(lambda: _call(ws, op, ws2), f"{name} ({a['bad']})")
    if name == "set_thetas":
        ws.set_thetas(a["th"])
        m.thetas = np.array(a["th"], float)
    elif name == "theta_bank":
        ws.theta_bank(a["bank"])
        m.bank = np.array(a["bank"], float)
    elif name == "use_theta_set":
        ws.use_theta_set(a["i"])
        m.thetas = m.bank[a["i"]].copy()
    elif name == "upload":
        ws.upload(a["buf"], a["data"])
        m.write(a["buf"], a["data"])
    elif name == "broadcast":
        ws.broadcast(a["buf"], a["data"])
        m.write(a["buf"], np.broadcast_to(a["data"], (B, dim, k)))
    elif name == "upload_lane":
        ws.upload(a["buf"], a["data"], lane=a["lane"])
        m.write(a["buf"], [a["data"]], lanes=[a["lane"]])
    elif name == "set_identity":
        ws.set_identity(a["buf"])
        m.write(a["buf"], np.broadcast_to(np.eye(dim, dtype=complex), (B, dim, dim)))
    elif name == "copy_in":     # ws.dst[dst_lane] <- ws2.Y[src_lane]
        ws.copy_lane_from(ws2, BUF_Y, a["src_lane"], a["dst"], a["dst_lane"])
        m.write(a["dst"], [m2.bufs[BUF_Y][a["src_lane"]]], lanes=[a["dst_lane"]])
    elif name == "copy_out":    # ws2.X[dst_lane] <- ws.src[src_lane], read back from ws2
        ws2.copy_lane_from(ws, a["src"], a["src_lane"], BUF_X, a["dst_lane"])
        m2.write(BUF_X, [m.bufs[a["src"]][a["src_lane"]]], lanes=[a["dst_lane"]])
        reads.append((f"copy_out({NAMES[a['src']]})", ws2.download(BUF_X, a["dst_lane"]), m2.bufs[BUF_X][a["dst_lane"]]))
    elif name == "download":
        buf, lane = a["buf"], a["lane"]
        reads.append((f"download({NAMES[buf]}, {lane})", ws.download(buf, lane), m.bufs[buf] if lane is None else m.bufs[buf][lane]))
    elif name == "gather":
        idx = np.array(a["idx"], np.int64)
        reads.append((f"gather({NAMES[a['buf']]})", ws.gather(a["buf"], idx), m.bufs[a["buf"]].reshape(B, -1)[:, idx]))
    elif name in ("vdot", "vdot_launch"):
        exp = np.einsum("bik,bik->b", np.conj(m.bufs[a["a"]]), m.bufs[a["b"]])
        if name == "vdot":
            got = ws.vdot(a["a"], a["b"])
        else:
            ws.vdot_launch(a["a"], a["b"])
            got = ws.vdot_fetch()
        reads.append((f"{name}({NAMES[a['a']]}, {NAMES[a['b']]})", got, exp))
    elif name == "apply":
        ws.apply(a["inverse"], a["src"], a["dst"])
        m.write(a["dst"], m.per_lane(m.orc.vdag if a["inverse"] else m.orc.v, m.bufs[a["src"]]))
        if a["dst"] == BUF_Z and a["inverse"]:
            m.scribbled(BUF_ZW)
    elif name == "grad":
        if a["x"] == BUF_X and a.get("plain"):
            ws.grad()
        else:
            ws.grad_from(a["x"])
        m.sweep(a["x"])
    elif name == "get_grads":
        reads.append(("get_grads", ws.get_grads(), m.grads))
    elif name == "eval":
        _, g = ws.eval(a["th"], a["vdag"], False, a["grad"], a["x"])
        if a["th"] is not None:
            m.thetas = np.array(a["th"], float)
        if a["vdag"]:
            m.vdag_into_z()
        if a["grad"]:
            reads.append(("eval.grads", g, m.sweep(a["x"])))
    elif name == "objective_launch":
        ws.objective_launch(a["x"])
        m.vdag_into_z()
        m.sweep(a["x"])
    elif name == "results_async":
        ws.results_async()
        m.pending = m.grads.copy()
    elif name == "results_fetch":
        reads.append(("results.grads", ws.results_fetch(small=False)[1], m.pending))
    elif name == "lbfgs_mat":
        kw = dict(maxiter=a["maxiter"], memory=a["memory"], max_backtracks=a["max_backtracks"])
        res = ws.lbfgs_mat(a["x0"], gtol=0.0, ftol=0.0, **kw)
        ref = lbfgs_reference(m.orc, m.bufs[BUF_X], m.bufs[BUF_Y], a["x0"], **kw)
        at_x = np.array([m.orc.objective(res["x"][b], m.bufs[BUF_X][b], m.bufs[BUF_Y][b])[0] for b in range(B)])
        assert not np.any(res["status"]), f"lbfgs_mat: status {res['status']}"
        assert [int(v) for v in res["nit"]] == [int(v) for v in ref["nit"]] and res["nfev"] == ref["nfev"], \
            f"lbfgs_mat: nit {res['nit']} nfev {res['nfev']}, reference {ref['nit']} {ref['nfev']}"
        reads += [("lbfgs_mat.x", res["x"], ref["x"], LBFGS_X), ("lbfgs_mat.fun", res["fun"], ref["fun"], LBFGS_F),
                  ("lbfgs_mat.fun at x", res["fun"], at_x, TOL)]
        m.scribbled(BUF_Z, BUF_W, BUF_ZW)
        m.returned_thetas(res["x"])
    elif name in ("cd_sweeps", "cd_sweep"):
        ns, steps = a.get("nsweeps", 1), a.get("max_steps", -1)
        if name == "cd_sweep":
            th, f = ws.cd_sweep(a["th"][0])
            th, fobj = th[None], np.array([[f]])
        else:
            th, fobj = ws.cd_sweeps(a["th"], ns, steps)
        ths, f_ref = cd_reference(m.circ, a["th"], m.bufs[BUF_Y], ns, steps)
        cut = steps >= 0
        reads.append((f"{name}.thetas", th, ths[-1], TOL if cut and ns == 1 else CD_TH))
        for s in range(ns):
            reads.append((f"{name}.fobj[{s}]", fobj[:, s], f_ref[:, s], TOL if cut and ns == 1 else CD_F[min(s, 1)]))
        m.scribbled(BUF_X, BUF_Z, BUF_W, BUF_ZW)
        m.returned_thetas(th)
    elif name == "cd_minimize":
        res = ws.cd_minimize(a["th"], a["maxiter"], chunk=a["chunk"], dtheta_thr=0.0, fobj_thr=0.0, route=a["route"])
        ths, f_ref = cd_reference(m.circ, a["th"], m.bufs[BUF_Y], a["maxiter"], -1)
        best_th, best_f, best = cd_best(ths, f_ref)
        got_best = [int(np.argmin(res["profile"][b])) for b in range(B)]
        assert got_best == [int(v) for v in best], f"cd_minimize: best sweep {got_best}, reference {best}"
        assert all(int(v) == a["maxiter"] for v in res["nit"]) and all(int(v) == 1 for v in res["status"]), (res["nit"], res["status"])
        assert np.array_equal(res["cost"], res["profile"][np.arange(B), got_best]), "cd_minimize: cost is not the profile's smallest entry"
        reads.append(("cd_minimize.thetas", res["thetas"], best_th, CD_TH))
        for s in range(a["maxiter"]):
            reads.append((f"cd_minimize.profile[{s}]", res["profile"][:, s], f_ref[:, s], CD_F[min(s, 1)]))
        m.scribbled(BUF_X, BUF_Z, BUF_W, BUF_ZW)
        m.returned_thetas(res["thetas"])
    elif name == "sketch_target":
        ws.sketch_target(a["U"])
        m.target = np.array(a["U"], complex)
    elif name == "sketch_generate":
        st = ws.sketch_generate(a["kind"], seed=a["seed"], iteration=a["iteration"], alt_idx=a["alt_idx"], omega=a["omega"])
        assert not np.any(st), f"sketch_generate: QR status {st}"
        m.rewritten |= {BUF_X, BUF_Y}
        x, y = ws.download(BUF_X), ws.download(BUF_Y)
        for b in range(B):
            xr, _ = sketch_pair(m.orc, a["kind"], m.target[b], k, m.thetas[b] if a["kind"] == "eigen" else None,
                                None if a["omega"] is None else a["omega"][b], None if a["alt_idx"] is None else a["alt_idx"][b])
            reads += [(f"sketch_generate.orthonormal[{b}]", np.conj(x[b].T) @ x[b], np.eye(k), ORTH),
                      (f"sketch_generate.range[{b}]", x[b] @ np.conj(x[b].T), xr @ np.conj(xr.T)),
                      (f"sketch_generate.Y[{b}]", y[b], m.target[b] @ x[b])]
        m.bufs[BUF_X] = x                            # the basis the device chose
        m.bufs[BUF_Y] = np.stack([m.target[b] @ x[b] for b in range(B)])
        m.scribbled(BUF_W, BUF_ZW)
    elif name == "sketch_draw":
        ws.sketch_draw(a["kind"], seed=a["seed"], iteration=a["iteration"], buf=a["buf"])
        m.write(a["buf"], np.stack([sk.omega(SKETCH_CODE[a["kind"]], a["seed"], a["iteration"], b, dim, k) for b in range(B)]))
    elif name == "sketch_adam":
        niter, reset = a["niter"], a["reset"]
        if m.adam is None:   # the state as the first call finds it: zeros, at the thetas in use
            m.adam = [dict(m=np.zeros(m.T), v=np.zeros(m.T), t=0, x=m.thetas[b].copy(), best_f=0.0, best_x=np.zeros(m.T), flag=0)
                      for b in range(B)]
        res = ws.sketch_adam(a["kind"], a["x0"], niter, a["lr"], tol=0.0, seed=a["seed"], iter0=a["iter0"], reset=reset,
                             alt_idx=a["alt_idx"], **ADAM_KW)
        assert not np.any(res["status"]), f"sketch_adam: QR status {res['status']}"
        prof, nit, new = np.zeros((B, niter + 1)), [], []
        for b in range(B):
            st = dict(m.adam[b])
            if reset[b] == 1:
                st.update(m=np.zeros(m.T), v=np.zeros(m.T), t=0, x=np.array(a["x0"][b], float), best_f=np.inf, flag=0)
            elif reset[b] == 2:
                st["flag"] = 2
            st, prof[b], n_b = adam_lane(m.orc, a["kind"], m.target[b], k, b, st, niter, a["lr"], a["seed"], a["iter0"], a["alt_idx"])
            new.append(st)
            nit.append(n_b)
        assert [int(v) for v in res["nit"]] == nit, f"sketch_adam: nit {res['nit']}, reference {nit}"
        reads += [("sketch_adam.x", res["x"], np.stack([s["x"] for s in new]), ADAM), ("sketch_adam.profile", res["profile"], prof, ADAM),
                  ("sketch_adam.best_f", res["best_f"], np.array([s["best_f"] for s in new]), ADAM),
                  ("sketch_adam.best_x", res["best_x"], np.stack([s["best_x"] for s in new]), ADAM)]
        for b in range(B):   # the run goes on from the point the device returned (m, v, t: the reference's)
            new[b]["x"] = res["x"][b].copy()
        m.adam = new
        m.scribbled(BUF_X, BUF_Y, BUF_Z, BUF_W, BUF_ZW)
        m.returned_thetas(res["x"])
    else:
        raise ValueError(f"unknown operation {name}")
    return reads


def _call(ws, op, ws2):
    """The bare call of an operation that is expected to be refused."""
    name, a = op
    if name == "upload_lane":
        return ws.upload(a["buf"], a["data"], lane=a["lane"])
    if name == "gather":
        return ws.gather(a["buf"], np.array(a["idx"], np.int64))
    if name == "grad":
        return ws.grad_from(a["x"], a["br"], True)
    if name == "use_theta_set":
        return ws.use_theta_set(a["i"])
    if name == "set_identity":
        return ws.set_identity(a["buf"])
    if name == "lbfgs_mat":
        return ws.lbfgs_mat(a["x0"], maxiter=1, gtol=0.0, ftol=0.0)
    if name == "cd_sweeps":
        return ws.cd_sweeps(a["th"], 1, -1)
    if name == "cd_sweep":
        return ws.cd_sweep(a["th"][0])
    if name == "cd_minimize":
        return ws.cd_minimize(a["th"], 1, dtheta_thr=0.0, fobj_thr=0.0, route=a.get("route", "auto"))
    if name == "sketch_target":
        return ws.sketch_target(a["U"])
    if name == "sketch_draw":
        return ws.sketch_draw("rand", seed=1, iteration=1, buf=a["buf"])
    if name == "sketch_adam":
        return ws.sketch_adam("rand", a["x0"], 1, 0.1, tol=0.0, reset=a["reset"], **ADAM_KW)
    raise ValueError(f"no refusal form of {name}")


# ---- generator -----------------------------------------------------------------------------------------------------------

class MatGen:
    """Seeded sequences for one shape.  `kind`: "pc" (a ParametricCircuit: everything that is legal there), "trotter" (data
    operations and the refusals of every matrix driver).  It tracks which buffers are specified, whether the target and the ADAM
    state exist, and the last thetas the host handed over -- nothing that depends on a device result."""

    def __init__(self, seed, circ, batch, ncols, fits_one_launch, kind="pc", part=(0, 1)):
        self.rng = np.random.default_rng(seed)
        self.part = part
        self.circ, self.B, self.k, self.kind = circ, batch, ncols, kind
        self.n, self.T, self.nb = circ.num_qubits, circ.num_thetas, circ.num_blocks
        self.dim = 1 << self.n
        self.square = ncols == self.dim
        self.cd_ok = self.square and circ.entangler in ("cx", "cz") and kind == "pc"
        self.fits = bool(fits_one_launch)
        self.sketch_ok = kind == "pc" and 1 < ncols <= 64 and ncols < self.dim and not (ncols & (ncols - 1))
        self.known = {b: False for b in NAMES}
        self.bank_sets = 0
        self.target = self.adam = False
        self.host_thetas = None       # the last thetas the host set (what "the same values as before the call" means)
        self.sketch_no = 0
        self.follow = {}

    # -- draws of values
    def mats(self, lanes):
        v = self.rng.standard_normal((lanes, self.dim, self.k)) + 1j * self.rng.standard_normal((lanes, self.dim, self.k))
        return v / np.linalg.norm(v.reshape(lanes, -1), axis=1)[:, None, None]

    def thetas(self):
        return np.pi * (2 * self.rng.random((self.B, self.T)) - 1)

    def unitaries(self):
        g = self.rng.standard_normal((self.B, self.dim, self.dim)) + 1j * self.rng.standard_normal((self.B, self.dim, self.dim))
        return np.stack([np.linalg.qr(a)[0] for a in g])

    def alt_idx(self, sets):
        idx = np.stack([np.stack([self.rng.permutation(self.dim)[:self.k] for _ in range(self.B)]) for _ in range(sets)])
        return idx.astype(np.int32)

    # -- bookkeeping
    def _set(self, th):
        self.host_thetas = th
        return ("set_thetas", {"th": th})

    def _wrote(self, *bufs):
        for b in bufs:
            self.known[b] = True

    def _lost(self, *bufs):
        for b in bufs:
            self.known[b] = False

    def setup(self):
        ops = [("upload", {"buf": BUF_Y, "data": self.mats(self.B)}), ("upload", {"buf": BUF_X, "data": self.mats(self.B)}),
               ("upload", {"buf": BUF_X2, "data": self.mats(self.B)})]
        self._wrote(BUF_Y, BUF_X, BUF_X2)
        if self.kind == "pc":
            ops.append(self._set(self.thetas()))
        return ops

    def known_bufs(self, among=tuple(NAMES)):
        return [b for b in among if self.known[b]]

    def read(self, buf=None, how=None):
        r = self.rng
        buf = int(r.choice(self.known_bufs())) if buf is None else buf
        how = ["download", "gather", "vdot", "vdot_launch"][int(r.integers(4))] if how is None else how
        if how == "download":
            return ("download", {"buf": buf, "lane": None if r.random() < 0.5 else int(r.integers(self.B))})
        if how == "gather":
            return ("gather", {"buf": buf, "idx": [int(i) for i in r.integers(0, self.dim * self.k, 4)]})
        return (how, {"a": buf, "b": int(r.choice(self.known_bufs()))})

    def writer(self, how, bufs=(BUF_Y, BUF_X, BUF_X2, BUF_W, BUF_ZW, BUF_Z)):
        r = self.rng
        buf = int(r.choice(bufs))
        if how == "lane":
            if self.B == 1:
                self._wrote(buf)
            return ("upload_lane", {"buf": buf, "lane": int(r.integers(self.B)), "data": self.mats(1)[0]})
        self._wrote(buf)
        if how == "upload":
            return ("upload", {"buf": buf, "data": self.mats(self.B)})
        if how == "broadcast":
            return ("broadcast", {"buf": buf, "data": self.mats(1)[0]})
        return ("set_identity", {"buf": buf})

    def theta_reader(self):
        """A call that reads the thetas in use, and the read that shows what it computed."""
        inv = bool(self.rng.random() < 0.5)
        self._wrote(BUF_W)
        return [("apply", {"inverse": inv, "src": BUF_X2, "dst": BUF_W}), ("download", {"buf": BUF_W, "lane": None})]

    def after_long(self, ops, before, ordinal=None):
        """What follows a long-running call: a theta-reading call at once, or set_thetas with the values from before it first."""
        if not self.known[BUF_X2]:
            ops.append(("upload", {"buf": BUF_X2, "data": self.mats(self.B)}))
            self._wrote(BUF_X2)
        call = [op for op in ops if op[0] in LONG][-1]
        count = self.follow.get(call[0], self.part[0]) if ordinal is None else ordinal   # both ways for every kind of call
        self.follow[call[0]] = count + 1
        call[1]["follow"] = "same" if count % 2 else "direct"
        if count % 2:
            ops.append(self._set(before.copy()))
        return ops + self.theta_reader()

    def ensure(self, *bufs):
        ops = []
        for b in bufs:
            if not self.known[b]:
                ops.append(("upload", {"buf": b, "data": self.mats(self.B)}))
                self._wrote(b)
        return ops

    # -- the deck: every kind of draw that is legal on this shape, in a fixed shuffled order; seed i of m plays every m-th card
    def deck(self):
        if self.kind == "trotter":
            return ["writer_upload", "writer_lane", "read_download", "read_gather", "read_vdot", "read_vdot_launch", "refused:0",
                    "refused:1", "refused:2", "refused:3"]
        cards = ["theta_set", "theta_bank", "writer_upload", "writer_broadcast", "writer_lane", "copy_in", "copy_out", "apply", "grad:0", "grad:1",
                 "read_download", "read_gather", "read_vdot", "read_vdot_launch", "eval_thetas", "eval_keep", "objective", "objective_long",
                 "refused:0", "refused:1", "refused:2", "refused:3", "lbfgs:0", "lbfgs:1", "pair_long"]
        cards += ["writer_identity"] if self.square else []
        cards += ["cd_minimize:0", "cd_minimize:1"] if self.cd_ok else []
        cards += ["cd_sweeps:0", "cd_sweeps:1"] if self.cd_ok and self.fits else []
        cards += ["cd_sweep:0", "cd_sweep:1"] if self.cd_ok and self.B == 1 else []
        cards += ["sketch_target", "sketch_generate:0", "sketch_generate:1", "sketch_generate:2", "sketch_draw", "sketch_adam:0",
                  "sketch_adam:1"] if self.sketch_ok else []
        return [cards[i] for i in np.random.default_rng(len(cards)).permutation(len(cards))]

    def draw(self, c):
        r, B = self.rng, self.B
        if c == "theta_set":
            return [self._set(self.thetas())]
        if c == "theta_bank":
            self.bank_sets = int(r.integers(2, 4))
            self.bank = np.stack([self.thetas() for _ in range(self.bank_sets)])
            i, j = int(r.integers(self.bank_sets)), int(r.integers(self.bank_sets))
            self.host_thetas = self.bank[j]
            return [("theta_bank", {"bank": self.bank}), ("use_theta_set", {"i": i})] + self.theta_reader() + [("use_theta_set", {"i": j})]
        if c.startswith("writer_"):
            return [self.writer(how=c[7:])]
        if c == "copy_in":
            dst = int(r.choice([BUF_Y, BUF_X, BUF_Z, BUF_ZW]))
            return [("copy_in", {"dst": dst, "dst_lane": int(r.integers(B)), "src_lane": int(r.integers(B))})] + \
                ([self.read(dst)] if self.known[dst] else [])
        if c == "copy_out":
            return [("copy_out", {"src": int(r.choice(self.known_bufs())), "src_lane": int(r.integers(B)), "dst_lane": int(r.integers(B))})]
        if c == "apply":
            src = int(r.choice(self.known_bufs()))
            dst = int(r.choice([b for b in (BUF_X, BUF_X2, BUF_W, BUF_ZW, BUF_Z) if b != src]))
            inv = bool(r.random() < 0.5)
            self._wrote(dst)
            if dst == BUF_Z and inv:
                self._lost(BUF_ZW)
            return [("apply", {"inverse": inv, "src": src, "dst": dst}), self.read(dst)]
        if c.startswith("grad:"):
            ops = []
            if not self.known[BUF_Z]:
                ops += self.ensure(BUF_Y) + [("apply", {"inverse": True, "src": BUF_Y, "dst": BUF_Z})]
                self._wrote(BUF_Z)
            plain = c == "grad:0"                        # aqc_ws_grad (from X), or aqc_ws_grad_from with either lhs buffer
            ops += self.ensure(BUF_X) if plain else []
            x = BUF_X if plain else int(r.choice(self.known_bufs((BUF_X, BUF_X2))))
            self._lost(BUF_W, BUF_ZW)
            return ops + [("grad", {"x": x, "plain": plain}), ("get_grads", {})]
        if c.startswith("read_"):
            return [self.read(how=c[5:])]
        if c in ("eval_thetas", "eval_keep"):
            ops = self.ensure(BUF_Y)
            vdag = bool(r.random() < 0.7) or not self.known[BUF_Z]
            th = self.thetas() if c == "eval_thetas" else None
            if th is not None:
                self.host_thetas = th
            grad = bool(r.random() < 0.8) or not vdag
            x = int(r.choice(self.known_bufs((BUF_X, BUF_X2))))
            if vdag:
                self._wrote(BUF_Z)
                self._lost(BUF_ZW)
            if grad:
                self._lost(BUF_W, BUF_ZW)
            return ops + [("eval", {"th": th, "vdag": vdag, "grad": grad, "x": x})] + ([] if grad else [self.read(BUF_Z)])
        if c in ("objective", "objective_long"):
            ops = self.ensure(BUF_Y)
            x = int(r.choice(self.known_bufs((BUF_X, BUF_X2))))
            self._wrote(BUF_Z)
            self._lost(BUF_W, BUF_ZW)
            ops += [("objective_launch", {"x": x}), ("results_async", {})]
            if c == "objective_long":
                ops += self.long_call(results_pending=True)
            return ops + [("results_fetch", {})]
        if c.startswith("refused:"):
            return self.refused(int(c[8:]))
        if c == "pair_long":
            return self.long_call() + self.long_call()
        which, _, ordinal = c.partition(":")
        return self.long_call(which, int(ordinal) if ordinal else None)

    def long_call(self, which=None, ordinal=None, results_pending=False):
        """One long-running call that is legal on this shape (with what it needs put in place first), and its follow-up."""
        r, B = self.rng, self.B
        legal = ["lbfgs"] + (["cd_minimize"] if self.cd_ok else []) + (["cd_sweeps"] if self.cd_ok and self.fits else []) + \
            (["cd_sweep"] if self.cd_ok and B == 1 else []) + \
            (["sketch_target", "sketch_generate", "sketch_draw", "sketch_adam"] if self.sketch_ok else [])
        if which is None:   # (behind results_async: one of the calls that run for long, not the target upload or the draw)
            among = [c for c in legal if c not in ("sketch_target", "sketch_draw")] if results_pending else legal
            which = among[int(r.integers(len(among)))]
        if which not in legal:
            return []
        pick = int(r.integers(6)) if ordinal is None else ordinal      # (a card's ordinal decides what a random draw would)
        before = self.host_thetas
        if before is None:   # (a long-running call left its own point in use: hand the host's values over first)
            ops = [self._set(self.thetas())]
            before = self.host_thetas
        else:
            ops = []
        if which == "lbfgs":
            # X and Y at the scale of the isolated tests, whose bounds are used (columns of norm 1 on average: f moves by O(1), not
            # by O(1 / k), and an Armijo test is not decided in the last digits); few backtracks, so that trials get rejected
            for buf in (BUF_X, BUF_Y):
                ops.append(("upload", {"buf": buf, "data": self.mats(B) * np.sqrt(self.k)}))
                self._wrote(buf)
            ops.append(("lbfgs_mat", {"x0": self.thetas(), "maxiter": int(r.integers(1, 3)), "memory": int(r.integers(1, 4)),
                                      "max_backtracks": int(r.choice([1, 2, 4]))}))
            self._lost(BUF_Z, BUF_W, BUF_ZW)
        elif which in ("cd_sweeps", "cd_sweep", "cd_minimize"):
            ops.append(("upload", {"buf": BUF_Y, "data": self.unitaries()}))   # unitary targets, as where the bounds used here were set
            self._wrote(BUF_Y)
            if which == "cd_sweeps":
                cut = pick % 2 == 1
                ops.append(("cd_sweeps", {"th": self.thetas(), "nsweeps": 1 if cut else int(r.integers(1, 3)),
                                          "max_steps": int(r.integers(1, 8)) if cut else -1}))
            elif which == "cd_sweep":
                ops.append(("cd_sweep", {"th": self.thetas()}))
            else:
                route = ["persistent", "wide", "auto"][pick % 3] if self.fits else ["wide", "auto"][pick % 2]
                ops.append(("cd_minimize", {"th": self.thetas(), "maxiter": int(r.integers(1, 3)), "chunk": int(r.integers(1, 3)),
                                            "route": route}))
            self._lost(BUF_X, BUF_Z, BUF_W, BUF_ZW)
        elif which == "sketch_target":
            self.target = True
            return ops + [("sketch_target", {"U": self.unitaries()})]
        elif which == "sketch_draw":
            buf = int(r.choice([BUF_X, BUF_X2, BUF_W]))
            self._wrote(buf)
            self.sketch_no += 1
            return ops + [("sketch_draw", {"kind": ["rand", "eigen"][int(r.integers(2))], "seed": int(r.integers(1, 1000)),
                                           "iteration": self.sketch_no, "buf": buf}), self.read(buf)]
        else:
            if not self.target:
                ops.append(("sketch_target", {"U": self.unitaries()}))
                self.target = True
            kind = ["rand", "alt", "eigen"][pick % 3]
            self.sketch_no += 3
            if which == "sketch_generate":
                om = None
                if kind == "rand":
                    om = r.random((B, self.dim, self.k)) + 1j * r.random((B, self.dim, self.k))
                elif kind == "eigen":
                    om = r.standard_normal((B, self.dim, self.k)) + 1j * r.standard_normal((B, self.dim, self.k))
                ops.append(("sketch_generate", {"kind": kind, "seed": 5, "iteration": self.sketch_no, "omega": om,
                                                "alt_idx": self.alt_idx(1)[0] if kind == "alt" else None}))
                self._wrote(BUF_X, BUF_Y)
                self._lost(BUF_W, BUF_ZW)
            else:
                niter = int(r.integers(1, 3))
                if not self.adam:   # (no run to continue yet: refused, and nothing starts; then every lane starts, or is parked)
                    ops.append(("sketch_adam", {"x0": None, "reset": np.zeros(B, np.int32), "bad": "reset = 0 before any run"}))
                    reset = np.where(np.arange(B) == (pick + 1) % B, 2, 1).astype(np.int32) if B > 1 else np.ones(1, np.int32)
                else:               # (continue, restart, park: every lane in turn)
                    reset = ((np.arange(B) + pick) % 3).astype(np.int32)
                chain = not self.adam
                self.adam = True
                ops.append(("sketch_adam", {"kind": kind, "x0": self.thetas(), "niter": niter, "lr": 0.1, "seed": int(r.integers(1, 1000)),
                                            "iter0": self.sketch_no, "reset": reset,
                                            "alt_idx": self.alt_idx(niter + 1) if kind == "alt" else None}))
                self._lost(BUF_X, BUF_Y, BUF_Z, BUF_W, BUF_ZW)
                if chain:           # a run's first chunk is followed by a second, with whatever the follow-up does in between
                    self.host_thetas = None
                    return self.after_long(ops, before, ordinal) + self.long_call("sketch_adam", None if ordinal is None else ordinal + 1)
        if ops[-1][0] != "sketch_generate":
            self.host_thetas = None
        return self.after_long(ops, before, ordinal)

    def refusals(self):
        """Every call the ABI must refuse on this shape: (those particular to the shape, those every shape has)."""
        B, th, eye = self.B, self.thetas(), np.eye(self.dim, dtype=complex)
        c = []
        if self.kind == "trotter":
            c += [("lbfgs_mat", {"x0": th, "bad": "trotter"}), ("sketch_target", {"U": eye, "bad": "trotter"})]
            c += [("cd_minimize", {"th": th, "bad": "trotter"})] if self.square else []
        if self.square and self.circ.entangler == "cp":
            c += [("cd_minimize", {"th": th, "bad": "cp entangler"}), ("cd_sweeps", {"th": th, "bad": "cp entangler"})]
        if not self.square:
            c += [("set_identity", {"buf": BUF_X, "bad": "identity on a rectangle"}),
                  ("cd_minimize", {"th": th, "bad": "coordinate descent on a rectangle"})]
        if self.kind == "pc" and (self.square or self.k & (self.k - 1)):
            why = "sketching on a square workspace" if self.square else "sketching with k not a power of two"
            c += [("sketch_target", {"U": eye, "bad": why}), ("sketch_draw", {"buf": BUF_X, "bad": why})]
        if self.cd_ok and B > 1:
            c.append(("cd_sweep", {"th": th, "bad": "lanes"}))
        if self.cd_ok and not self.fits:
            c.append(("cd_minimize", {"th": th, "route": "persistent", "bad": "route"}))
        e = [("upload_lane", {"buf": BUF_X, "lane": B, "data": self.mats(1)[0], "bad": "lane"}),
             ("gather", {"buf": BUF_X, "idx": [0, self.dim * self.k], "bad": "index"})]
        if self.kind == "pc":
            e.append(("grad", {"x": BUF_X, "br": (self.nb, self.nb + 1), "bad": "block range"}))
            e += [("use_theta_set", {"i": self.bank_sets + 2, "bad": "index"})] if self.bank_sets else []
        return c, e

    def refused(self, q):
        """Two calls the ABI must refuse here (the q-th of either list), then a read of the buffer they would have written."""
        own, common = self.refusals()
        picks = ([own[q % len(own)]] if own else []) + [common[q % len(common)]]
        return self.ensure(BUF_X) + picks + [("download", {"buf": BUF_X, "lane": None})]

    def sequence(self):
        ops = self.setup()
        for card in self.deck()[self.part[0]::self.part[1]]:
            ops += self.draw(card)
        return ops


def checked_preconditions(ops, batch):
    """The generator's side of the contract, replayed on flags: every read names a specified buffer, no theta-reading call
    follows a long-running one's scribbles."""
    known = {b: False for b in NAMES}
    for name, a in ops:
        if a.get("bad"):
            continue
        if name in ("upload", "broadcast", "set_identity", "sketch_draw") or (name == "upload_lane" and batch == 1):
            known[a["buf"]] = True
        elif name == "apply":
            assert known[a["src"]], f"apply from an unspecified {NAMES[a['src']]}"
            known[a["dst"]] = True
            if a["dst"] == BUF_Z and a["inverse"]:
                known[BUF_ZW] = False
        elif name in ("download", "gather"):
            assert known[a["buf"]], f"{name} of an unspecified {NAMES[a['buf']]}"
        elif name in ("vdot", "vdot_launch"):
            assert known[a["a"]] and known[a["b"]], f"{name} of an unspecified buffer"
        elif name == "copy_out":
            assert known[a["src"]], f"copy_out of an unspecified {NAMES[a['src']]}"
        elif name == "grad":
            assert known[a["x"]] and known[BUF_Z], "grad from an unspecified buffer"
            known[BUF_W] = known[BUF_ZW] = False
        elif name in ("eval", "objective_launch"):
            vdag = name == "objective_launch" or a["vdag"]
            assert known[a["x"]] and (known[BUF_Y] if vdag else known[BUF_Z]), f"{name} from an unspecified buffer"
            if vdag:
                known[BUF_Z], known[BUF_ZW] = True, False
            if name == "objective_launch" or a["grad"]:
                known[BUF_W] = known[BUF_ZW] = False
        elif name == "lbfgs_mat":
            assert known[BUF_X] and known[BUF_Y], "lbfgs_mat without X or Y"
            known[BUF_Z] = known[BUF_W] = known[BUF_ZW] = False
        elif name in ("cd_sweeps", "cd_sweep", "cd_minimize"):
            assert known[BUF_Y], f"{name} without a target"
            known[BUF_X] = known[BUF_Z] = known[BUF_W] = known[BUF_ZW] = False
        elif name == "sketch_generate":
            known[BUF_X] = known[BUF_Y] = True
            known[BUF_W] = known[BUF_ZW] = False
        elif name == "sketch_adam":
            for b in (BUF_X, BUF_Y, BUF_Z, BUF_W, BUF_ZW):
                known[b] = False
    return True


# ---- the oracle's rendering of the workspace -------------------------------------------------------------------------------

class FakeMatWorkspace:
    """What a correct matrix workspace returns, computed with the oracle.  A buffer the contract leaves unspecified is filled
    with NaN: a model that read it would fail.  The planted-fault variants of tests/test_ws_model_mat.py override one method."""

    def __init__(self, circ, batch, ncols, orc=None, fits_one_launch=True, trotter=False):
        self.circ, self.batch, self.ncols, self.T, self.nb = circ, batch, ncols, circ.num_thetas, circ.num_blocks
        self.dim = 1 << circ.num_qubits
        self.orc = orc or MatOracle(circ)
        self.fits, self.trotter = fits_one_launch, trotter
        self.b = {key: np.zeros((batch, self.dim, ncols), complex) for key in NAMES}
        self.th = np.zeros((batch, self.T))
        self.bank = None
        self.g = np.zeros((batch, self.T), complex)
        self.vd = self.target = self.adam = self._res = None
        self._gen = [0] * 6

    # -- bookkeeping
    def _touch(self, *bufs):
        for buf in bufs:
            self._gen[buf] += 1

    def generation(self, buf):
        return self._gen[buf]

    def _put(self, buf, value):
        self._touch(buf)
        self.b[buf] = np.array(value, complex).reshape(self.batch, self.dim, self.ncols)

    def _scribble(self, *bufs):
        for buf in bufs:
            self._touch(buf)
            self.b[buf] = np.full((self.batch, self.dim, self.ncols), np.nan + 0j)

    def _lanes(self, fn, *arrays):
        return np.stack([fn(self.th[b], *[a[b] for a in arrays]) for b in range(self.batch)])

    def _no_trotter(self):
        if self.trotter:
            raise RuntimeError("aqc_hip: matrix path does not support the Trotter ansatz")

    def _sketching(self):
        self._no_trotter()
        k = self.ncols
        if k >= self.dim or k > 64 or k & (k - 1):
            raise RuntimeError("aqc_hip: sketching needs a power of two below the dimension")

    def _cd(self):
        if self.ncols != self.dim:
            raise RuntimeError("aqc_hip: coordinate descent needs a square workspace (ncols == 2^n)")
        if self.circ.entangler == "cp":
            raise RuntimeError("aqc_hip: CPhase entangler is not supported yet")
        self._no_trotter()

    # -- data
    def set_thetas(self, th):
        self.th = np.array(th, float).reshape(self.batch, self.T)

    def theta_bank(self, bank):
        self.bank = np.array(bank, float).reshape(-1, self.batch, self.T)

    def use_theta_set(self, i):
        if self.bank is None or not 0 <= i < self.bank.shape[0]:
            raise RuntimeError("aqc_hip: theta set out of range")
        self.th = self.bank[i].copy()

    def upload(self, buf, data, lane=None):
        if lane is None:
            return self._put(buf, data)
        if not 0 <= lane < self.batch:
            raise RuntimeError("aqc_hip: lane out of range")
        self._touch(buf)
        self.b[buf][lane] = data

    def broadcast(self, buf, data):
        self._put(buf, np.broadcast_to(np.asarray(data, complex), (self.batch, self.dim, self.ncols)))

    def download(self, buf, lane=None):
        return self.b[buf].copy() if lane is None else self.b[buf][lane].copy()

    def copy_lane_from(self, src, src_buf, src_lane, dst_buf, dst_lane):
        self._touch(dst_buf)
        self.b[dst_buf][dst_lane] = src.b[src_buf][src_lane]

    def set_identity(self, buf):
        if self.ncols != self.dim:
            raise RuntimeError("aqc_hip: identity needs a square workspace (ncols == 2^n)")
        self._put(buf, np.broadcast_to(np.eye(self.dim, dtype=complex), (self.batch, self.dim, self.dim)))

    # -- compute
    def apply(self, inverse, src=BUF_Y, dst=BUF_Z):
        self._put(dst, self._lanes(self.orc.vdag if inverse else self.orc.v, self.b[src]))
        if inverse and dst == BUF_Z:
            self._scribble(BUF_ZW)

    def grad_from(self, x, br=None, front=True):
        if br is not None and not (0 <= br[0] < br[1] <= self.nb):
            raise RuntimeError(f"aqc_hip: invalid block_range [{br[0]}, {br[1]})")
        self.g = self._lanes(self.orc.grad, self.b[x], self.b[BUF_Z])
        self._scribble(BUF_W, BUF_ZW)

    def grad(self, br=None, front=True):
        self.grad_from(BUF_X, br, front)

    def get_grads(self):
        return self.g.copy()

    def eval(self, thetas=None, vdag=True, gather=False, grad=True, x_buf=BUF_X, block_range=None, front_layer=True):
        if thetas is not None:
            self.set_thetas(thetas)
        if vdag:
            self.apply(True, BUF_Y, BUF_Z)
        if grad:
            self.grad_from(x_buf)
        return None, (self.g.copy() if grad else None)

    def objective_launch(self, x_buf=BUF_X, block_range=None, front_layer=True):
        self.apply(True, BUF_Y, BUF_Z)
        self.grad_from(x_buf)

    def results_async(self):
        self._res = self.g.copy()

    def results_fetch(self, small=True, grads=True):
        return None, self._res

    def gather(self, buf, index):
        idx = np.asarray(index, np.int64)
        if np.any(idx < 0) or np.any(idx >= self.dim * self.ncols):
            raise RuntimeError("aqc_hip: gather index out of range")
        return self.b[buf].reshape(self.batch, -1)[:, idx]

    def vdot(self, a, b):
        return np.einsum("bik,bik->b", np.conj(self.b[a]), self.b[b])

    def vdot_launch(self, a, b):
        self.vd = self.vdot(a, b)

    def vdot_fetch(self):
        return self.vd.copy()

    # -- long-running calls
    def lbfgs_mat(self, x0, *, maxiter=100, memory=10, gtol=1e-7, ftol=1e-12, fobj_thr=0.0, fidelity_thr=0.0, max_backtracks=12):
        self._no_trotter()
        ref = lbfgs_reference(self.orc, self.b[BUF_X], self.b[BUF_Y], np.array(x0, float), maxiter, memory, max_backtracks)
        self._scribble(BUF_Z, BUF_W, BUF_ZW)
        self._lbfgs_exit(ref)
        return {"x": ref["x"].copy(), "fun": ref["fun"].copy(), "fidelity": np.zeros(self.batch), "nit": ref["nit"], "nfev": ref["nfev"],
                "status": np.zeros(self.batch, np.int32)}

    def _lbfgs_exit(self, ref):
        self.th = ref["x"].copy()

    def cd_sweeps(self, thetas, nsweeps=1, max_steps=-1):
        self._cd()
        if not self.fits:
            raise RuntimeError("aqc_hip: the operands of this coordinate descent do not fit one workgroup's LDS")
        ths, fobj = cd_reference(self.circ, np.array(thetas, float).reshape(self.batch, self.T), self.b[BUF_Y], nsweeps, max_steps)
        self._scribble(BUF_X, BUF_Z, BUF_W, BUF_ZW)
        self.th = ths[-1].copy()
        return ths[-1].copy(), fobj

    def cd_sweep(self, thetas):
        self._cd()
        if self.batch != 1:
            raise RuntimeError("aqc_hip: aqc_ws_cd_sweep takes a single-lane workspace")
        ths, fobj = cd_reference(self.circ, np.array(thetas, float).reshape(1, self.T), self.b[BUF_Y], 1, -1)
        self._scribble(BUF_X, BUF_Z, BUF_W, BUF_ZW)
        self.th = ths[-1].copy()
        return ths[-1][0].copy(), float(fobj[0, 0])

    def cd_minimize(self, thetas0, maxiter, *, chunk=64, dtheta_thr=1e-8, fobj_thr=1e-2, time_limit=-1.0, route="auto", max_steps=-1):
        self._cd()
        if route == "persistent" and not self.fits:
            raise RuntimeError("aqc_hip: the persistent route is not available")
        wide = route == "wide" or not self.fits
        ths, fobj = cd_reference(self.circ, np.array(thetas0, float).reshape(self.batch, self.T), self.b[BUF_Y], maxiter, -1)
        best_th, best_f, _ = cd_best(ths, fobj)
        self._cd_exit(wide, ths, best_th)
        return {"thetas": best_th.copy(), "cost": best_f.copy(), "nit": np.full(self.batch, maxiter), "status": np.ones(self.batch, np.int32),
                "profile": fobj}

    def _cd_exit(self, wide, ths, best_th):
        self._scribble(BUF_X, BUF_Z, BUF_W, BUF_ZW)
        self.th = best_th.copy()

    def sketch_target(self, target, shared=None):
        self._sketching()
        self.target = np.array(np.broadcast_to(np.asarray(target, complex), (self.batch, self.dim, self.dim)))

    def _eigen_thetas(self):
        return self.th

    def sketch_generate(self, kind, seed=0, iteration=0, alt_idx=None, omega=None, status=True):
        self._sketching()
        th = self._eigen_thetas()
        pairs = [sketch_pair(self.orc, kind, self.target[b], self.ncols, th[b] if kind == "eigen" else None,
                             None if omega is None else omega[b], None if alt_idx is None else alt_idx[b]) for b in range(self.batch)]
        self._prev_thetas = self.th.copy()
        self._put(BUF_X, np.stack([p[0] for p in pairs]))
        self._put(BUF_Y, np.stack([p[1] for p in pairs]))
        self._scribble(BUF_W, BUF_ZW)
        return np.zeros(self.batch, np.int32)

    def sketch_draw(self, kind, seed=0, iteration=0, buf=BUF_X):
        self._sketching()
        self._put(buf, np.stack([sk.omega(SKETCH_CODE[kind], seed, iteration, b, self.dim, self.ncols) for b in range(self.batch)]))

    def _adam_resume(self, lane):
        return self.adam[lane]["x"]

    def sketch_adam(self, kind, x0, niter, lr, *, beta1=0.9, beta2=0.99, eps=1e-8, tol=1e-6, seed=0, iter0=0, reset=None, alt_idx=None):
        self._sketching()
        reset = np.broadcast_to(np.asarray(1 if reset is None and self.adam is None else 0 if reset is None else reset), (self.batch,))
        if self.adam is None and (reset == 0).any():
            raise RuntimeError("aqc_hip: a lane continues a run that has not started")
        if self.adam is None:
            self.adam = [dict(m=np.zeros(self.T), v=np.zeros(self.T), t=0, x=self.th[b].copy(), best_f=0.0, best_x=np.zeros(self.T), flag=0)
                         for b in range(self.batch)]
        prof, nit = np.zeros((self.batch, niter + 1)), np.zeros(self.batch, np.int64)
        for b in range(self.batch):
            st = dict(self.adam[b], x=np.array(self._adam_resume(b), float))
            if reset[b] == 1:
                st.update(m=np.zeros(self.T), v=np.zeros(self.T), t=0, x=np.array(x0[b], float), best_f=np.inf, flag=0)
            elif reset[b] == 2:
                st["flag"] = 2
            self.adam[b], prof[b], nit[b] = adam_lane(self.orc, kind, self.target[b], self.ncols, b, st, niter, lr, seed, iter0, alt_idx)
        self._scribble(BUF_X, BUF_Y, BUF_Z, BUF_W, BUF_ZW)
        self.th = np.stack([s["x"] for s in self.adam])
        return {"x": self.th.copy(), "profile": prof, "nit": nit, "cost": prof[np.arange(self.batch), nit],
                "best_f": np.array([s["best_f"] for s in self.adam]), "best_x": np.stack([s["best_x"] for s in self.adam]),
                "status": np.zeros(self.batch, np.int32)}

    def close(self):
        pass


class MatKit:
    """The matrix workspace's side of wm.run_sequence: bind the number of columns with MatKit(ncols)."""

    def __init__(self, ncols):
        self.ncols = ncols

    def models(self, orc, batch, circ):
        return MatModel(orc, batch, circ, self.ncols), MatModel(orc, batch, circ, self.ncols)

    def prepare_second(self, ws2, model2, batch, circ):
        rng = np.random.default_rng(54321)
        shape = (batch, 1 << circ.num_qubits, self.ncols)
        y2 = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
        y2 /= np.linalg.norm(y2.reshape(batch, -1), axis=1)[:, None, None]
        ws2.upload(BUF_Y, y2)
        model2.write(BUF_Y, y2)
        ws2.upload(BUF_X, y2[::-1].copy())
        model2.write(BUF_X, y2[::-1].copy())

    apply_op = staticmethod(apply_op)


# ---- the shapes both test files play (CPU: on FakeMatWorkspace; GPU: on engine.Workspace) ----------------------------------------

def _pc(n, ent, depth):
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    return ParametricCircuit(n, ent, create_ansatz_structure(n, "spin", "full", depth))


def _trotter(n, layers):
    from aqc_research_amd import TrotterAnsatz
    from aqc_research_amd.circuit_structures import make_trotter_like_circuit

    return TrotterAnsatz(n, make_trotter_like_circuit(n, layers), second_order=True)


# name -> (circuit, ncols, tile bits (0: the default), lanes, coordinate descent fits one launch, kind, seeds).  The first four are the
# smallest with two stages, a mirrored V^H with its checkpoint: the matrix-core kernels take tiles of 2^8 elements at least, two of
# their bits stay column bits, so a stage holds six qubits and two stages start at seven.  Coordinate descent fits one launch up to
# six qubits only: sq6 has two stages on the VALU kernel families (2^7 tiles) and one on the matrix cores.  The rest exist for the
# calls and refusals those cannot reach: aqc_ws_cd_sweep (one lane), the cp entangler handed to coordinate descent (square, cp), a
# Trotter ansatz.
SHAPES = {
    "sq6": (lambda: _pc(6, "cx", 6), 64, 7, 3, True, "pc", (1, 2, 3)),
    "sq7": (lambda: _pc(7, "cz", 7), 128, 8, 2, False, "pc", (1, 2, 3)),
    "sk7": (lambda: _pc(7, "cp", 6), 8, 8, 3, False, "pc", (1, 2, 3)),
    "rect7": (lambda: _pc(7, "cx", 8), 3, 8, 2, False, "pc", (1, 2, 3)),
    "sq6_1": (lambda: _pc(6, "cx", 6), 64, 7, 1, True, "pc", (1, 2, 3)),
    "cp3sq": (lambda: _pc(3, "cp", 6), 8, 0, 2, True, "pc", (1, 2, 3)),
    "trot4": (lambda: _trotter(4, 1), 2, 0, 2, False, "trotter", (1,)),
}


def planned_stages(ctx, ncols, tile):
    """Stages of V^H, the sweep and V as a workspace plans them (host only): the fewest over the low-bit choices it tries."""
    return [min(len(ctx.plan(which, ncols, tile, low_bits)) for low_bits in (3, 2)) for which in (0, 1, 2)]


def sequence(name, seed, circ=None):
    make, ncols, _, lanes, fits, kind, seeds = SHAPES[name]
    return MatGen(seed, circ or make(), lanes, ncols, fits, kind, part=(seeds.index(seed), len(seeds))).sequence()


# ---- directed sequences: one per finding; the device test plays them, the CPU test checks their decision margins -------------------

PROBE = [("apply", {"inverse": False, "src": BUF_X2, "dst": BUF_W}), ("download", {"buf": BUF_W, "lane": None})]


def opening(name, seed, circ, scale=1.0):
    """(generator, [Y, X, X2, thetas]) of a directed sequence on shape `name`; Y and X scaled by `scale`."""
    _, ncols, _, lanes = SHAPES[name][:4]
    g = MatGen(seed, circ, lanes, ncols, True)
    ops = [("upload", {"buf": BUF_Y, "data": g.mats(lanes) * scale}), ("upload", {"buf": BUF_X, "data": g.mats(lanes) * scale}),
           ("upload", {"buf": BUF_X2, "data": g.mats(lanes)}), ("set_thetas", {"th": g.thetas()})]
    return g, ops


def directed(circ_of):
    """key -> (shape, operations, extras).  `circ_of(name)` hands out the circuit of a shape."""
    out = {}
    # aqc_ws_lbfgs_mat with one trial per line search: a lane that rejects it ends at x_out with the trial in the theta buffer
    name = "sk7"
    circ, (_, ncols, _, lanes) = circ_of(name), SHAPES[name][:4]
    g, ops = opening(name, 21, circ, np.sqrt(8.0))
    x0 = g.thetas()
    om = g.rng.standard_normal((lanes, circ.dimension, ncols)) + 1j * g.rng.standard_normal((lanes, circ.dimension, ncols))
    ops += [("sketch_target", {"U": g.unitaries()}),
            ("lbfgs_mat", {"x0": x0, "maxiter": 2, "memory": 2, "max_backtracks": 1}),
            ("eval", {"th": None, "vdag": True, "grad": True, "x": BUF_X}), ("download", {"buf": BUF_Z, "lane": None})] + PROBE + \
           [("sketch_generate", {"kind": "eigen", "seed": 1, "iteration": 1, "omega": om, "alt_idx": None})]
    out["lbfgs"] = (name, ops, {})
    for name, route in (("sq6", "persistent"), ("sq6", "wide"), ("sq7", "wide"), ("sq7", "auto")):
        g, ops = opening(name, 22, circ_of(name))
        ops += [("upload", {"buf": BUF_Y, "data": g.unitaries()}),
                ("cd_minimize", {"th": g.thetas(), "maxiter": 2, "chunk": 1, "route": route}),
                ("set_identity", {"buf": BUF_X}), ("apply", {"inverse": False, "src": BUF_X, "dst": BUF_W}),
                ("download", {"buf": BUF_W, "lane": None}), ("vdot", {"a": BUF_W, "b": BUF_Y})]
        out[f"cd_minimize:{name}:{route}"] = (name, ops, {})
    for name in ("sq6", "sq6_1"):
        g, ops = opening(name, 23, circ_of(name))
        ops += [("upload", {"buf": BUF_Y, "data": g.unitaries()}), ("cd_sweeps", {"th": g.thetas(), "nsweeps": 2, "max_steps": -1})] + PROBE
        if SHAPES[name][3] == 1:
            ops += [("cd_sweep", {"th": g.thetas()})] + PROBE
        out[f"cd_sweeps:{name}"] = (name, ops, {})
    # ADAM in one run of four iterations; the device test also plays it as two chunks with a visit to `other` in between
    for kind in ("alt", "eigen"):
        name = "sk7"
        g, ops = opening(name, 24, circ_of(name))
        u, x0, other = g.unitaries(), g.thetas(), g.thetas()
        ops += [("sketch_target", {"U": u}),
                ("sketch_adam", {"kind": kind, "x0": x0, "niter": 4, "lr": 0.1, "seed": 9, "iter0": 0, "reset": np.ones(3, np.int32),
                                 "alt_idx": g.alt_idx(5) if kind == "alt" else None})]
        out[f"adam:{kind}"] = (name, ops, {"other": other})
    for name, call in (("rect7", "lbfgs_mat"), ("sq7", "cd_minimize"), ("sk7", "sketch_adam")):
        ncols, lanes = SHAPES[name][1], SHAPES[name][3]
        g, ops = opening(name, 25, circ_of(name), np.sqrt(ncols) if call == "lbfgs_mat" else 1.0)
        ops += [("objective_launch", {"x": BUF_X}), ("results_async", {})]
        if call == "lbfgs_mat":
            ops.append(("lbfgs_mat", {"x0": g.thetas(), "maxiter": 2, "memory": 3, "max_backtracks": 4}))
        elif call == "cd_minimize":
            ops += [("upload", {"buf": BUF_Y, "data": g.unitaries()}),
                    ("cd_minimize", {"th": g.thetas(), "maxiter": 1, "chunk": 1, "route": "wide"})]
        else:
            ops += [("sketch_target", {"U": g.unitaries()}),
                    ("sketch_adam", {"kind": "rand", "x0": g.thetas(), "niter": 2, "lr": 0.1, "seed": 4, "iter0": 0,
                                     "reset": np.ones(lanes, np.int32), "alt_idx": None})]
        out[f"results:{name}:{call}"] = (name, ops + [("results_fetch", {})] + PROBE, {})
    g, ops = opening("sq6", 26, circ_of("sq6"), np.sqrt(64.0))
    ops += [("lbfgs_mat", {"x0": g.thetas(), "maxiter": 1, "memory": 1, "max_backtracks": 2}),
            ("upload", {"buf": BUF_Y, "data": g.unitaries()}),
            ("cd_minimize", {"th": g.thetas(), "maxiter": 2, "chunk": 2, "route": "persistent"}),
            ("cd_minimize", {"th": g.thetas(), "maxiter": 1, "chunk": 1, "route": "wide"})] + PROBE + \
           [("upload", {"buf": BUF_X, "data": g.mats(3) * np.sqrt(64.0)}),
            ("lbfgs_mat", {"x0": g.thetas(), "maxiter": 2, "memory": 2, "max_backtracks": 4})] + PROBE
    out["back_to_back:sq6"] = ("sq6", ops, {})
    g, ops = opening("sk7", 27, circ_of("sk7"), np.sqrt(8.0))
    adam = {"kind": "rand", "x0": g.thetas(), "niter": 2, "lr": 0.1, "seed": 6, "iter0": 0, "reset": np.ones(3, np.int32), "alt_idx": None}
    ops += [("sketch_target", {"U": g.unitaries()}), ("sketch_adam", adam),
            ("upload", {"buf": BUF_Y, "data": g.mats(3) * np.sqrt(8.0)}), ("upload", {"buf": BUF_X, "data": g.mats(3) * np.sqrt(8.0)}),
            ("lbfgs_mat", {"x0": g.thetas(), "maxiter": 2, "memory": 2, "max_backtracks": 4}),
            ("sketch_adam", dict(adam, x0=None, iter0=2, reset=np.array([0, 2, 0], np.int32)))] + PROBE
    out["back_to_back:sk7"] = ("sk7", ops, {})
    g, ops = opening("rect7", 28, circ_of("rect7"))
    ops += [("apply", {"inverse": True, "src": BUF_Y, "dst": BUF_Z}), ("set_identity", {"buf": BUF_Z, "bad": "identity on a rectangle"}),
            ("download", {"buf": BUF_Z, "lane": None}), ("grad", {"x": BUF_X, "plain": True}), ("get_grads", {})]
    out["identity:rect7"] = ("rect7", ops, {})
    return out
