"""Shadow model of one long-lived engine.Workspace, a seeded generator of call sequences and the runner that plays a
sequence on a workspace and checks every read against the model.

The model follows the buffer rules of include/aqc_hip.h (buffer paragraph, one-call evaluations, surrogate objective):

- Z after apply(True, Y, Z), eval(vdag=True), objective_launch or surrogate_eval is V^H(theta) Y for the theta and Y of
  that call.  Once the thetas (or Y) have changed, a reader of Z returns exactly that old value, or raises RuntimeError
  ("BUF_Z holds") -- the latter only when the last writer of Z was a one-call evaluation, which may have left Z partial.
  A writer of some lanes of Z in that state may refuse with the same message.
- W and ZW are known only after a call that writes them as data (upload, broadcast, upload_lane, copy_lane, apply);
  every sweep, evaluation or V^H into Z makes them UNKNOWN.  X2 is UNKNOWN after surrogate_eval.  UNKNOWN buffers are
  never read.
- A refused call (bad block_range, bad max_no, an index or lane out of range) changes nothing.

Expected values come from the compiled CPU restatement (oracle/aqc_ref.py), memoised by digest of (thetas, operand).
FakeWorkspace computes every call from the same oracle: it lets the generator and the runner be checked without a GPU.
"""
import hashlib
import re

import numpy as np

from oracle import aqc_ref as cref

BUF_Y, BUF_Z, BUF_X, BUF_W, BUF_ZW, BUF_X2 = range(6)
NAMES = {BUF_Y: "Y", BUF_Z: "Z", BUF_X: "X", BUF_W: "W", BUF_ZW: "ZW", BUF_X2: "X2"}
TOL = 1e-10
Z_REFUSED = re.compile("BUF_Z holds")


def _digest(*arrays) -> bytes:
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.digest()


class Oracle:
    """Per-lane V, V^H and gradients of one circuit, memoised (a sequence repeats its operands; the configurations of one
    seed repeat the whole sequence)."""

    def __init__(self, circ):
        self.circ = circ
        self.memo = {}

    def _get(self, kind, fn, *args):
        key = (kind, _digest(*[np.asarray(a) for a in args[:3]]), args[3:])
        if key not in self.memo:
            self.memo[key] = fn()
        return self.memo[key]

    def vdag(self, th, y):
        return self._get("vh", lambda: cref.v_dagger_mul_vec(self.circ, th, y), th, y)

    def v(self, th, y):
        return self._get("v", lambda: cref.v_mul_vec(self.circ, th, y), th, y)

    def grad(self, th, x, z, block_range=None, front=True):
        br = None if block_range is None else tuple(block_range)
        return self._get("g", lambda: cref.grad_of_dot_product(self.circ, th, x, z, br, front), th, x, z, br, bool(front))


def surrogate_lane(orc: Oracle, th, y, idx, weight, max_no, update_state, block_range, front):
    """One lane of aqc_ws_surrogate_eval (objective_lhs_sur_max.py:82-191): returns (f, fidelity, hs, complex grad, weight,
    max_no, lhs state of the one sweep)."""
    z = orc.vdag(th, y)
    hs = z[idx]
    hs2 = np.abs(hs) ** 2
    w, mx = float(weight), int(max_no)
    if update_state:
        best = hs2[mx]
        for i in range(idx.size):
            if 1.1 * best < hs2[i]:
                best, mx = hs2[i], i
    if update_state == 1:
        f_old = 1.0 - (1.0 - w) * hs2[0] - w * hs2[mx]
        w = w + 0.1 * (np.sqrt(abs(f_old)) - w)
    f = 1.0 - (1.0 - w) * hs2[0] - w * hs2[mx]
    c0, cm = -2 * (1 - w) * np.conj(hs[0]), -2 * w * np.conj(hs[mx])
    x = np.zeros(z.size, complex)
    x[idx[0]] += np.conj(c0)
    x[idx[mx]] += np.conj(cm)
    return f, hs2[0], hs, orc.grad(th, x, z, block_range, front), w, mx, x


class Model:
    """Logical content of one workspace (see the module docstring)."""

    def __init__(self, orc: Oracle, batch: int, n: int):
        self.orc, self.B, self.dim = orc, batch, 1 << n
        self.bufs = {b: None for b in NAMES}
        self.thetas = None
        self.bank = None
        self.gather = None
        self.small = None                 # d_small: the last registered gather (gather_launch, evaluations)
        self.vdot = None
        self.grads = None
        self.z_one_call = False           # the last writer of Z was a one-call evaluation ...
        self.z_stale = False              # ... and the thetas or Y have changed since: a reader may refuse

    # -- helpers -------------------------------------------------------------
    def z_refusable(self) -> bool:
        return self.z_one_call and self.z_stale

    def new_thetas(self, th):
        self.thetas = np.array(th, float)
        if self.z_one_call:
            self.z_stale = True

    def write(self, buf, value, lanes=None):
        """Data written to `buf` (all lanes, or the listed ones)."""
        if lanes is None:
            self.bufs[buf] = np.array(value, complex)
        else:
            cur = self.bufs[buf]
            cur = np.zeros((self.B, self.dim), complex) if cur is None else cur.copy()
            for lane, v in zip(lanes, value):
                cur[lane] = v
            self.bufs[buf] = cur if self.bufs[buf] is not None or len(lanes) == self.B else None
        if buf == BUF_Z:
            self.z_one_call = self.z_stale = False
        if buf == BUF_Y and self.z_one_call:
            self.z_stale = True

    def vdag_all(self, y=None):
        y = self.bufs[BUF_Y] if y is None else y
        return np.stack([self.orc.vdag(self.thetas[b], y[b]) for b in range(self.B)])

    def evaluation_writes_z(self):
        self.bufs[BUF_Z] = self.vdag_all()
        self.bufs[BUF_W] = self.bufs[BUF_ZW] = None
        self.z_one_call, self.z_stale = True, False

    def sweep(self, x_buf, block_range, front):
        z, x = self.bufs[BUF_Z], self.bufs[x_buf]
        self.grads = np.stack([self.orc.grad(self.thetas[b], x[b], z[b], block_range, front) for b in range(self.B)])
        self.bufs[BUF_W] = self.bufs[BUF_ZW] = None
        return self.grads


# ------------------------------------------------------------------------------------------------------------------------
# operation catalogue: op = (name, dict); `apply_op` performs one on a workspace and the model, returns the reads
# ------------------------------------------------------------------------------------------------------------------------

def _block_range(br):
    return None if br is None else tuple(br)


def apply_op(ws, model: Model, op, ws2=None, model2=None):
    """Run `op` on `ws` (`ws2`: a second workspace on the same context, for copy_lane) and update the model(s).  Returns
    the (label, got, expected) of every read the operation made."""
    name, a = op
    reads = []
    m = model

    def z_read(fn, label, expected):
        """A reader of Z: its value, or (only when allowed) the readers' refusal."""
        if m.z_refusable():
            try:
                got = fn()
            except RuntimeError as e:
                assert Z_REFUSED.search(str(e)), f"{label}: unexpected error {e}"
                return None
            reads.append((label, got, expected()))
            m.z_stale = m.z_one_call = False
            return got
        got = fn()
        reads.append((label, got, expected()))
        return got

    def refused(fn):
        try:
            fn()
        except (RuntimeError, ValueError):
            return
        raise AssertionError(f"{name} {a.get('why', '')}: the call was expected to be refused")

    if name == "set_thetas":
        ws.set_thetas(a["th"])
        m.new_thetas(a["th"])
    elif name == "theta_bank":
        ws.theta_bank(a["bank"])
        m.bank = np.array(a["bank"], float)
    elif name == "use_theta_set":
        if a["i"] >= m.bank.shape[0]:
            return refused(lambda: ws.use_theta_set(a["i"])) or reads
        ws.use_theta_set(a["i"])
        m.new_thetas(m.bank[a["i"]])
    elif name == "upload":
        ws.upload(a["buf"], a["data"])
        m.write(a["buf"], a["data"])
    elif name == "broadcast":
        ws.broadcast(a["buf"], a["data"])
        m.write(a["buf"], np.broadcast_to(a["data"], (m.B, m.dim)))
    elif name == "upload_lane":
        if not 0 <= a["lane"] < m.B:
            return refused(lambda: ws.upload(a["buf"], a["data"], lane=a["lane"])) or reads
        if a["buf"] == BUF_Z and m.z_refusable() and m.B > 1:
            try:
                ws.upload(a["buf"], a["data"], lane=a["lane"])
            except RuntimeError as e:
                assert Z_REFUSED.search(str(e)), f"upload_lane(Z): unexpected error {e}"
                return reads
        else:
            ws.upload(a["buf"], a["data"], lane=a["lane"])
        m.write(a["buf"], [a["data"]], lanes=[a["lane"]])
    elif name == "set_basis":
        if any(not 0 <= i < m.dim for i in a["idx"]):
            return refused(lambda: ws.set_basis(a["buf"], a["idx"])) or reads
        ws.set_basis(a["buf"], a["idx"])
        x = np.zeros((m.B, m.dim), complex)
        x[np.arange(m.B), a["idx"]] = 1
        m.write(a["buf"], x)
    elif name == "set_combo":
        ws.set_combo(a["buf"], a["idx"], a["coef"])
        x = np.zeros((m.B, m.dim), complex)
        for b in range(m.B):
            x[b, a["idx"][b][0]] += a["coef"][b][0]
            if a["idx"][b][1] >= 0:
                x[b, a["idx"][b][1]] += a["coef"][b][1]
        m.write(a["buf"], x)
    elif name == "gather_setup":
        if any(not 0 <= i < m.dim for i in a["idx"]):
            return refused(lambda: ws.gather_setup(a["idx"])) or reads
        ws.gather_setup(a["idx"])
        m.gather = np.array(a["idx"], np.int64)
        m.small = None   # (the result buffer may be reallocated)
    elif name == "apply":
        inv, src, dst = a["inverse"], a["src"], a["dst"]
        f = m.orc.vdag if inv else m.orc.v
        expected = lambda: np.stack([f(m.thetas[b], m.bufs[src][b]) for b in range(m.B)])   # noqa: E731
        if src == BUF_Z and m.z_refusable():
            try:
                ws.apply(inv, src, dst)
            except RuntimeError as e:
                assert Z_REFUSED.search(str(e)), f"apply from Z: unexpected error {e}"
                return reads
            m.z_stale = m.z_one_call = False
        else:
            ws.apply(inv, src, dst)
        val = expected()
        m.write(dst, val)
        if dst == BUF_Z:
            m.bufs[BUF_ZW] = None if inv else m.bufs[BUF_ZW]   # (the mirrored V^H keeps its checkpoint there)
    elif name == "grad":
        br = _block_range(a["br"])
        if a.get("bad"):
            return refused(lambda: ws.grad_from(a["x"], br, a["front"])) or reads
        if m.z_refusable():
            try:
                ws.grad_from(a["x"], br, a["front"])
            except RuntimeError as e:
                assert Z_REFUSED.search(str(e)), f"grad_from: unexpected error {e}"
                return reads
            m.z_stale = m.z_one_call = False
        else:
            ws.grad_from(a["x"], br, a["front"])
        m.sweep(a["x"], br, a["front"])
    elif name == "objective_launch":
        br = _block_range(a["br"])
        if a.get("bad"):
            return refused(lambda: ws.objective_launch(a["x"], br, a["front"])) or reads
        ws.objective_launch(a["x"], br, a["front"])
        m.evaluation_writes_z()
        if m.gather is not None:
            m.small = m.bufs[BUF_Z][:, m.gather]
        m.sweep(a["x"], br, a["front"])
    elif name == "eval":
        br = _block_range(a["br"])
        if a.get("bad"):
            return refused(lambda: ws.eval(a["th"], a["vdag"], a["gather"], a["grad"], a["x"], br, a["front"])) or reads
        reads_z = not a["vdag"] and (a["gather"] or a["grad"])
        if reads_z and m.z_refusable():
            try:
                hs, g = ws.eval(a["th"], a["vdag"], a["gather"], a["grad"], a["x"], br, a["front"])
            except RuntimeError as e:
                assert Z_REFUSED.search(str(e)), f"eval: unexpected error {e}"
                return reads
            m.z_stale = m.z_one_call = False
        else:
            hs, g = ws.eval(a["th"], a["vdag"], a["gather"], a["grad"], a["x"], br, a["front"])
        if a["th"] is not None:
            m.new_thetas(a["th"])
        if a["vdag"]:
            m.evaluation_writes_z()
        if a["gather"]:
            m.small = m.bufs[BUF_Z][:, m.gather]
            reads.append(("eval.gathered", hs, m.small))
        if a["grad"]:
            reads.append(("eval.grads", g, m.sweep(a["x"], br, a["front"])))
    elif name == "surrogate_eval":
        br = _block_range(a["br"])
        weight, max_no = a["weight"].copy(), a["max_no"].copy()
        if a.get("bad"):
            return refused(lambda: ws.surrogate_eval(a["th"], weight, max_no, a["update"], br, a["front"], a["real_only"])) or reads
        f, fid, hs, g = ws.surrogate_eval(a["th"], weight, max_no, a["update"], br, a["front"], a["real_only"])
        m.new_thetas(a["th"])
        m.evaluation_writes_z()
        res = [surrogate_lane(m.orc, m.thetas[b], m.bufs[BUF_Y][b], m.gather, a["weight"][b], a["max_no"][b], a["update"], br,
                              a["front"]) for b in range(m.B)]
        m.grads = np.stack([r[3] for r in res])
        m.small = np.stack([r[2] for r in res])
        m.bufs[BUF_X2] = None
        reads += [("surrogate.f", f, np.array([r[0] for r in res])), ("surrogate.hs", hs, m.small),
                  ("surrogate.grad", g, m.grads.real if a["real_only"] else m.grads)]
        if a["update"]:
            reads += [("surrogate.fidelity", fid, np.array([r[1] for r in res])),
                      ("surrogate.weight", weight, np.array([r[4] for r in res])),
                      ("surrogate.max_no", max_no.astype(float), np.array([r[5] for r in res], float))]
    elif name == "download":
        buf, lane = a["buf"], a["lane"]
        exp = (lambda: m.bufs[buf]) if lane is None else (lambda: m.bufs[buf][lane])
        if buf == BUF_Z:
            z_read(lambda: ws.download(buf, lane), f"download({NAMES[buf]}, {lane})", exp)
        else:
            reads.append((f"download({NAMES[buf]}, {lane})", ws.download(buf, lane), exp()))
    elif name == "gather":
        buf, idx = a["buf"], np.array(a["idx"], np.int64)
        exp = lambda: m.bufs[buf][:, idx]   # noqa: E731
        if buf == BUF_Z:
            z_read(lambda: ws.gather(buf, idx), "gather(Z)", exp)
        else:
            reads.append((f"gather({NAMES[buf]})", ws.gather(buf, idx), exp()))
    elif name == "gather_launch":
        buf = a["buf"]
        exp = lambda: m.bufs[buf][:, m.gather]   # noqa: E731
        if buf == BUF_Z and m.z_refusable():
            try:
                ws.gather_launch(buf)
            except RuntimeError as e:
                assert Z_REFUSED.search(str(e)), f"gather_launch: unexpected error {e}"
                return reads
        else:
            ws.gather_launch(buf)
        m.small = exp()
        reads.append((f"gather_launch({NAMES[buf]})+fetch", ws.gather_fetch(), m.small))
    elif name in ("vdot", "vdot_launch"):
        ba, bb = a["a"], a["b"]
        exp = lambda: np.einsum("bi,bi->b", np.conj(m.bufs[ba]), m.bufs[bb])   # noqa: E731
        if name == "vdot":
            fn = lambda: ws.vdot(ba, bb)   # noqa: E731
        else:
            def fn():
                ws.vdot_launch(ba, bb)
                return ws.vdot_fetch()
        if BUF_Z in (ba, bb):
            z_read(fn, f"{name}({NAMES[ba]}, {NAMES[bb]})", exp)
        else:
            reads.append((f"{name}({NAMES[ba]}, {NAMES[bb]})", fn(), exp()))
    elif name == "results":
        kind = a["kind"]
        if kind == "async":
            ws.results_async()
            hs, g = ws.results_fetch(small=m.small is not None)
            if m.small is not None:
                reads.append(("results.small", hs, m.small))
            reads.append(("results.grads", g, m.grads))
        elif kind == "gather_fetch" and m.small is not None:
            reads.append(("gather_fetch", ws.gather_fetch(), m.small))
        else:
            reads.append(("get_grads", ws.get_grads(), m.grads))
    elif name == "ws2_launch":
        ws2.objective_launch(BUF_X)
        model2.evaluation_writes_z()
        model2.sweep(BUF_X, None, True)
    elif name == "copy_in":   # ws.dst[dst_lane] <- ws2.src[src_lane]
        dst, src, dl, sl = a["dst"], a["src"], a["dst_lane"], a["src_lane"]
        val = model2.bufs[src][sl]
        if src == BUF_Z and model2.z_refusable():
            try:
                ws.copy_lane_from(ws2, src, sl, dst, dl)
            except RuntimeError as e:
                assert Z_REFUSED.search(str(e)), f"copy_lane from a partial Z: unexpected error {e}"
                return reads
            model2.z_stale = model2.z_one_call = False
        elif dst == BUF_Z and m.z_refusable() and m.B > 1:
            try:
                ws.copy_lane_from(ws2, src, sl, dst, dl)
            except RuntimeError as e:
                assert Z_REFUSED.search(str(e)), f"copy_lane into Z: unexpected error {e}"
                return reads
        else:
            ws.copy_lane_from(ws2, src, sl, dst, dl)
        m.write(dst, [val], lanes=[dl])
    elif name == "copy_out":   # ws2.Y[dst_lane] <- ws.src[src_lane], then read back from ws2
        src, sl, dl = a["src"], a["src_lane"], a["dst_lane"]
        if src == BUF_Z and m.z_refusable():
            try:
                ws2.copy_lane_from(ws, src, sl, BUF_Y, dl)
            except RuntimeError as e:
                assert Z_REFUSED.search(str(e)), f"copy_lane from Z: unexpected error {e}"
                return reads
            m.z_stale = m.z_one_call = False
        else:
            ws2.copy_lane_from(ws, src, sl, BUF_Y, dl)
        model2.write(BUF_Y, [m.bufs[src][sl]], lanes=[dl])
        reads.append((f"copy_out({NAMES[src]})", ws2.download(BUF_Y, dl), model2.bufs[BUF_Y][dl]))
    else:
        raise ValueError(f"unknown operation {name}")
    return reads


# ------------------------------------------------------------------------------------------------------------------------
# generator
# ------------------------------------------------------------------------------------------------------------------------

class Gen:
    """Seeded sequence generator.  It tracks only what the preconditions need (which buffers are known, gather set, bank),
    so the sequence does not depend on any device result.  Draws are biased toward the pairs where host-side bookkeeping
    decides what work to skip: an evaluation followed by a writer of W / ZW / Z, a replayed one-call evaluation between two
    objective_launch calls, a theta change while Z may be partial."""

    def __init__(self, seed, n, batch, T, num_blocks, tile_bits):
        self.rng = np.random.default_rng(seed)
        self.n, self.B, self.T, self.nb, self.tile = n, batch, T, num_blocks, tile_bits
        self.dim = 1 << n
        self.known = {BUF_Y: True, BUF_Z: False, BUF_X: False, BUF_W: False, BUF_ZW: False, BUF_X2: False}
        self.sparse_lhs = {BUF_X: False, BUF_X2: False}
        self.gather = None
        self.bank_sets = 0
        self.z_one_call = False

    # indices inside the tiles of the gather set, outside them, in a second first-stage tile
    def index(self, where):
        r = self.rng
        lo_mask = (1 << self.tile) - 1
        if where == "in" and self.gather is not None:
            g = int(self.gather[r.integers(len(self.gather))])
            return (g & ~lo_mask) | int(r.integers(0, 1 << self.tile))
        if where == "tile1":
            return (1 << self.tile) | int(r.integers(0, 1 << self.tile))
        return int(r.integers(0, self.dim))

    def state(self, lanes):
        v = self.rng.standard_normal((lanes, self.dim)) + 1j * self.rng.standard_normal((lanes, self.dim))
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def thetas(self):
        return np.pi * (2 * self.rng.random((self.B, self.T)) - 1)

    def block_range(self):
        r = self.rng.random()
        if r < 0.6 or self.nb < 2:
            return None
        lo = int(self.rng.integers(0, self.nb - 1))
        return (lo, int(self.rng.integers(lo + 1, self.nb + 1)))

    def lhs(self):
        c = [b for b in (BUF_X, BUF_X2) if self.known[b]]
        return int(self.rng.choice(c)) if c else None

    def setup(self):
        """The opening: target, lhs states, gather set, thetas."""
        ops = [("upload", {"buf": BUF_Y, "data": self.state(self.B)})]
        base = [self.index("any") & ~((1 << self.tile) - 1) for _ in range(1)][0]
        flips = [base] + [base ^ (1 << q) for q in range(self.tile, self.n)][:3]
        ops.append(self._gather_setup(flips))
        ops.append(self._set_basis(BUF_X, [self.index("in") for _ in range(self.B)]))
        ops.append(self._set_basis(BUF_X2, [self.index("any") for _ in range(self.B)]))
        ops.append(("set_thetas", {"th": self.thetas()}))
        return ops

    def _gather_setup(self, idx):
        self.gather = np.array(idx, np.int64)
        return ("gather_setup", {"idx": [int(i) for i in idx]})

    def _set_basis(self, buf, idx):
        self.known[buf] = True
        self.sparse_lhs[buf] = True
        return ("set_basis", {"buf": buf, "idx": [int(i) for i in idx]})

    def _eval_z(self):
        self.known[BUF_Z] = True
        self.known[BUF_W] = self.known[BUF_ZW] = False
        self.z_one_call = True

    def draw(self):
        """One operation (or a short dangerous pair) whose preconditions hold."""
        r, B = self.rng, self.B
        kinds = ["objective_launch", "eval", "surrogate", "theta", "writer", "lhs", "apply", "grad", "read", "read", "refused",
                 "gather_setup", "copy", "pair_replay", "pair_eval_writer", "pair_theta_partial"]
        k = kinds[int(r.integers(len(kinds)))]
        x = self.lhs()
        if k == "objective_launch" and x is not None:
            self._eval_z()
            return [("objective_launch", {"x": x, "br": self.block_range(), "front": bool(r.random() < 0.7)}),
                    ("results", {"kind": ["async", "gather_fetch", "get_grads"][int(r.integers(3))]})]
        if k == "eval" and x is not None:
            vdag = bool(r.random() < 0.7) or not self.known[BUF_Z]
            th = self.thetas() if r.random() < 0.6 else None
            grad = bool(r.random() < 0.8)
            if vdag:
                self._eval_z()
            if grad:
                self.known[BUF_W] = self.known[BUF_ZW] = False
            return [("eval", {"th": th, "vdag": vdag, "gather": bool(r.random() < 0.6), "grad": grad, "x": x,
                              "br": self.block_range(), "front": bool(r.random() < 0.7)})]
        if k == "surrogate":
            return [self.surrogate()]
        if k == "theta":
            if r.random() < 0.5 or self.bank_sets == 0:
                if r.random() < 0.5:
                    return [("set_thetas", {"th": self.thetas()})]
                self.bank_sets = int(r.integers(2, 4))
                return [("theta_bank", {"bank": np.stack([self.thetas() for _ in range(self.bank_sets)])}),
                        ("use_theta_set", {"i": int(r.integers(self.bank_sets))})]
            return [("use_theta_set", {"i": int(r.integers(self.bank_sets))})]
        if k == "writer":
            return [self.writer()]
        if k == "lhs":
            buf = [BUF_X, BUF_X2][int(r.integers(2))]
            where = ["in", "any", "tile1"][int(r.integers(3))]
            if r.random() < 0.5:
                return [self._set_basis(buf, [self.index(where) for _ in range(B)])]
            self.known[buf] = True
            self.sparse_lhs[buf] = True
            idx = [[self.index(where), self.index("in") if r.random() < 0.6 else -1] for _ in range(B)]
            idx = [[i, j if j != i else -1] for i, j in idx]
            coef = r.standard_normal((B, 2)) + 1j * r.standard_normal((B, 2))
            return [("set_combo", {"buf": buf, "idx": idx, "coef": coef})]
        if k == "apply":
            return [self.apply_op()] if self.apply_op_ok() else []
        if k == "grad" and x is not None and self.known[BUF_Z]:
            self.known[BUF_W] = self.known[BUF_ZW] = False
            return [("grad", {"x": x, "br": self.block_range(), "front": bool(r.random() < 0.7)})]
        if k == "read":
            return [self.read()]
        if k == "refused":
            return [self.refused()]
        if k == "gather_setup":
            cnt = int(r.integers(1, 7))
            return [self._gather_setup(sorted({self.index(["in", "any", "tile1"][int(r.integers(3))]) for _ in range(cnt)}))]
        if k == "copy":
            return self.copy()
        if k == "pair_replay" and self.known[BUF_X]:
            x = BUF_X
            # objective_launch, a replayed one-call evaluation (the graph is captured on its first use), objective_launch
            self._eval_z()
            other = self.surrogate() if r.random() < 0.5 else ("eval", {"th": self.thetas(), "vdag": True, "gather": True,
                                                                        "grad": True, "x": BUF_X2 if self.known[BUF_X2] else x,
                                                                        "br": None, "front": True})
            self._eval_z()
            return [("objective_launch", {"x": x, "br": None, "front": True}), ("results", {"kind": "async"}), other,
                    ("objective_launch", {"x": x, "br": None, "front": True}), ("results", {"kind": "get_grads"})]
        if k == "pair_eval_writer" and x is not None:
            self._eval_z()
            ops = [("objective_launch", {"x": x, "br": None, "front": True})]
            w = self.writer(prefer_z_side=True)
            return ops + [w, ("download", {"buf": BUF_Z, "lane": None})]
        if k == "pair_theta_partial" and x is not None:
            self._eval_z()
            ops = [("objective_launch", {"x": x, "br": None, "front": True}), ("set_thetas", {"th": self.thetas()})]
            return ops + [self.writer(prefer_z_side=True), self.read(prefer_z=True)]
        return []

    def surrogate(self):
        r, B = self.rng, self.B
        S = len(self.gather)
        self._eval_z()
        self.known[BUF_X2] = False
        self.sparse_lhs[BUF_X2] = False
        real_only = bool(r.random() < 0.3)
        return ("surrogate_eval", {"th": self.thetas(), "update": int(r.integers(3)), "real_only": real_only,
                                   "weight": r.random(B), "max_no": r.integers(0, S, size=B).astype(np.int64),
                                   "br": self.block_range(), "front": bool(r.random() < 0.7)})

    def writer(self, prefer_z_side=False):
        r, B = self.rng, self.B
        bufs = [BUF_W, BUF_ZW, BUF_Z] if prefer_z_side else [BUF_Y, BUF_X, BUF_X2, BUF_W, BUF_ZW, BUF_Z]
        buf = int(r.choice(bufs))
        how = int(r.integers(3))
        if prefer_z_side and buf != BUF_Z and self.known[BUF_X] and r.random() < 0.5:   # V x into ZW / W: the stages overwrite it
            self.known[buf] = True
            return ("apply", {"inverse": False, "src": BUF_X, "dst": buf})
        if how == 0:
            self.known[buf] = True
            self._data_written(buf)
            return ("upload", {"buf": buf, "data": self.state(B)})
        if how == 1:
            self.known[buf] = True
            self._data_written(buf)
            return ("broadcast", {"buf": buf, "data": self.state(1)[0]})
        if not self.known[buf] and B > 1:   # a lane of a buffer that is not known leaves it unknown
            self.known[buf] = False
        self._data_written(buf, lane=True)
        return ("upload_lane", {"buf": buf, "lane": int(r.integers(B)), "data": self.state(1)[0]})

    def _data_written(self, buf, lane=False):
        if buf in self.sparse_lhs:
            self.sparse_lhs[buf] = False
        if buf == BUF_Z:
            self.z_one_call = False
        if lane and self.B == 1:
            self.known[buf] = True

    def apply_op_ok(self):
        return any(self.known[b] for b in (BUF_Y, BUF_X, BUF_X2, BUF_ZW, BUF_Z))

    def apply_op(self):
        r = self.rng
        srcs = [b for b in (BUF_Y, BUF_X, BUF_X2, BUF_ZW, BUF_Z, BUF_W) if self.known[b]]
        src = int(r.choice(srcs))
        dst = int(r.choice([b for b in (BUF_X, BUF_X2, BUF_W, BUF_ZW, BUF_Z) if b != src]))
        inv = bool(r.random() < 0.5)
        self.known[dst] = True
        self._data_written(dst)
        if dst == BUF_Z and inv:
            self.known[BUF_ZW] = False
        return ("apply", {"inverse": inv, "src": src, "dst": dst})

    def read(self, prefer_z=False):
        r, B = self.rng, self.B
        known = [b for b, k in self.known.items() if k]
        buf = BUF_Z if prefer_z and self.known[BUF_Z] else int(r.choice(known))
        k = int(r.integers(5))
        if k == 0:
            return ("download", {"buf": buf, "lane": None if r.random() < 0.5 else int(r.integers(B))})
        if k == 1:
            return ("gather", {"buf": buf, "idx": [self.index(["in", "any", "tile1"][int(r.integers(3))]) for _ in range(3)]})
        if k == 2 and self.gather is not None:
            return ("gather_launch", {"buf": buf})
        other = int(r.choice(known))
        return ("vdot" if k == 3 else "vdot_launch", {"a": buf, "b": other})

    def refused(self):
        r, B = self.rng, self.B
        bad_br = (self.nb, self.nb + 1) if self.nb > 0 else (0, 0)
        x = self.lhs() or BUF_X
        k = int(r.integers(7))
        if k == 0:
            return ("objective_launch", {"x": x, "br": bad_br, "front": True, "bad": True, "why": "block_range"})
        if k == 1:
            return ("grad", {"x": x, "br": bad_br, "front": True, "bad": True, "why": "block_range"})
        if k == 2:
            return ("eval", {"th": self.thetas(), "vdag": True, "gather": False, "grad": True, "x": x, "br": bad_br,
                             "front": True, "bad": True, "why": "block_range"})
        if k == 3:
            return ("surrogate_eval", {"th": self.thetas(), "update": 1, "real_only": False, "weight": np.full(B, 0.5),
                                       "max_no": np.full(B, len(self.gather), np.int64), "br": None, "front": True,
                                       "bad": True, "why": "max_no"})
        if k == 4:
            return ("set_basis", {"buf": x, "idx": [self.dim] * B})
        if k == 5:
            return ("upload_lane", {"buf": BUF_X, "lane": B, "data": self.state(1)[0]})
        return ("use_theta_set", {"i": max(self.bank_sets, 1) + 2}) if self.bank_sets else \
            ("gather_setup", {"idx": [0, self.dim]})

    def copy(self):
        r, B = self.rng, self.B
        if r.random() < 0.3:
            return [("ws2_launch", {})]
        if r.random() < 0.5:
            dst = int(r.choice([BUF_Y, BUF_X, BUF_Z, BUF_ZW]))
            if dst in (BUF_X, BUF_Z, BUF_ZW) and not self.known[dst] and B > 1:
                return []
            self._data_written(dst, lane=True)
            return [("copy_in", {"dst": dst, "src": int(r.choice([BUF_Y, BUF_Z])), "dst_lane": int(r.integers(B)),
                                 "src_lane": int(r.integers(B))})]
        src = int(r.choice([b for b in (BUF_Y, BUF_Z, BUF_X) if self.known[b]]))
        return [("copy_out", {"src": src, "src_lane": int(r.integers(B)), "dst_lane": int(r.integers(B))})]

    def sequence(self, length):
        ops = self.setup()
        while len(ops) < length:
            ops += self.draw()
        return ops


def checked_preconditions(ops, batch, n):
    """The generator's side of the contract, replayed on flags: every read names a known buffer, every sweep a known lhs
    state and a known Z (what the self-test asserts)."""
    dim = 1 << n
    known = {b: False for b in NAMES}
    gather = False
    for name, a in ops:
        bad = a.get("bad", False)
        if name in ("upload", "broadcast"):
            known[a["buf"]] = True
        elif name in ("upload_lane", "copy_in"):
            lane = a.get("lane", a.get("dst_lane"))
            buf = a.get("buf", a.get("dst"))
            if 0 <= lane < batch:
                known[buf] = known[buf] or batch == 1
        elif name == "set_basis":
            if all(0 <= i < dim for i in a["idx"]):
                known[a["buf"]] = True
        elif name == "set_combo":
            known[a["buf"]] = True
        elif name == "gather_setup":
            gather = gather or all(0 <= i < dim for i in a["idx"])
        elif name == "apply":
            assert known[a["src"]], f"apply from an unknown {NAMES[a['src']]}"
            known[a["dst"]] = True
            if a["dst"] == BUF_Z and a["inverse"]:
                known[BUF_ZW] = False
        elif name in ("objective_launch", "eval", "grad", "surrogate_eval") and not bad:
            if name != "surrogate_eval":
                assert known[a["x"]], f"{name} from an unknown lhs {NAMES[a['x']]}"
            if name == "grad" or (name == "eval" and not a["vdag"]):
                assert known[BUF_Z], f"{name} reads an unknown Z"
            if name == "surrogate_eval":
                assert gather, "surrogate_eval without a gather set"
                known[BUF_X2] = False
            if name in ("objective_launch", "surrogate_eval") or (name == "eval" and a["vdag"]):
                known[BUF_Z] = True
                known[BUF_W] = known[BUF_ZW] = False
            if name == "grad" or (name == "eval" and a["grad"]):
                known[BUF_W] = known[BUF_ZW] = False
        elif name in ("download", "gather", "gather_launch"):
            assert known[a["buf"]], f"{name} of an unknown {NAMES[a['buf']]}"
        elif name in ("vdot", "vdot_launch"):
            assert known[a["a"]] and known[a["b"]], f"{name} of an unknown buffer"
        elif name == "copy_out":
            assert known[a["src"]], f"copy_out of an unknown {NAMES[a['src']]}"
    return True


# ------------------------------------------------------------------------------------------------------------------------
# runner
# ------------------------------------------------------------------------------------------------------------------------

def maxdiff(a, b) -> float:
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"shape {a.shape} != {b.shape}"
    return float(np.max(np.abs(a - b))) if a.size else 0.0


class VectorKit:
    """What the runner needs to know about one kind of workspace: the pair of models, the state the second workspace (the other
    end of copy_lane) starts from, and the operation catalogue.  This one: state-vector workspaces (tests/ws_model_mat.py has the
    matrix one)."""

    @staticmethod
    def models(orc, batch, circ):
        return Model(orc, batch, circ.num_qubits), Model(orc, batch, circ.num_qubits)

    @staticmethod
    def prepare_second(ws2, model2, batch, circ):
        n = circ.num_qubits
        rng2 = np.random.default_rng(12345)
        y2 = rng2.standard_normal((batch, 1 << n)) + 1j * rng2.standard_normal((batch, 1 << n))
        y2 /= np.linalg.norm(y2, axis=1, keepdims=True)
        th2 = np.pi * (2 * rng2.random((batch, circ.num_thetas)) - 1)
        ws2.upload(BUF_Y, y2); model2.write(BUF_Y, y2)
        ws2.set_basis(BUF_X, [3] * batch)
        x2 = np.zeros((batch, 1 << n), complex); x2[:, 3] = 1; model2.write(BUF_X, x2)
        ws2.gather_setup([3, 5]); model2.gather = np.array([3, 5])
        ws2.set_thetas(th2); model2.new_thetas(th2)
        ws2.objective_launch(BUF_X); model2.evaluation_writes_z(); model2.sweep(BUF_X, None, True)

    apply_op = staticmethod(apply_op)


def run_sequence(make_ws, circ, batch, ops, orc=None, tol=TOL, kit=VectorKit, residuals=False):
    """Play `ops` on a workspace from make_ws() (and a second one on the same context for copy_lane), compare every read
    with the model.  A read is (label, got, expected) or (label, got, expected, its own tolerance) -- the outputs of a long-running
    call against its reference.  Where the model names the buffers an operation rewrote (`model.rewritten`) and the workspace
    counts generations, every one of them must have moved.  Returns the list of (step, label, got) of every read, for
    comparisons across configurations; with `residuals`, (step, label, got - expected) of the reads held to `tol` -- what is left
    to compare where the expected values themselves depend on the configuration (an optimiser's returned point does, in its last
    digits times whatever the optimiser amplifies them by)."""
    orc = orc or Oracle(circ)
    ws, ws2 = make_ws(), make_ws()
    model, model2 = kit.models(orc, batch, circ)
    out = []
    try:
        kit.prepare_second(ws2, model2, batch, circ)
        for step, op in enumerate(ops):
            gens = {b: ws.generation(b) for b in NAMES} if hasattr(ws, "generation") else None
            if hasattr(model, "rewritten"):
                model.rewritten = set()
            try:
                reads = kit.apply_op(ws, model, op, ws2, model2)
            except AssertionError:
                raise
            except Exception as e:
                raise AssertionError(f"step {step} {op[0]}: {type(e).__name__}: {e}\n{describe(ops, step)}") from e
            for label, got, exp, *own in reads:
                d = maxdiff(got, exp)
                bound = own[0] if own else tol
                assert d < bound, (f"step {step} {op[0]} -> {label}: differs from the model by {d:.3g} (bound {bound:g})\n"
                                   f"{describe(ops, step)}")
                if not residuals:
                    out.append((step, label, np.array(got)))
                elif not own:
                    out.append((step, label, np.asarray(got) - np.asarray(exp)))
            if gens is not None:
                for b in getattr(model, "rewritten", ()):
                    assert ws.generation(b) != gens[b], (f"step {step} {op[0]}: rewrote {NAMES[b]} and left its generation() at {gens[b]}\n"
                                                         f"{describe(ops, step)}")
    finally:
        ws.close()
        ws2.close()
    return out


def describe(ops, upto):
    lines = []
    for i, (name, a) in enumerate(ops[: upto + 1]):
        short = {k: (NAMES.get(v, v) if k in ("buf", "x", "src", "dst", "a", "b") and isinstance(v, int) else v)
                 for k, v in a.items() if not isinstance(v, np.ndarray) and k not in ("data", "coef")}
        lines.append(f"  {i:3d} {name} {short}")
    return "sequence:\n" + "\n".join(lines)


# ------------------------------------------------------------------------------------------------------------------------
# FakeWorkspace: engine.Workspace's method surface, computed by the oracle (CPU self-test of the runner)
# ------------------------------------------------------------------------------------------------------------------------

class FakeWorkspace:
    """What a correct workspace returns, computed with the oracle; Z is always whole (a correct implementation may do that)."""

    def __init__(self, circ, batch, orc=None):
        self.circ, self.batch, self.T, self.nb = circ, batch, circ.num_thetas, circ.num_blocks
        self.dim = 1 << circ.num_qubits
        self.orc = orc or Oracle(circ)
        self.b = {k: np.zeros((batch, self.dim), complex) for k in NAMES}
        self.th = np.zeros((batch, self.T))
        self.bank = None
        self.gidx = None
        self.small = None
        self.vd = None
        self.g = np.zeros((batch, self.T), complex)
        self.closed = False

    def _br(self, br):
        if br is not None and not (0 <= br[0] < br[1] <= self.nb):
            raise RuntimeError(f"aqc_hip: invalid block_range [{br[0]}, {br[1]})")

    def set_thetas(self, th):
        self.th = np.array(th, float).reshape(self.batch, self.T)

    def theta_bank(self, bank):
        self.bank = np.array(bank, float).reshape(-1, self.batch, self.T)
        return self.bank.shape[0]

    def use_theta_set(self, i):
        if not 0 <= i < self.bank.shape[0]:
            raise RuntimeError("aqc_hip: theta set out of range")
        self.th = self.bank[i].copy()

    def upload(self, buf, data, lane=None):
        if lane is None:
            self.b[buf] = np.array(data, complex).reshape(self.batch, self.dim)
        else:
            if not 0 <= lane < self.batch:
                raise RuntimeError("aqc_hip: lane out of range")
            self.b[buf][lane] = data

    def broadcast(self, buf, data):
        self.b[buf] = np.tile(np.asarray(data, complex), (self.batch, 1))

    def download(self, buf, lane=None):
        return self.b[buf].copy() if lane is None else self.b[buf][lane].copy()

    def copy_lane_from(self, src, src_buf, src_lane, dst_buf, dst_lane):
        self.b[dst_buf][dst_lane] = src.b[src_buf][src_lane]

    def set_basis(self, buf, idx):
        idx = np.broadcast_to(np.asarray(idx, np.int64), (self.batch,))
        if np.any(idx < 0) or np.any(idx >= self.dim):
            raise RuntimeError("aqc_hip: basis index out of range")
        x = np.zeros((self.batch, self.dim), complex)
        x[np.arange(self.batch), idx] = 1
        self.b[buf] = x

    def set_combo(self, buf, idx, coef):
        x = np.zeros((self.batch, self.dim), complex)
        for b in range(self.batch):
            x[b, idx[b][0]] += coef[b][0]
            if idx[b][1] >= 0:
                x[b, idx[b][1]] += coef[b][1]
        self.b[buf] = x

    def gather_setup(self, idx):
        idx = np.asarray(idx, np.int64)
        if np.any(idx < 0) or np.any(idx >= self.dim):
            raise RuntimeError("aqc_hip: gather index out of range")
        self.gidx = idx

    def apply(self, inverse, src, dst):
        f = self.orc.vdag if inverse else self.orc.v
        self.b[dst] = np.stack([f(self.th[b], self.b[src][b]) for b in range(self.batch)])
        if inverse and dst == BUF_Z:
            self.b[BUF_ZW][:] = np.nan   # the checkpoint: not data

    def grad_from(self, x, br=None, front=True):
        self._br(br)
        self.g = np.stack([self.orc.grad(self.th[b], self.b[x][b], self.b[BUF_Z][b], br, front) for b in range(self.batch)])
        self.b[BUF_W][:] = np.nan
        self.b[BUF_ZW][:] = np.nan

    def objective_launch(self, x, br=None, front=True):
        self._br(br)
        self.apply(True, BUF_Y, BUF_Z)
        if self.gidx is not None:
            self.small = self.b[BUF_Z][:, self.gidx]
        self.grad_from(x, br, front)

    def eval(self, thetas=None, vdag=True, gather=False, grad=True, x_buf=BUF_X, block_range=None, front_layer=True):
        if grad:
            self._br(block_range)
        if thetas is not None:
            self.set_thetas(thetas)
        if vdag:
            self.apply(True, BUF_Y, BUF_Z)
        hs = g = None
        if gather:
            self.small = hs = self.b[BUF_Z][:, self.gidx]
        if grad:
            self.grad_from(x_buf, block_range, front_layer)
            g = self.g.copy()
        return hs, g

    def surrogate_eval(self, thetas, weight, max_no, update_state=True, block_range=None, front_layer=True, real_only=False):
        self._br(block_range)
        if np.any(max_no < 0) or np.any(max_no >= len(self.gidx)):
            raise RuntimeError("aqc_hip: leading state out of range")
        self.set_thetas(thetas)
        self.apply(True, BUF_Y, BUF_Z)
        res = [surrogate_lane(self.orc, self.th[b], self.b[BUF_Y][b], self.gidx, weight[b], max_no[b], int(update_state),
                              block_range, front_layer) for b in range(self.batch)]
        self.g = np.stack([r[3] for r in res])
        self.small = np.stack([r[2] for r in res])
        self.b[BUF_X2] = np.stack([r[6] for r in res])
        self.b[BUF_W][:] = np.nan
        self.b[BUF_ZW][:] = np.nan
        if update_state:
            weight[:] = [r[4] for r in res]
            max_no[:] = [r[5] for r in res]
        f = np.array([r[0] for r in res])
        fid = np.array([r[1] for r in res]) if update_state else None
        return f, fid, self.small.copy(), (self.g.real.copy() if real_only else self.g.copy())

    def get_grads(self):
        return self.g.copy()

    def gather(self, buf, idx):
        return self.b[buf][:, np.asarray(idx, np.int64)]

    def gather_launch(self, buf):
        self.small = self.b[buf][:, self.gidx]

    def gather_fetch(self):
        return self.small.copy()

    def vdot(self, a, b):
        return np.einsum("bi,bi->b", np.conj(self.b[a]), self.b[b])

    def vdot_launch(self, a, b):
        self.vd = self.vdot(a, b)

    def vdot_fetch(self):
        return self.vd.copy()

    def results_async(self):
        self._res = (None if self.small is None else self.small.copy(), self.g.copy())

    def results_fetch(self, small=True, grads=True):
        return (self._res[0] if small else None), (self._res[1] if grads else None)

    def close(self):
        self.closed = True
