"""
Thin object layer over the C ABI: ``HipContext`` (one per ansatz structure) and
``Workspace`` (device-resident batch of evaluations).  No arithmetic happens
here -- every number comes from the HIP kernels.
"""
import ctypes
from ctypes import byref, c_double, c_float, c_int, c_int32, c_int64, c_void_p
from typing import Optional, Tuple

import numpy as np

from . import _lib
from ._lib import BUF_W, BUF_X, BUF_X2, BUF_Y, BUF_Z, BUF_ZW, K_APPLY, K_COEF, K_FINALIZE, K_MISC, K_SWEEP, check, dptr  # noqa: F401


def default_device() -> int:
    """Device of the function-level drop-ins: ``AQC_DEVICE`` if set, else this process's ``LOCAL_RANK`` (one process
    per GPU under torch.distributed.run / job_executor), else 0."""
    import os

    for name in ("AQC_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(name, "")
        if v.strip().isdigit():
            # ranks outnumbering the visible GPUs (CPU rehearsals with gloo) share devices round-robin
            return int(v) % max(1, _lib.lib().aqc_device_count()) if name == "LOCAL_RANK" else int(v)
    return 0


def live_buffers() -> tuple:
    """(device, pinned) allocations the library's handles hold right now (aqc_live_buffers): equal before and after a handle's life."""
    dev, pin = c_int64(0), c_int64(0)
    check(_lib.lib().aqc_live_buffers(byref(dev), byref(pin)))
    return dev.value, pin.value


def _structure_key(circ) -> tuple:
    trotter = hasattr(circ, "is_second_order")
    blocks = np.ascontiguousarray(circ.blocks, dtype=np.int32)
    return (int(circ.num_qubits), str(circ.entangler), blocks.shape[1], blocks.tobytes(), trotter,
            bool(circ.is_second_order) if trotter else False)


class HipContext:
    """Immutable gate program of one ansatz (aqc_create / aqc_destroy)."""

    _cache = {}

    def __init__(self, circ):
        L = _lib.lib()
        n, ent, nb, _, trotter, second = key = _structure_key(circ)
        if ent not in _lib.ENTANGLERS:
            raise ValueError(f"unknown entangler {ent!r}")
        blocks = np.ascontiguousarray(circ.blocks, dtype=np.int32)
        handle = c_void_p()
        status = L.aqc_create(n, _lib.ENTANGLERS[ent], blocks.ctypes.data_as(ctypes.POINTER(c_int32)), nb,
                              int(trotter), int(second), byref(handle))
        if status != 0:
            raise ValueError("aqc_hip: " + L.aqc_last_error().decode())
        self.handle = handle
        self.key = key
        self.num_qubits, self.entangler, self.num_blocks = n, ent, nb
        self.trotter, self.second_order = trotter, second
        self.num_thetas = L.aqc_num_thetas(handle)
        self.num_gate_groups = L.aqc_num_gate_groups(handle)
        self._ws = {}

    @classmethod
    def of(cls, circ) -> "HipContext":
        """Context for the circuit's *current* structure (circuits are mutable:
        update_structure / insert_unit_blocks)."""
        key = _structure_key(circ)
        ctx = cls._cache.get(key)
        if ctx is None:
            if len(cls._cache) >= 64:
                cls._cache.pop(next(iter(cls._cache)))
            ctx = cls._cache[key] = cls(circ)
        return ctx

    def workspace(self, batch: int = 1, ncols: int = 1, device: Optional[int] = None, **kw) -> "Workspace":
        """Cached workspace for the given shape (function-level drop-ins reuse it)."""
        if device is None:
            device = default_device()
        key = (batch, ncols, device, tuple(sorted(kw.items())))
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = Workspace(self, batch=batch, ncols=ncols, device=device, **kw)
        return ws

    def plan_projected(self, tile_bits: int = 0, low_bits: int = -1) -> dict:
        """Host-only: the projected route (Workspace.projected_info) a state-vector workspace of this tiling would take, or {}."""
        c = (ctypes.c_int32 * 16)()
        check(_lib.lib().aqc_plan_projected(self.handle, tile_bits, low_bits, c))
        if not c[0]:
            return {}
        return {"virtual_qubits": int(c[1]), "touched_qubits": int(c[2]), "shared_with_first_stage": int(c[3]), "stages": int(c[4]),
                "substages": int(c[5]), "tile_bits": int(c[6]), "substages_on_the_register": int(c[7]), "summed_bits": int(c[8]),
                "padded_qubits": int(c[9]), "substages_per_stage": [int(c[10 + i]) for i in range(min(int(c[4]), 6))]}

    def plan(self, which: int = 1, ncols: int = 1, tile_bits: int = 0, low_bits: int = -1):
        """Host-only planner introspection: list of (local_bits, gate_group_indices)."""
        L = _lib.lib()
        ns = c_int()
        check(L.aqc_plan_query(self.handle, ncols, which, tile_bits, low_bits, -1, byref(ns), None, None, None, None))
        out = []
        bits = (c_int * 64)()
        ops = (c_int * max(1, self.num_gate_groups))()
        for s in range(ns.value):
            nb, no = c_int(), c_int()
            check(L.aqc_plan_query(self.handle, ncols, which, tile_bits, low_bits, s, byref(ns), bits, byref(nb), ops, byref(no)))
            out.append((list(bits[: nb.value]), list(ops[: no.value])))
        return out

    def __del__(self):
        try:
            for ws in self._ws.values():
                ws.close()
            if self.handle:
                _lib.lib().aqc_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class Workspace:
    """``batch`` independent evaluations resident in HBM (aqc_ws_*)."""

    def __init__(self, ctx: HipContext, batch: int = 1, ncols: int = 1, device: Optional[int] = None,
                 tile_bits_apply: int = 0, tile_bits_sweep: int = 0):
        device = default_device() if device is None else int(device)   # one process per GPU: LOCAL_RANK's device
        self.ctx, self.batch, self.ncols, self.device = ctx, int(batch), int(ncols), device
        self.dim = 1 << ctx.num_qubits
        self.T = ctx.num_thetas
        self._L = _lib.lib()
        handle = c_void_p()
        check(self._L.aqc_ws_create(ctx.handle, device, batch, ncols, tile_bits_apply, tile_bits_sweep, byref(handle)))
        self.handle = handle
        self._gather_count = 0
        self._gen = [0] * 6   # per buffer: bumped by every call that (re)writes it

    def _touch(self, *bufs) -> None:
        for b in bufs:
            self._gen[b] += 1

    def generation(self, buf: int) -> int:
        """Changes whenever `buf` is written through this object: lets a caller that left a result there find out later
        whether it is still the one (mps_operations.DenseBackedMPS)."""
        return self._gen[buf]

    # -- data movement -------------------------------------------------------
    def _shape(self):
        return (self.batch, self.dim) if self.ncols == 1 else (self.batch, self.dim, self.ncols)

    def set_thetas(self, thetas) -> None:
        th = _lib.as_f64(thetas, self.batch * self.T, "thetas")
        check(self._L.aqc_ws_set_thetas(self.handle, dptr(th)))

    def upload(self, buf: int, data, lane: Optional[int] = None) -> None:
        self._touch(buf)
        if lane is None:
            a = _lib.as_c128(data)
            if a.size != self.batch * self.dim * self.ncols:
                raise ValueError(f"expected {self._shape()} complex values, got shape {a.shape}")
            check(self._L.aqc_ws_upload(self.handle, buf, dptr(a)))
        else:
            a = _lib.as_c128(data)
            if a.size != self.dim * self.ncols:
                raise ValueError("lane data has the wrong size")
            check(self._L.aqc_ws_upload_lane(self.handle, buf, lane, dptr(a)))

    def broadcast(self, buf: int, data) -> None:
        self._touch(buf)
        a = _lib.as_c128(data)
        if a.size != self.dim * self.ncols:
            raise ValueError("broadcast data has the wrong size")
        check(self._L.aqc_ws_broadcast(self.handle, buf, dptr(a)))

    def download(self, buf: int, lane: Optional[int] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        if out is not None:   # the pointer goes straight to a D2H copy: refuse anything that is not the exact layout
            want = self._shape() if lane is None else self._shape()[1:]
            if not (isinstance(out, np.ndarray) and out.dtype == np.complex128 and out.flags.c_contiguous
                    and out.flags.writeable and out.size == int(np.prod(want))):
                raise ValueError(f"out must be a writable C-contiguous complex128 array of {int(np.prod(want))} elements")
        if lane is None:
            res = np.empty(self._shape(), dtype=np.complex128) if out is None else out
            check(self._L.aqc_ws_download(self.handle, buf, dptr(res)))
        else:
            res = np.empty(self._shape()[1:], dtype=np.complex128) if out is None else out
            check(self._L.aqc_ws_download_lane(self.handle, buf, lane, dptr(res)))
        return res

    def copy_lane_from(self, src: "Workspace", src_buf: int, src_lane: int, dst_buf: int, dst_lane: int) -> None:
        """this.dst_buf[dst_lane] <- src.src_buf[src_lane], device to device (targets that are already resident)."""
        self._touch(dst_buf)
        check(self._L.aqc_ws_copy_lane(self.handle, dst_buf, dst_lane, src.handle, src_buf, src_lane))

    def set_basis(self, buf: int, index) -> None:
        self._touch(buf)
        idx = np.ascontiguousarray(np.broadcast_to(np.asarray(index, dtype=np.int64), (self.batch,)))
        check(self._L.aqc_ws_set_basis(self.handle, buf, idx.ctypes.data_as(ctypes.POINTER(c_int64))))

    def set_combo(self, buf: int, index, coef) -> None:
        """buffer[lane] = coef[lane][0] |index[lane][0]> + coef[lane][1] |index[lane][1]>  (index[lane][1] < 0: one term)."""
        self._touch(buf)
        idx = np.ascontiguousarray(np.asarray(index, dtype=np.int64).reshape(self.batch, 2))
        cf = np.ascontiguousarray(np.asarray(coef, dtype=np.complex128).reshape(self.batch, 2))
        check(self._L.aqc_ws_set_combo(self.handle, buf, idx.ctypes.data_as(ctypes.POINTER(c_int64)), dptr(cf)))

    def set_identity(self, buf: int) -> None:
        self._touch(buf)
        check(self._L.aqc_ws_set_identity(self.handle, buf))

    # -- compute -------------------------------------------------------------
    def apply(self, inverse: bool, src: int = BUF_Y, dst: int = BUF_Z) -> None:
        self._touch(dst, *([BUF_ZW] if inverse and dst == BUF_Z else []))   # (V^H into Z leaves its checkpoint in ZW)
        check(self._L.aqc_ws_apply(self.handle, int(bool(inverse)), src, dst))

    def grad(self, block_range: Optional[Tuple[int, int]] = None, front_layer: bool = True) -> None:
        self._touch(BUF_W, BUF_ZW)
        lo, hi = (-1, -1) if block_range is None else (int(block_range[0]), int(block_range[1]))
        check(self._L.aqc_ws_grad(self.handle, lo, hi, int(bool(front_layer))))

    def eval(self, thetas=None, vdag: bool = True, gather: bool = False, grad: bool = True, x_buf: int = BUF_X,
             block_range: Optional[Tuple[int, int]] = None, front_layer: bool = True):
        """One native call, one host synchronisation: [thetas ->] [Z = V^H Y] [gather from Z] [sweep].
        Returns (gathered or None, grads or None)."""
        self._touch(*(([BUF_Z, BUF_ZW] if vdag else []) + ([BUF_W, BUF_ZW] if grad else [])))
        th = None if thetas is None else _lib.as_f64(thetas, self.batch * self.T, "thetas")
        hs = np.empty((self.batch, self._gather_count), dtype=np.complex128) if gather else None
        g = np.empty((self.batch, self.T), dtype=np.complex128) if grad else None
        lo, hi = (-1, -1) if block_range is None else (int(block_range[0]), int(block_range[1]))
        check(self._L.aqc_ws_eval(self.handle, None if th is None else th.ctypes.data, int(bool(vdag)),
                                  None if hs is None else hs.ctypes.data, x_buf, lo, hi, int(bool(front_layer)),
                                  None if g is None else g.ctypes.data))
        return hs, g

    def surrogate_eval(self, thetas, weight: np.ndarray, max_no: np.ndarray, update_state: bool = True,
                       block_range: Optional[Tuple[int, int]] = None, front_layer: bool = True, real_only: bool = False):
        """One evaluation of the lane-batched surrogate objective in one native call (``aqc_ws_surrogate_eval``): V^H, the
        flip-state amplitudes, the optional state update, the value and ONE sweep from every lane's combined lhs state.
        ``weight`` (float64[batch]) and ``max_no`` (int64[batch]) are the objective state, updated IN PLACE when
        ``update_state`` (True / 1: hysteresis and weight smoothing; 2: hysteresis only, as objective() does on its own).
        Returns (f[batch], fidelity[batch] or None, hs[batch][states], complex grads[batch][T]); with ``real_only`` the last
        item is the real part alone (float64[batch][T]: the surrogate's gradient, half the bytes over the bus)."""
        self._touch(BUF_Z, BUF_W, BUF_ZW, BUF_X2)
        th = _lib.as_f64(thetas, self.batch * self.T, "thetas")
        if not (isinstance(weight, np.ndarray) and weight.dtype == np.float64 and weight.flags.c_contiguous and weight.size == self.batch):
            raise ValueError("weight must be a C-contiguous float64 array of one entry per lane")
        if not (isinstance(max_no, np.ndarray) and max_no.dtype == np.int64 and max_no.flags.c_contiguous and max_no.size == self.batch):
            raise ValueError("max_no must be a C-contiguous int64 array of one entry per lane")
        f = np.empty(self.batch)
        fid = np.empty(self.batch) if update_state else None
        hs = np.empty((self.batch, self._gather_count), dtype=np.complex128)
        g = np.empty((self.batch, self.T), dtype=np.float64 if real_only else np.complex128)
        lo, hi = (-1, -1) if block_range is None else (int(block_range[0]), int(block_range[1]))
        check(self._L.aqc_ws_surrogate_eval(self.handle, dptr(th), int(update_state), dptr(weight),
                                            max_no.ctypes.data_as(ctypes.POINTER(c_int64)), lo, hi, int(bool(front_layer)),
                                            dptr(f), None if fid is None else dptr(fid), dptr(hs),
                                            None if real_only else dptr(g), dptr(g) if real_only else None))
        return f, fid, hs, g

    def grad_from(self, x_buf: int, block_range: Optional[Tuple[int, int]] = None, front_layer: bool = True) -> None:
        self._touch(BUF_W, BUF_ZW)
        lo, hi = (-1, -1) if block_range is None else (int(block_range[0]), int(block_range[1]))
        check(self._L.aqc_ws_grad_from(self.handle, x_buf, lo, hi, int(bool(front_layer))))

    def get_grads(self) -> np.ndarray:
        g = np.empty((self.batch, self.T), dtype=np.complex128)
        check(self._L.aqc_ws_get_grads(self.handle, dptr(g)))
        return g

    def gather(self, buf: int, index) -> np.ndarray:
        idx = np.ascontiguousarray(index, dtype=np.int64).ravel()
        out = np.empty((self.batch, idx.size), dtype=np.complex128)
        check(self._L.aqc_ws_gather(self.handle, buf, idx.ctypes.data_as(ctypes.POINTER(c_int64)), idx.size, dptr(out)))
        return out

    def vdot(self, buf_a: int, buf_b: int) -> np.ndarray:
        out = np.empty(self.batch, dtype=np.complex128)
        check(self._L.aqc_ws_vdot(self.handle, buf_a, buf_b, dptr(out)))
        return out

    # -- asynchronous, HBM-resident variants ------------------------------------
    def theta_bank(self, thetas) -> int:
        th = np.ascontiguousarray(thetas, dtype=np.float64)
        if th.size % (self.batch * self.T):
            raise ValueError("theta bank must have shape (nsets, batch, T)")
        nsets = th.size // (self.batch * self.T)
        check(self._L.aqc_ws_theta_bank(self.handle, dptr(th), nsets))
        return nsets

    def use_theta_set(self, i: int) -> None:
        check(self._L.aqc_ws_use_theta_set(self.handle, int(i)))

    def gather_setup(self, index) -> None:
        idx = np.ascontiguousarray(index, dtype=np.int64).ravel()
        check(self._L.aqc_ws_gather_setup(self.handle, idx.ctypes.data_as(ctypes.POINTER(c_int64)), idx.size))
        self._gather_count = idx.size   # (after the call: a refused set-up keeps the old count, which sizes every fetch)

    def gather_launch(self, buf: int) -> None:
        check(self._L.aqc_ws_gather_launch(self.handle, buf))

    def gather_fetch(self) -> np.ndarray:
        out = np.empty((self.batch, self._gather_count), dtype=np.complex128)
        check(self._L.aqc_ws_gather_fetch(self.handle, dptr(out)))
        return out

    def vdot_launch(self, buf_a: int, buf_b: int) -> None:
        check(self._L.aqc_ws_vdot_launch(self.handle, buf_a, buf_b))

    def vdot_fetch(self) -> np.ndarray:
        out = np.empty(self.batch, dtype=np.complex128)
        check(self._L.aqc_ws_vdot_fetch(self.handle, dptr(out)))
        return out

    def objective_launch(self, x_buf: int = BUF_X, block_range: Optional[Tuple[int, int]] = None, front_layer: bool = True) -> None:
        """Z = V^H Y (where the evaluation reads it), the registered gather, the sweep from ``x_buf``: enqueued, not waited for."""
        self._touch(BUF_Z, BUF_W, BUF_ZW)
        lo, hi = (-1, -1) if block_range is None else (int(block_range[0]), int(block_range[1]))
        check(self._L.aqc_ws_objective_launch(self.handle, x_buf, lo, hi, int(bool(front_layer))))

    def results_async(self) -> None:
        """Enqueue the copies of this evaluation's gradients and gathered amplitudes (or <A|B>) into pinned host memory."""
        check(self._L.aqc_ws_results_async(self.handle))

    def results_fetch(self, small: bool = True, grads: bool = True):
        """Wait for the stream; returns (gathered amplitudes / <A|B> or None, gradients or None) of the last results_async."""
        hs = np.empty((self.batch, max(self._gather_count, 1)), dtype=np.complex128) if small else None
        g = np.empty((self.batch, self.T), dtype=np.complex128) if grads else None
        check(self._L.aqc_ws_results_fetch(self.handle, None if hs is None else dptr(hs), None if g is None else dptr(g)))
        return hs, g

    def sync(self) -> None:
        check(self._L.aqc_ws_sync(self.handle))

    # -- sketched AQC on the device (aqc_ws_sketch_*) ---------------------------
    def sketch_target(self, target, shared: Optional[bool] = None) -> None:
        """The target unitary of every lane, (batch, d, d), or one (d, d) for all lanes, resident in HBM."""
        u = _lib.as_c128(target)
        if shared is None:
            shared = u.ndim == 2
        if u.size != (1 if shared else self.batch) * self.dim * self.dim:
            raise ValueError(f"target of shape {u.shape} does not fit {'one' if shared else self.batch} ({self.dim}, {self.dim}) matrices")
        check(self._L.aqc_ws_sketch_target(self.handle, dptr(u), int(bool(shared))))

    def _alt_idx(self, alt_idx, sets: int):
        if alt_idx is None:
            return None, None
        idx = np.ascontiguousarray(alt_idx, dtype=np.int32)
        if idx.size != sets * self.batch * self.ncols:
            raise ValueError(f"alt_idx needs {sets} x {self.batch} x {self.ncols} column indices, got shape {idx.shape}")
        return idx, idx.ctypes.data_as(ctypes.POINTER(c_int32))

    def sketch_generate(self, kind: str, seed: int = 0, iteration: int = 0, alt_idx=None, omega=None, status: bool = True):
        """X, Y = U X of every lane into BUF_X / BUF_Y on the device, with the thetas in use (``eigen``).  ``omega``: a host
        draw (batch, d, k) instead of the device's Philox draw; ``alt_idx``: (batch, k) columns for ``alt``.  Returns the QR's
        status word per lane (int32[batch]; 0 = fine), or None with ``status=False`` (nothing is waited for then)."""
        self._touch(BUF_X, BUF_Y, BUF_W, BUF_ZW)   # X and Y: the result; W and ZW: unspecified afterwards
        keep, idx = self._alt_idx(alt_idx, 1)
        om = None
        if omega is not None:
            om = _lib.as_c128(omega)
            if om.size != self.batch * self.dim * self.ncols:
                raise ValueError(f"omega must have shape {self._shape()}")
        st = np.zeros(self.batch, dtype=np.int32) if status else None
        check(self._L.aqc_ws_sketch_generate(self.handle, _lib.SKETCH_KINDS[kind], int(seed), int(iteration), idx, None if om is None else dptr(om),
                                             None if st is None else st.ctypes.data_as(ctypes.POINTER(c_int32))))
        del keep
        return st

    def sketch_draw(self, kind: str, seed: int = 0, iteration: int = 0, buf: int = BUF_X) -> None:
        """``buf`` <- the device's draw Omega of every lane for (kind, seed, iteration), nothing else (``rand`` / ``eigen``)."""
        self._touch(buf)
        check(self._L.aqc_ws_sketch_draw(self.handle, _lib.SKETCH_KINDS[kind], int(seed), int(iteration), buf))

    def sketch_adam(self, kind: str, x0, niter: int, lr, *, beta1: float = 0.9, beta2: float = 0.99, eps: float = 1e-8, tol: float = 1e-6,
                    seed: int = 0, iter0: int = 0, reset=None, alt_idx=None) -> dict:
        """``niter`` ADAM iterations of the sketched objective on every lane without leaving the device (aqc_ws_sketch_adam), one
        fetch at the end.  ``lr``: a number or one per lane; ``reset``: None, a number or one per lane (0 continue, 1 restart from
        x0, 2 parked); ``alt_idx``: (niter + 1, batch, k).  Returns x (batch, T), profile (batch, niter + 1), nit (batch,), cost
        (profile[lane][nit[lane]]: the objective at the final point under the next sketch), best_f, best_x, status."""
        self._touch(BUF_X, BUF_Y, BUF_Z, BUF_W, BUF_ZW)
        niter = int(niter)
        keep, idx = self._alt_idx(alt_idx, niter + 1)
        x0a = None if x0 is None else _lib.as_f64(x0, self.batch * self.T, "x0")
        lra = np.ascontiguousarray(np.broadcast_to(np.asarray(lr, dtype=np.float64), (self.batch,)))
        rs = None if reset is None else np.ascontiguousarray(np.broadcast_to(np.asarray(reset, dtype=np.int32), (self.batch,)))
        x = np.empty((self.batch, self.T))
        prof = np.empty((self.batch, niter + 1))
        best_f, best_x = np.empty(self.batch), np.empty((self.batch, self.T))
        nit, st = np.zeros(self.batch, dtype=np.int64), np.zeros(self.batch, dtype=np.int32)
        i32 = ctypes.POINTER(c_int32)
        check(self._L.aqc_ws_sketch_adam(self.handle, _lib.SKETCH_KINDS[kind], None if x0a is None else dptr(x0a), niter, dptr(lra), beta1, beta2,
                                         eps, tol, int(seed), int(iter0), None if rs is None else rs.ctypes.data_as(i32), idx, dptr(x), dptr(prof),
                                         dptr(best_f), dptr(best_x), nit.ctypes.data_as(ctypes.POINTER(c_int64)), st.ctypes.data_as(i32)))
        del keep
        return {"x": x, "profile": prof, "nit": nit, "cost": prof[np.arange(self.batch), nit], "best_f": best_f, "best_x": best_x, "status": st}

    # -- coordinate-descent driver (aqc_ws_cd_minimize) ---------------------------
    def cd_minimize(self, thetas0, maxiter: int, *, chunk: int = 64, dtheta_thr: float = 1e-8, fobj_thr: float = 1e-2,
                    time_limit: float = -1.0, route: str = "auto", max_steps: int = -1) -> dict:
        """Coordinate-descent sweeps of every lane from ``thetas0`` (batch, T) until the lane's stop rule ends it, targets in BUF_Y of
        a square workspace: best-so-far value and thetas, the profile and the exit status are kept on the device and fetched once.
        The host reads one word per ``chunk`` sweeps and checks ``time_limit`` (seconds; <= 0: none) there, so a timeout takes
        effect between chunks, never inside one.  ``route``: "auto", "persistent" (operands in LDS, up to 6 qubits) or "wide".
        Returns thetas (the best ones), cost, nit, status (int32: 1 normal, 2 early, 3 timeout) and profile (batch, maxiter)."""
        self._touch(BUF_X, BUF_Z, BUF_W, BUF_ZW)   # unspecified afterwards on every route (the wide walk's V^H leaves a checkpoint in ZW)
        th = _lib.as_f64(thetas0, self.batch * self.T, "thetas0")
        maxiter = int(maxiter)
        if maxiter < 1:
            raise ValueError("maxiter must be positive")
        best_x, best_f = np.empty((self.batch, self.T)), np.empty(self.batch)
        nit, st = np.zeros(self.batch, dtype=np.int64), np.zeros(self.batch, dtype=np.int32)
        prof = np.zeros((self.batch, maxiter))
        check(self._L.aqc_ws_cd_minimize(self.handle, dptr(th), maxiter, int(chunk), float(dtheta_thr), float(fobj_thr), float(time_limit),
                                         _lib.CD_ROUTES[route], int(max_steps), dptr(best_x), dptr(best_f),
                                         nit.ctypes.data_as(ctypes.POINTER(c_int64)), st.ctypes.data_as(ctypes.POINTER(c_int32)), dptr(prof)))
        return {"thetas": best_x, "cost": best_f, "nit": nit, "status": st, "profile": prof}

    def cd_sweeps(self, thetas, nsweeps: int = 1, max_steps: int = -1):
        """``nsweeps`` coordinate-descent sweeps of every lane in one persistent launch (aqc_ws_cd_sweeps; up to 6 qubits), targets
        in BUF_Y.  Returns (thetas after the last sweep (batch, T) -- the thetas in use afterwards --, fobj (batch, nsweeps))."""
        th = _lib.as_f64(thetas, self.batch * self.T, "thetas").reshape(self.batch, self.T).copy()
        fobj = np.zeros((self.batch, int(nsweeps)))
        self._touch(BUF_X, BUF_Z, BUF_W, BUF_ZW)
        check(self._L.aqc_ws_cd_sweeps(self.handle, dptr(th), dptr(fobj), int(nsweeps), int(max_steps)))
        return th, fobj

    def cd_sweep(self, thetas):
        """One sweep on a one-lane workspace (aqc_ws_cd_sweep: the persistent launch where it fits, else one sweep of the wide walk).
        Returns (thetas after the sweep (T,) -- the thetas in use afterwards --, the objective there)."""
        th = _lib.as_f64(thetas, self.T, "thetas").copy()
        fobj = np.zeros(1)
        self._touch(BUF_X, BUF_Z, BUF_W, BUF_ZW)
        check(self._L.aqc_ws_cd_sweep(self.handle, dptr(th), dptr(fobj)))
        return th, float(fobj[0])

    # -- device-resident L-BFGS on the matrix objective (aqc_ws_lbfgs_mat) ---------
    def lbfgs_mat(self, x0, *, maxiter: int = 100, memory: int = 10, gtol: float = 1e-7, ftol: float = 1e-12, fobj_thr: float = 0.0,
                  fidelity_thr: float = 0.0, max_backtracks: int = 12) -> dict:
        """L-BFGS on f = 1 - Re tr(X^H V^H Y) / ncols of every lane, X and Y as the buffers hold them.  Z, W and ZW are unspecified
        afterwards; the thetas in use are the returned ``x``.  Returns x, fun, fidelity, nit, nfev (of the batch) and status."""
        x = _lib.as_f64(x0, self.batch * self.T, "x0")
        xo = np.empty((self.batch, self.T))
        f, fid = np.empty(self.batch), np.empty(self.batch)
        nit, status, nfev = np.zeros(self.batch, dtype=np.int64), np.zeros(self.batch, dtype=np.int32), c_int64()
        self._touch(BUF_Z, BUF_W, BUF_ZW)
        check(self._L.aqc_ws_lbfgs_mat(self.handle, dptr(x), int(maxiter), int(memory), float(gtol), float(ftol), float(fobj_thr),
                                       float(fidelity_thr), int(max_backtracks), dptr(xo), dptr(f), dptr(fid),
                                       nit.ctypes.data_as(ctypes.POINTER(c_int64)), byref(nfev), status.ctypes.data_as(ctypes.POINTER(c_int32))))
        return {"x": xo, "fun": f, "fidelity": fid, "nit": nit, "nfev": int(nfev.value), "status": status}

    # -- measurement ---------------------------------------------------------
    def timer_start(self) -> None:
        check(self._L.aqc_ws_timer_start(self.handle))

    def timer_stop(self) -> float:
        ms = c_float()
        check(self._L.aqc_ws_timer_stop(self.handle, byref(ms)))
        return float(ms.value)

    def profile(self, on: bool) -> None:
        check(self._L.aqc_ws_profile_enable(self.handle, int(on)))
        if on:
            check(self._L.aqc_ws_profile_reset(self.handle))

    def profile_get(self, kind: int) -> Tuple[int, float]:
        n, ms = c_int64(), c_double()
        check(self._L.aqc_ws_profile_get(self.handle, kind, byref(n), byref(ms)))
        return int(n.value), float(ms.value)

    def profile_log(self) -> list:
        """(kind, ms) of every launch profiled since profile(True), in launch order."""
        n = c_int()
        check(self._L.aqc_ws_profile_log(self.handle, None, None, 0, byref(n)))
        kinds = np.zeros(max(n.value, 1), dtype=np.int32)
        ms = np.zeros(max(n.value, 1), dtype=np.float64)
        check(self._L.aqc_ws_profile_log(self.handle, kinds.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), dptr(ms), n.value, byref(n)))
        return [(int(kinds[i]), float(ms[i])) for i in range(n.value)]

    def plan_stage(self, which: int, stage: int) -> Tuple[int, int, list]:
        """(sub-stages, gate groups, local address bits) of one stage of plan ``which`` as this workspace runs it."""
        a, b = c_int(), c_int()
        bits = (c_int * 32)()
        check(self._L.aqc_ws_plan_stage(self.handle, which, stage, byref(a), byref(b), bits))
        return a.value, b.value, list(bits[: self.plan_info(which)[1]])

    def plan_skips(self, which: int, stage: int) -> list:
        """Per sub-stage of a stage: (log2 share of groups, log2 share of W K-steps) a sweep from one basis state per lane issues."""
        nsub = self.plan_stage(which, stage)[0]
        out = (c_int * (2 * max(nsub, 1)))()
        check(self._L.aqc_ws_plan_skips(self.handle, which, stage, out, nsub))
        return [(out[2 * i], out[2 * i + 1]) for i in range(nsub)]

    def sweep_r_only_sub(self) -> int:
        """Index (over all stages) of the sweep's sub-stage that is taken from its inputs alone (R-only), or -1."""
        return int(self._L.aqc_ws_sweep_r_only_sub(self.handle))

    def virtual_backwalk(self) -> int:
        """1 when an objective by projection walks its virtual stage back from (M_end, Y_end) in the launch that leaves Y_0, else 0."""
        return int(self._L.aqc_ws_virtual_backwalk(self.handle))

    def sparse_counts(self) -> Tuple[int, int, int]:
        """Items of the last sparse evaluation: (sweep first stage, tiles cleared in W, V^H last stage); -1 = never built."""
        c = (c_int64 * 3)()
        check(self._L.aqc_ws_sparse_counts(self.handle, c))
        return int(c[0]), int(c[1]), int(c[2])

    def switch(self, name: str) -> int:
        """The value of a ``create`` switch (include/aqc_switches.def) this workspace was created with."""
        v = c_int64()
        check(self._L.aqc_ws_switch(self.handle, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def projected_info(self) -> dict:
        """The projected route of the sparse-lhs sweep (its stages after the first on a virtual register), or {} without it."""
        c = (ctypes.c_int32 * 16)()
        check(self._L.aqc_ws_projected_info(self.handle, c))
        if not c[0]:
            return {}
        return {"virtual_qubits": int(c[1]), "touched_qubits": int(c[2]), "shared_with_first_stage": int(c[3]), "stages": int(c[4]),
                "substages": int(c[5]), "tile_bits": int(c[6]), "substages_on_the_register": int(c[7]), "summed_bits": int(c[8]),
                "padded_qubits": int(c[9]), "substages_per_stage": [int(c[10 + i]) for i in range(min(int(c[4]), 6))]}

    def plan_info(self, which: int) -> Tuple[int, int, int]:
        a, b, c = c_int(), c_int(), c_int()
        check(self._L.aqc_ws_plan_info(self.handle, which, byref(a), byref(b), byref(c)))
        return a.value, b.value, c.value

    _FAMILIES = {1: ("valu_fp64", "sweep_stage_kernel"), 2: ("valu_fp64", "sweep_stage_kernel2"), 3: ("mfma", "sweep_mfma_kernel")}

    def kernel_family(self, which: int = 1) -> int:
        """1 per-gate-group, 2 register-blocked (both fp64 VALU), 3 fp64 matrix cores."""
        return int(self._L.aqc_ws_kernel_family(self.handle, which))

    def plan_substages(self, which: int = 1) -> int:
        """Sub-stages of a plan (each is one 16 x 16 complex unitary per lane on the matrix-core path)."""
        return int(self._L.aqc_ws_plan_substages(self.handle, which))

    def family_name(self) -> str:
        return self._FAMILIES[self.kernel_family(1)][0]

    def sweep_kernel_name(self) -> str:
        return self._FAMILIES[self.kernel_family(1)][1]

    def close(self) -> None:
        if getattr(self, "handle", None):
            self._L.aqc_ws_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pack_mps(mps, n: int):
    """QiskitMPS tuple -> (dims int32[n+1], gammas c128 packed, lambdas f64 packed); pure marshaling."""
    gam, lam = mps
    if len(gam) != n or len(lam) != n - 1:
        raise ValueError("MPS does not match the number of qubits")
    dims = [1]
    parts = []
    for q in range(n):
        g0 = np.asarray(gam[q][0], dtype=np.complex128)
        g1 = np.asarray(gam[q][1], dtype=np.complex128)
        if g0.ndim != 2 or g0.shape != g1.shape or g0.shape[0] != dims[-1]:
            raise ValueError(f"inconsistent Gamma shapes at site {q}")
        dims.append(g0.shape[1])
        parts.append(np.stack((g0, g1)).ravel())
    lams = [np.asarray(l, dtype=np.float64).ravel() for l in lam]
    for q, l in enumerate(lams):
        if l.size != dims[q + 1]:
            raise ValueError(f"lambda {q} does not match the bond dimension")
    return (np.asarray(dims, dtype=np.int32), np.ascontiguousarray(np.concatenate(parts)),
            np.ascontiguousarray(np.concatenate(lams)) if lams else np.zeros(1))


def _ws_mps_upload(self, slot: int, mps) -> None:
    dims, gam, lam = _pack_mps(mps, self.ctx.num_qubits)
    check(self._L.aqc_ws_mps_upload(self.handle, slot, dims.ctypes.data_as(ctypes.POINTER(c_int32)), dptr(gam), dptr(lam)))


def _ws_mps_to_vec(self, slot: int, buf: int, lane: int = 0) -> None:
    self._touch(buf)
    check(self._L.aqc_ws_mps_to_vec(self.handle, slot, buf, lane))


def _ws_mps_dot(self, slot_a: int, slot_b: int) -> complex:
    out = np.empty(1, dtype=np.complex128)
    check(self._L.aqc_ws_mps_dot(self.handle, slot_a, slot_b, dptr(out)))
    return complex(out[0])


_MPS_SLOTS = 64          # AQC_MPS_SLOTS of include/aqc_hip.h
_MPS_FIRST_CACHED = 4    # slots 0..3 stay with the explicit mps_upload / mps_to_vec / mps_dot calls


_DIGEST_FULL_BYTES = 512 * 1024   # tuples up to this size are digested completely on every call
_DIGEST_WINDOW = 1024             # larger ones: three windows of this many bytes per tensor (first, middle, last) + all Schmidt vectors


def _mps_fingerprint(mps) -> tuple:
    """Content check of a QiskitMPS tuple, taken on EVERY call (identity of the tuple is only the cache key): shapes plus an
    xxh3 digest of the tensors -- all bytes for tuples up to 512 KiB (a 16-qubit target of bond 16 is 128 KiB), three 1 KiB
    windows per tensor and every Schmidt vector beyond (a bond-64 target is 2 MiB: a full pass per call and lane would cost more
    than the evaluation).  The caller's arrays are never touched: an in-place edit between two calls changes the digest and the
    resident copy is uploaded again, which is what the reference's reload on every call amounts to (mps_dot_objective.py:100-101).
    Residual hazard, stated: an edit of a few entries of a LARGE tensor outside the windows goes unseen -- pass new arrays (or
    call ``Workspace.mps_forget``) for such edits; whole-tensor edits (rescaling, truncation) always land in the windows."""
    import xxhash

    gam, lam = mps
    arrays = [np.asarray(g) for pair in gam for g in pair]
    lams = [np.asarray(l) for l in lam]
    total = sum(a.nbytes for a in arrays)
    h = xxhash.xxh3_64()
    for a in arrays:
        b = memoryview(a if a.flags.c_contiguous else np.ascontiguousarray(a)).cast("B")
        if total <= _DIGEST_FULL_BYTES or len(b) <= 3 * _DIGEST_WINDOW:
            h.update(b)
        else:
            mid = (len(b) // 2) & ~15
            h.update(b[:_DIGEST_WINDOW]); h.update(b[mid:mid + _DIGEST_WINDOW]); h.update(b[-_DIGEST_WINDOW:])
    for l in lams:
        h.update(memoryview(l if l.flags.c_contiguous else np.ascontiguousarray(l)).cast("B"))
    return (tuple(a.shape for a in arrays), h.intdigest())


def _mps_bond_dims(mps) -> tuple:
    return tuple(int(np.shape(g0)[1]) for g0, _ in mps[0][:-1])


def _pad_mps(mps, bonds):
    """The same state with every bond widened to ``bonds`` by zero rows / columns of the tensors (Schmidt entries 1 on the padding: they
    multiply zeros) -- exact, and it gives the lanes of a batch ONE common shape."""
    gam, lam = mps
    n = len(gam)
    dims = (1,) + tuple(bonds) + (1,)
    out_g = []
    for q, (g0, g1) in enumerate(gam):
        pair = []
        for g in (g0, g1):
            a = np.zeros((dims[q], dims[q + 1]), dtype=np.complex128)
            g = np.asarray(g)
            a[: g.shape[0], : g.shape[1]] = g
            pair.append(a)
        out_g.append(tuple(pair))
    out_l = []
    for q in range(n - 1):
        v = np.ones(dims[q + 1])
        src = np.asarray(lam[q], dtype=np.float64).ravel()
        v[: src.size] = src
        out_l.append(v)
    return out_g, out_l


def _ws_mps_slot_for(self, mps, bonds=None) -> int:
    """Slot holding a device-resident copy of `mps`: uploaded on first sight, found again by the tuple's identity plus a
    digest of its tensors (mps_dot_objective.py:41 receives the same target tuple on every call of an
    optimisation; the reference re-loads it into the simulator each time, :100-101).  Least recently used slot is recycled.
    ``bonds``: bond dimensions the resident copy is zero-padded to (``_pad_mps``; None: as they are)."""
    cache = self.__dict__.setdefault("_mps_cache", {})        # id(mps) -> [slot, fingerprint, tick, keep-alive reference]
    self._mps_tick = getattr(self, "_mps_tick", 0) + 1
    fp = (_mps_fingerprint(mps), None if bonds is None or tuple(bonds) == _mps_bond_dims(mps) else tuple(bonds))
    ent = cache.get(id(mps))
    if ent is not None and ent[1] == fp:
        ent[2] = self._mps_tick
        return ent[0]
    if ent is not None:
        slot = ent[0]                                           # same object, new contents: re-upload in place
    elif len(cache) < _MPS_SLOTS - _MPS_FIRST_CACHED:
        slot = _MPS_FIRST_CACHED + len(cache)
    else:
        victim = min(cache, key=lambda k: cache[k][2])
        slot = cache.pop(victim)[0]
    self.mps_upload(slot, mps if fp[1] is None else _pad_mps(mps, fp[1]))
    cache[id(mps)] = [slot, fp, self._mps_tick, mps]
    return slot


def _ws_mps_forget(self, mps) -> None:
    """Drop the resident copy of ``mps`` (after an in-place edit that the windowed digest of a large tuple may not see)."""
    ent = self.__dict__.setdefault("_mps_cache", {}).get(id(mps))
    if ent is not None:
        ent[1] = None   # (the slot stays with the tuple: the next call uploads into it again)


def _mps_basis_term(mps):
    """(index, amplitude) when the MPS is a computational-basis state times a scalar -- every bond 1, one of the two tensors of
    every site exactly zero (the |0> / flip states the objectives hand in as ``lvec``, objective_base.py:345-435) -- else None."""
    gam, lam = mps
    index, amp = 0, 1.0 + 0.0j
    for q, (g0, g1) in enumerate(gam):
        if np.size(g0) != 1 or np.size(g1) != 1:
            return None
        a0, a1 = complex(np.reshape(g0, -1)[0]), complex(np.reshape(g1, -1)[0])
        if (a0 == 0) == (a1 == 0):
            return None
        if a0 == 0:
            index |= 1 << q
        amp *= a1 if a0 == 0 else a0
    for l in lam:
        if np.size(l) != 1:
            return None
        amp *= float(np.reshape(l, -1)[0])
    return index, amp


def _ws_mps_to_vec_batch(self, mps_list, buf: int, lanes=None) -> None:
    """Dense states of `mps_list` (QiskitMPS tuples, one per lane) into lanes `lanes` (default 0..len-1) of `buf`: resident
    copies through the slot cache, lanes that share a tuple share its slot, ONE contraction chain for all lanes (operands of different
    bond dimensions are zero-padded to a common shape)."""
    lanes = np.arange(len(mps_list), dtype=np.int32) if lanes is None else np.ascontiguousarray(lanes, dtype=np.int32)
    if lanes.size != len(mps_list):
        raise ValueError("one lane per MPS")
    if buf in (BUF_X, BUF_X2) and lanes.size == self.batch and np.array_equal(lanes, np.arange(self.batch)):
        # lhs states that are basis states (what every objective sweeps from): two amplitudes per lane written in place instead of a
        # contraction chain -- and the workspace knows the support, so the sweep takes its sparse route (aqc_ws_sweep.cpp)
        terms = {id(m): _mps_basis_term(m) for m in {id(m): m for m in mps_list}.values()}
        if all(t is not None for t in terms.values()):
            self.set_combo(buf, [[terms[id(m)][0], -1] for m in mps_list], [[terms[id(m)][1], 0.0] for m in mps_list])
            return
    if len({id(m) for m in mps_list}) > _MPS_SLOTS - _MPS_FIRST_CACHED:
        raise ValueError(f"at most {_MPS_SLOTS - _MPS_FIRST_CACHED} distinct MPS per batched contraction")
    # Truncated canonical tensors (the reference's trunc_thr = 1e-6) differ from target to target by a few bond entries, and the native
    # call runs one contraction chain per distinct shape: the resident copies are zero-padded to the widest bonds among the lanes, so the
    # whole batch is one chain again (config 3 at 1e-6: 62.9 k -> the 1e-16 rate)
    distinct = {id(m): m for m in mps_list}
    shapes = {_mps_bond_dims(m) for m in distinct.values()}
    bonds = tuple(max(b) for b in zip(*shapes)) if len(shapes) > 1 else None
    by_id = {}
    slots = np.empty(len(mps_list), dtype=np.int32)
    for i, m in enumerate(mps_list):
        if id(m) not in by_id:
            by_id[id(m)] = self.mps_slot_for(m, bonds)
        slots[i] = by_id[id(m)]
    i32 = ctypes.POINTER(c_int32)
    check(self._L.aqc_ws_mps_to_vec_batch(self.handle, int(slots.size), slots.ctypes.data_as(i32), buf, lanes.ctypes.data_as(i32)))
    self._touch(buf)


Workspace.mps_upload = _ws_mps_upload
Workspace.mps_to_vec = _ws_mps_to_vec
Workspace.mps_dot = _ws_mps_dot
Workspace.mps_slot_for = _ws_mps_slot_for
Workspace.mps_forget = _ws_mps_forget
Workspace.mps_to_vec_batch = _ws_mps_to_vec_batch


class RankDeficientSketch(RuntimeError):
    """The device QR of a lane's sketching matrix met a vanishing pivot (for instance ``eigen`` with V = U: nothing left to sketch).
    ``lanes`` names the lanes."""

    def __init__(self, lanes):
        self.lanes = [int(b) for b in lanes]
        super().__init__(f"aqc_hip: the sketching matrix of lane(s) {self.lanes} is rank deficient")


def qr(a: np.ndarray, device: Optional[int] = None) -> np.ndarray:
    """Orthonormal basis of the columns of ``a`` (m x k, k a power of two <= 64) by the device's CholeskyQR2 (aqc_qr): what
    ``np.linalg.qr(a)[0]`` spans.  Raises RankDeficientSketch when a pivot vanishes or ``a`` is too ill-conditioned (from about 1e6
    with its columns scaled to norm 1) for two passes to end orthonormal."""
    a = _lib.as_c128(a)
    if a.ndim != 2:
        raise ValueError("qr expects a matrix")
    q = np.empty_like(a)
    st = c_int32(0)
    check(_lib.lib().aqc_qr(default_device() if device is None else int(device), a.shape[0], a.shape[1], dptr(a), dptr(q), byref(st)))
    if st.value:
        raise RankDeficientSketch([0])
    return q


def zgemm(a: np.ndarray, b: np.ndarray, conj_trans_a: bool = False, device: Optional[int] = None) -> np.ndarray:
    """op(a) @ b on the device (aqc_zgemm); op(a) = a or a^H."""
    a = _lib.as_c128(a)
    b = _lib.as_c128(b)
    if a.ndim != 2 or b.ndim != 2:
        raise ValueError("zgemm expects two matrices")
    m, k = (a.shape[1], a.shape[0]) if conj_trans_a else a.shape
    if b.shape[0] != k:
        raise ValueError("inner dimensions differ")
    c = np.empty((m, b.shape[1]), dtype=np.complex128)
    check(_lib.lib().aqc_zgemm(default_device() if device is None else int(device), int(conj_trans_a), m, b.shape[1], k, dptr(a), a.shape[1], dptr(b), b.shape[1], dptr(c), c.shape[1]))
    return c
