"""
Coordinate-descent AQC with every sweep and every stop rule on the device: the counterpart of ``_single_simulation``
(aqc_coord_descent.py:32-122) for one problem or a batch of lanes (restarts and / or targets).

The objective is ``1 - |<V(thetas), U>|^2 / d^2``; a sweep updates every parameter once (``core_op_matrix.coord_descent_single_sweep``).
The loop of the reference (:70-101) -- best value and thetas so far, "normal" when no theta moved by 1e-8 or ``maxiter`` is reached,
"early" below ``fobj_thr``, "timeout" -- runs in ``Workspace.cd_minimize``.  One difference follows from that: the host looks at its
clock once per ``chunk`` sweeps, so ``time_limit`` ends the lanes still running at the end of a chunk, never in the middle of one
(``chunk=1`` is the reference's timing at one host visit per sweep).
"""
from typing import Optional

import numpy as np

from .. import _lib
from ..engine import BUF_X, BUF_Y, BUF_Z, HipContext, Workspace
from ..parametric_circuit import TrotterAnsatz


def coordinate_descent_aqc(circ, target: np.ndarray, thetas_0: np.ndarray, *, maxiter: int, time_limit: float = -1, fobj_thr: float = 1e-2,
                           thetas_change_thr: float = 1e-8, chunk: int = 64, device: Optional[int] = None, route: str = "auto"):
    """``thetas_0``: (T,) for one problem or (lanes, T); ``target``: (d, d) shared by the lanes or (lanes, d, d).  ``route``: "auto"
    (one persistent launch per chunk up to 6 qubits, the wide walk beyond), "persistent" or "wide".  Returns the reference's result
    dictionary (:103-121) -- cost, nit, num_fun_ev, num_grad_ev, num_iters, ini_thetas, thetas (the best ones), entangler, blocks,
    fidelity (at the best thetas), stats = {convergence_profile (float32, nit values), nit}, exit_status ("normal" / "early" /
    "timeout") -- or a list of them for ``(lanes, T)`` starts.  ``time_limit`` in seconds (<= 0: none) acts between chunks of
    ``chunk`` sweeps."""
    if isinstance(circ, TrotterAnsatz):
        raise ValueError("the matrix path takes a plain ParametricCircuit (core_op_matrix.py:480-559)")
    if circ.entangler == "cp":
        raise NotImplementedError("CPhase entangler is not supported yet")
    if route not in _lib.CD_ROUTES:
        raise ValueError(f"route must be one of {sorted(_lib.CD_ROUTES)}, got {route!r}")
    if not (int(maxiter) > 0 and int(chunk) > 0):
        raise ValueError("maxiter and chunk must be positive")
    th0 = np.array(thetas_0, dtype=np.float64)
    single = th0.ndim == 1
    th0 = np.atleast_2d(th0)
    if th0.ndim != 2 or th0.shape[1] != circ.num_thetas:
        raise ValueError("thetas_0: expects (circ.num_thetas,) or (lanes, circ.num_thetas)")
    lanes, d = th0.shape[0], circ.dimension
    tg = np.asarray(target)
    if tg.dtype != np.complex128 or tg.ndim not in (2, 3) or tg.shape[-2:] != (d, d):
        raise ValueError("target: expects complex128 (d, d) or (lanes, d, d)")
    if tg.ndim == 3 and tg.shape[0] != lanes:
        raise ValueError("one target per lane, or one for all")
    ws = Workspace(HipContext.of(circ), batch=lanes, ncols=d, device=device)
    try:
        ws.upload(BUF_Y, np.ascontiguousarray(np.broadcast_to(tg, (lanes, d, d))))
        res = ws.cd_minimize(th0, int(maxiter), chunk=int(chunk), dtheta_thr=float(thetas_change_thr), fobj_thr=float(fobj_thr),
                             time_limit=float(time_limit), route=route)
        # fidelity at the best thetas (:110, sk_utils.fidelity): (1 + |Tr V^H U|^2 / d) / (d + 1), the trace as <I|V^H U>
        ws.set_thetas(res["thetas"])
        ws.apply(True, BUF_Y, BUF_Z)
        ws.set_identity(BUF_X)
        tr = ws.vdot(BUF_X, BUF_Z)
    finally:
        ws.close()
    out = []
    for b in range(lanes):
        nit = int(res["nit"][b])
        out.append({"cost": float(res["cost"][b]), "nit": nit, "num_fun_ev": nit, "num_grad_ev": nit, "num_iters": nit,
                    "ini_thetas": th0[b].copy(), "thetas": res["thetas"][b].copy(), "entangler": circ.entangler, "blocks": circ.blocks.copy(),
                    "fidelity": float((1.0 + abs(tr[b]) ** 2 / d) / (d + 1)),
                    "stats": {"convergence_profile": res["profile"][b, :nit].astype(np.float32), "nit": nit},
                    "exit_status": _lib.CD_STATUS[int(res["status"][b])]})
    return out[0] if single else out
