"""
Sketched AQC with every ADAM iteration on the device: the counterpart of ``_stochastic_aqc`` (aqc_sketching.py:53-104) for one
problem or a batch of lanes (restarts and / or targets).

The device runs the iterations in chunks (``Workspace.sketch_adam``: generate, V^H Y, trace, sweep, ADAM step, nothing on the
host in between); the restart policy of the reference stays on the host and looks at each chunk's objective values afterwards.
Differences from the reference, all of them consequences of that split:

* the sketching draws come from Philox (csrc/aqc_philox.h) instead of ``np.random``; ``alt`` permutations are still drawn on the
  host with the reference's rule and sent as indices;
* a stagnation warning is noticed at the END of the chunk in which the ``NotImproveStopper`` fired: the lane finishes that chunk
  with the old learning rate, then restarts from its best thetas with the learning rate halved (``chunk=1`` reproduces the
  reference's timing at one host visit per iteration);
* as in the reference, every objective call counts as an iteration, the budget of a restarted run shrinks by ALL evaluations made
  so far (``maxiter -= objv.num_iterations``, aqc_sketching.py:100), and after the last correction the stopper is disabled and
  the run restarts from the start point of the previous run.
"""
import copy
from typing import Optional

import numpy as np

from ..engine import HipContext, RankDeficientSketch, Workspace
from ..optimizer import NotImproveStopper, StagnantOptimizationWarning


class AltIndexSchedule:
    """Column indices of AlternatingSketchingVectors (sk_core.py:359-401) for ``lanes`` independent generators: a permutation of
    range(d) per lane, consumed k at a time, redrawn from ``np.random`` when the offset runs past d."""

    def __init__(self, dim: int, num_skvecs: int, lanes: int = 1):
        if dim % num_skvecs:
            raise ValueError("the dimension must be divisible by num_skvecs")
        self._dim, self._k, self._offset = int(dim), int(num_skvecs), 0
        self._perm = [np.random.permutation(dim) for _ in range(lanes)]

    def next(self) -> np.ndarray:
        """(lanes, k) indices of the next request."""
        if self._offset >= self._dim:
            self._offset = 0
            self._perm = [np.random.permutation(self._dim) for _ in self._perm]
        out = np.stack([p[self._offset:self._offset + self._k] for p in self._perm]).astype(np.int32)
        self._offset += self._k
        return out

    def take(self, count: int) -> np.ndarray:
        return np.stack([self.next() for _ in range(count)])

    def rewind(self, count: int) -> None:
        """Give back the last ``count`` requests (they did not cross a redraw): the evaluation that closes a chunk is made again by
        the next one under the same sketch."""
        self._offset -= count * self._k
        if self._offset < 0:
            raise ValueError("cannot rewind across a redraw")


class ChunkPolicy:
    """One lane's restart policy of ``_stochastic_aqc`` fed with chunks of objective values (host only)."""

    def __init__(self, maxiter: int, learn_rate: float, stopper: Optional[NotImproveStopper], max_corrections: int = 5):
        self.budget, self.learn_rate, self.stopper = int(maxiter), float(learn_rate), stopper
        self.max_corrections, self.corrections = int(max_corrections), 0
        self.run_iters = 0        # evaluations of the current ADAM run
        self.evals_total = 0      # of all runs (SketchingObjectiveEx.num_iterations)
        self.finished, self.exit_status = False, None
        self.restart_from_best = False

    @property
    def remaining(self) -> int:
        return self.budget - self.run_iters

    def feed(self, profile) -> bool:
        """The objective values of one chunk, in evaluation order.  True when the stopper fired: the lane restarts (from its best
        thetas while corrections are left) with ``learn_rate`` as it is afterwards."""
        fired = False
        for i, f in enumerate(profile):
            if self.stopper is None:
                break
            try:
                self.stopper.check(fobj=float(f), iter_no=self.evals_total + i + 1)
            except StagnantOptimizationWarning:
                fired = True
                break
        self.evals_total += len(profile)
        self.run_iters += len(profile)
        if fired:
            self.corrections += 1
            self.restart_from_best = self.corrections < self.max_corrections
            if self.restart_from_best:
                self.stopper.reset()
                self.learn_rate *= 0.5
            else:
                self.stopper.disable()
            self.budget -= self.evals_total
            self.run_iters = 0
            if self.budget <= 0:
                self.finished, self.exit_status = True, "premature"
        elif self.run_iters >= self.budget:
            self.finished, self.exit_status = True, "normal"
        return fired

    def converged(self) -> None:
        self.finished, self.exit_status = True, "normal"


def stochastic_aqc(circ, target: np.ndarray, skvecs_type: str, num_skvecs: int, thetas_0: np.ndarray, *, maxiter: int, learn_rate: float,
                   seed: int = 0, chunk: int = 32, device: Optional[int] = None, stop_stagnant: Optional[NotImproveStopper] = None):
    """ADAM on the sketched objective with restarts, device-resident.  ``thetas_0``: (T,) for one problem or (lanes, T);
    ``target``: (d, d) shared by the lanes or (lanes, d, d).  ``stop_stagnant`` (a NotImproveStopper raising
    StagnantOptimizationWarning; each lane gets a copy) drives the restarts; None: a single ADAM run per lane.  Returns the
    dictionary of ``SketchingObjectiveEx.optim_results`` plus ``exit_status`` ("normal" / "premature"), a list of them for
    ``(lanes, T)`` starts.  Raises RankDeficientSketch naming the lanes whose sketching matrix lost rank."""
    if skvecs_type not in ("rand", "alt", "eigen"):
        raise ValueError(f"the device loop serves the 'rand', 'alt' and 'eigen' generators, got {skvecs_type!r} (full AQC: full_aqc in this module)")
    if not (maxiter > 0 and 0 < learn_rate < 1 and chunk > 0):
        raise ValueError("maxiter and chunk must be positive and 0 < learn_rate < 1")
    th0 = np.array(thetas_0, dtype=np.float64)
    single = th0.ndim == 1
    th0 = np.atleast_2d(th0)
    lanes, dim, k = th0.shape[0], circ.dimension, int(num_skvecs)
    if th0.shape[1] != circ.num_thetas:
        raise ValueError("thetas_0 does not match the circuit")
    ws = Workspace(HipContext.of(circ), batch=lanes, ncols=k, device=device)
    try:
        ws.sketch_target(target)
        sched = AltIndexSchedule(dim, k, lanes) if skvecs_type == "alt" else None
        pols = [ChunkPolicy(maxiter, learn_rate, copy.deepcopy(stop_stagnant)) for _ in range(lanes)]
        start = th0.copy()                 # start point of each lane's current run (ini_thetas of the reference)
        final_x, final_cost = th0.copy(), np.full(lanes, 1e30)
        best_f, best_x = np.full(lanes, np.inf), th0.copy()
        reset = np.ones(lanes, dtype=np.int32)
        fed = [[] for _ in range(lanes)]   # per lane: the objective values handed to its policy, chunk by chunk
        sketch_no = 0
        while not all(p.finished for p in pols):
            n = min([int(chunk)] + [p.remaining for p in pols if not p.finished])
            idx = None if sched is None else sched.take(n + 1)
            res = ws.sketch_adam(skvecs_type, start, n, [p.learn_rate for p in pols], seed=seed, iter0=sketch_no, reset=reset, alt_idx=idx)
            if sched is not None:
                sched.rewind(1)
            sketch_no += n
            bad = np.flatnonzero(res["status"])
            if bad.size:
                raise RankDeficientSketch(bad)
            for b, p in enumerate(pols):
                if p.finished:
                    continue
                if res["best_f"][b] < best_f[b]:
                    best_f[b], best_x[b] = res["best_f"][b], res["best_x"][b]
                nit = int(res["nit"][b])
                done = nit < n                                   # the step norm fell below ADAM's tolerance
                fed[b].append(np.array(res["profile"][b, :nit + 1] if done else res["profile"][b, :n]))
                fired = p.feed(fed[b][-1])
                final_x[b], final_cost[b] = res["x"][b], res["cost"][b]
                if fired and not p.finished:
                    if p.restart_from_best:
                        start[b] = best_x[b]
                    reset[b] = 1
                elif done and not fired:
                    p.converged()
                else:
                    reset[b] = 0
                if p.finished:
                    reset[b] = 2
    finally:
        ws.close()
    out = []
    for b, p in enumerate(pols):
        normal = p.exit_status == "normal"
        out.append({"cost": float(final_cost[b] if normal else best_f[b]), "num_fun_ev": p.evals_total, "num_grad_ev": p.evals_total,
                    "num_iters": p.evals_total, "thetas": (final_x[b] if normal else best_x[b]).copy(), "entangler": circ.entangler,
                    "blocks": circ.blocks.copy(), "exit_status": p.exit_status, "learn_rate": p.learn_rate, "corrections": p.corrections,
                    "stats": {"chunks": fed[b], "convergence_profile": np.concatenate(fed[b]).astype(np.float32)}})
    return out[0] if single else out


def full_aqc(circ, target: np.ndarray, thetas_0: np.ndarray, *, maxiter: int, device: Optional[int] = None, fobj_thr: float = 0.0):
    """Full AQC, ``1 - Re<V(thetas), U>/d`` minimised by L-BFGS with every iteration on the device: the counterpart of ``_full_aqc``
    (aqc_sketching.py:35-50) for one problem or a batch of lanes.  ``thetas_0``: (T,) or (lanes, T); ``target``: (d, d) shared by the
    lanes or (lanes, d, d).  ``fobj_thr`` > 0 stops a lane once its cost is that small (the reference's SmallObjectiveStopper).
    Returns the dictionary of ``SketchingObjectiveEx.optim_results`` plus ``exit_status``, and a list of them for ``(lanes, T)``
    starts: the keys of ``stochastic_aqc`` without ``learn_rate``, ``corrections`` and ``stats``, which belong to ADAM and its
    chunks (``_full_aqc`` has none of them either).  ``exit_status`` is "early" when the lane ended at a cost <= ``fobj_thr`` and
    "normal" otherwise.  A lane stops at the first accepted point that small, whatever else holds there (gtol, ftol, the last
    iteration), just as the reference's stopper fires on the first evaluation below its threshold before the optimiser tests
    anything, so the final cost alone tells that the threshold ended the lane.  The optimiser is this package's L-BFGS
    (``BatchedSketchingObjective.minimize_on_device``), not scipy's L-BFGS-B: same objective, not the same trajectory."""
    from ..batched_optimizer import BatchedSketchingObjective

    if not maxiter > 0:
        raise ValueError("maxiter must be positive")
    th0 = np.array(thetas_0, dtype=np.float64)
    single = th0.ndim == 1
    th0 = np.atleast_2d(th0)
    if th0.ndim != 2 or th0.shape[1] != circ.num_thetas:
        raise ValueError("thetas_0 does not match the circuit")
    lanes = th0.shape[0]
    tg = np.asarray(target)
    if tg.ndim == 3 and tg.shape[0] != lanes:
        raise ValueError("one target per lane, or one for all")
    bo = BatchedSketchingObjective(circ, tg, lanes=lanes, device=device)
    try:
        res = bo.minimize_on_device(th0, maxiter=int(maxiter), fobj_thr=float(fobj_thr))
    finally:
        bo.close()
    bad = np.flatnonzero(res["status"])
    if bad.size:
        raise FloatingPointError(f"the objective or its gradient is not finite on lanes {bad.tolist()}")
    out = []
    for b in range(lanes):
        early = fobj_thr > 0 and res["fun"][b] <= fobj_thr
        out.append({"cost": float(res["fun"][b]), "num_fun_ev": int(res["nfev"]), "num_grad_ev": int(res["nfev"]),
                    "num_iters": int(res["nit"][b]), "thetas": res["x"][b].copy(), "entangler": circ.entangler,
                    "blocks": circ.blocks.copy(), "exit_status": "early" if early else "normal"})
    return out[0] if single else out
