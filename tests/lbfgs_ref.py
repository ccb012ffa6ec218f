"""The device L-BFGS rule (csrc/aqc_lbfgs.hip, csrc/aqc_ws_optim.cpp) stated in NumPy for B lanes, with a trace.

Written from the kernels and their comments, kernel by kernel, not from the host loop in batched_optimizer.py (which
tests/test_lbfgs_ref.py compares it with).  ``fun(x[B][T]) -> (f[B], g[B][T])`` has no state: this is the rule of
``aqc_ws_lbfgs_mat``, and of ``aqc_ws_lbfgs`` for as long as |state_0> leads on every lane (the accepted trial's value and
gradient are then final, lb_commit0_kernel).  One iteration ``count``:

  lb_direction   q = g; for j = k-1 .. 0 (k = min(count, memory)), slot (count - k + j) % memory: alpha_j = rho <s, q>, q -= alpha_j y;
                 k > 0: q *= gamma = 1 / (rho <y, y>) of the last pair (1 where yy or rho is not positive); k = 0: q /= max(|g|_2, 1);
                 for j = 0 .. k-1: q += (alpha_j - rho <y, q>) s; d = -q, slope = <g, d>; slope >= 0: d = -g, slope = -<g, g>;
                 step = 1 on active lanes, 0 on the others, which are done from the start
  lb_trial       x + step d for every lane -- an inactive lane is evaluated at its own point
  lb_armijo      a lane that is not done accepts when ft <= f + c1 step slope, else halves its step; trials end when no lane
                 halves any more or after max_backtracks of them
  lb_history     s = x_new - x, y = g_acc - g into slot count % memory, zeroed unless the lane was active, accepted, moved and
                 sy > 1e-12 yy; rho = 1 / sy or 0; nit += active; active &= moved and not |f - f_acc| <= ftol max(1, |f|)

and at the top of every iteration (lb_active / lb_mat_goes_on) active &= max|g| > gtol; the loop ends when no lane is active.
"""
import numpy as np

__all__ = ["lbfgs_ref"]


def _dot(a, b):
    return np.einsum("bt,bt->b", a, b)


def lbfgs_ref(fun, x0, *, maxiter=100, memory=10, gtol=1e-7, ftol=1e-12, c1=1e-4, max_backtracks=12):
    """Returns {"x", "fun", "jac", "gmax", "nit", "nfev", "active", "trace"}; ``gmax`` is max|g| at the final point, which the
    next iteration's gtol test would see.  ``nfev`` counts evaluations of the batch as the device
    does: the start point and one per line-search trial.  ``trace[k]`` describes iteration k (0-based), which leads from point k
    to point k + 1:

      x, f          the point and value AFTER the iteration (x_{k+1}, f_{k+1}), [B][T] and [B]
      f_in          the value at the point the iteration started from
      gmax, tested  max|g| at that point -- what the gtol test saw -- and the lanes still active when it was taken
      d, slope      search direction and <g, d>
      step          the accepted step length (0 on lanes that accepted nothing)
      trials        [B] trials each lane took part in (0 on a lane that entered inactive)
      margins       one [B] array per trial: ft - (f + c1 step slope) on the lanes that took the Armijo test there, NaN elsewhere
      good          [B] the pair went into the history (else the slot was zeroed)
      active_in     [B] active after the gtol test at the top of this iteration
      active        [B] active after it (before the next gtol test)
    """
    x = np.array(x0, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("x0 must have shape (lanes, T)")
    if not 1 <= int(memory) <= 32:
        raise ValueError("the L-BFGS memory must be in [1, 32]")     # alpha[32] in lb_direction_body
    if int(maxiter) < 1 or int(max_backtracks) < 1:
        raise ValueError("maxiter and max_backtracks must be positive")
    if not (gtol >= 0.0) or not (ftol >= 0.0):
        raise ValueError("tolerances must not be negative")
    memory, maxiter, max_backtracks = int(memory), int(maxiter), int(max_backtracks)
    B, T = x.shape
    f, g = fun(x)
    f, g = np.array(f, dtype=np.float64), np.array(g, dtype=np.float64)
    nfev = 1
    S, Y, rho = np.zeros((memory, B, T)), np.zeros((memory, B, T)), np.zeros((memory, B))
    active = np.ones(B, dtype=bool)
    nit = np.zeros(B, dtype=np.int64)
    trace = []
    for count in range(maxiter):
        gmax = np.max(np.abs(g), axis=1)
        tested = active.copy()
        active = active & (gmax > gtol)
        if not active.any():
            break
        active_in = active.copy()
        # ---- lb_direction
        k = min(count, memory)
        q = g.copy()
        alpha = np.zeros((k, B))
        for j in range(k - 1, -1, -1):
            slot = (count - k + j) % memory
            alpha[j] = rho[slot] * _dot(S[slot], q)
            q -= alpha[j][:, None] * Y[slot]
        if k:
            last = (count - 1) % memory
            yy, r = _dot(Y[last], Y[last]), rho[last]
            ok = (yy > 0.0) & (r > 0.0)
            q *= np.where(ok, 1.0 / np.where(ok, r * yy, 1.0), 1.0)[:, None]
        else:
            q /= np.maximum(np.sqrt(_dot(g, g)), 1.0)[:, None]
        for j in range(k):
            slot = (count - k + j) % memory
            beta = rho[slot] * _dot(Y[slot], q)
            q += (alpha[j] - beta)[:, None] * S[slot]
        d = -q
        slope = _dot(g, d)
        up = slope >= 0.0
        d[up] = -g[up]
        slope[up] = -_dot(g[up], g[up])
        step = np.where(active, 1.0, 0.0)
        done = ~active
        x_new, f_acc, g_acc = x.copy(), f.copy(), g.copy()
        trials = np.zeros(B, dtype=np.int64)
        margins = []
        taken = np.zeros(B)
        # ---- lb_trial, the evaluation, lb_armijo
        for _ in range(max_backtracks):
            xt = x + step[:, None] * d
            ft, gt = fun(xt)
            nfev += 1
            testing = ~done
            trials += testing
            margin = ft - (f + c1 * step * slope)
            margins.append(np.where(testing, margin, np.nan))
            ok = testing & (ft <= f + c1 * step * slope)
            x_new[ok], f_acc[ok], g_acc[ok] = xt[ok], np.asarray(ft)[ok], np.asarray(gt)[ok]
            taken[ok] = step[ok]
            done = done | ok
            if done.all():
                break
            step = np.where(done, step, 0.5 * step)
        # ---- lb_history
        s, y = x_new - x, g_acc - g
        sy, yy = _dot(s, y), _dot(y, y)
        moved = done & active & (s != 0.0).any(axis=1)
        good = moved & (sy > 1e-12 * yy)
        slot = count % memory
        S[slot] = np.where(good[:, None], s, 0.0)
        Y[slot] = np.where(good[:, None], y, 0.0)
        rho[slot] = np.where(good, 1.0 / np.where(good, sy, 1.0), 0.0)
        small = np.abs(f - f_acc) <= ftol * np.maximum(1.0, np.abs(f))
        nit += active
        active = active & moved & ~small
        f_in = f
        x, f, g = x_new, f_acc, g_acc
        trace.append({"x": x.copy(), "f": f.copy(), "f_in": f_in, "gmax": gmax, "tested": tested, "d": d, "slope": slope, "step": taken, "trials": trials,
                      "margins": margins, "good": good, "active_in": active_in, "active": active.copy()})
    return {"x": x, "fun": f, "jac": g, "gmax": np.max(np.abs(g), axis=1), "nit": nit, "nfev": nfev, "active": active, "trace": trace}
