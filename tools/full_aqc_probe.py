#!/usr/bin/env python
"""Full AQC (1 - Re<V, U>/d by L-BFGS): the same number of iterations through the host loop (batched_lbfgs on
BatchedSketchingObjective.value_and_grad: thetas up, trace and B x T complex gradients down, the two-loop recursion in NumPy) and
through the device-resident loop (minimize_on_device, aqc_ws_lbfgs_mat), timed in one process, interleaved, median of --reps after
a warm-up.

Shapes: the tutorial's 5-qubit ansatz (cyclic spin, 180 blocks) and n = 10, 40 blocks; 1 lane and 64 lanes (--lanes).  The targets are
planted (V at random thetas) and the starts perturbed, so the iterations are real line searches, not a plateau.  Prints one JSON line per
(shape, lanes): both medians per iteration, their spread, evaluations per run, the cost each loop reaches.

Memory: a workspace holds up to six 2^n x 2^n complex128 buffers per lane, and the targets are built on a second workspace and pass
through the host.  n = 10 at 64 lanes is 1 GiB per buffer: several GiB on the device and 1 GiB on the host."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aqc_research_amd import ParametricCircuit  # noqa: E402
from aqc_research_amd.batched_optimizer import BatchedSketchingObjective, batched_lbfgs  # noqa: E402
from aqc_research_amd.circuit_structures import create_ansatz_structure  # noqa: E402
from aqc_research_amd.engine import BUF_X, BUF_Y, HipContext, Workspace  # noqa: E402

SHAPES = {"mat5_cyc180": (5, "cyclic_spin", 180), "mat10_l40": (10, "spin", 40)}


def _targets(circ, truth):
    """V(truth) of every lane, computed on the device: V applied to the identity."""
    ws = Workspace(HipContext.of(circ), batch=len(truth), ncols=circ.dimension)
    ws.set_identity(BUF_X)
    ws.set_thetas(truth)
    ws.apply(False, BUF_X, BUF_Y)
    out = ws.download(BUF_Y)
    ws.close()
    return out


def _host(bo, x0, iters):
    t0 = time.perf_counter()
    res = batched_lbfgs(bo.value_and_grad, x0, maxiter=iters)
    return time.perf_counter() - t0, res


def _device(bo, x0, iters):
    t0 = time.perf_counter()
    res = bo.minimize_on_device(x0, maxiter=iters)
    return time.perf_counter() - t0, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lanes", default="1,64")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    if args.reps < 1 or args.iters < 1:
        ap.error("--reps and --iters must be positive")
    for name in args.shapes.split(","):
        n, layout, depth = SHAPES[name]
        circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, layout, "full", depth))
        for lanes in (int(v) for v in args.lanes.split(",")):
            rng = np.random.default_rng(7)
            truth = np.pi * (2 * rng.random((lanes, circ.num_thetas)) - 1)
            x0 = truth + 0.05 * rng.standard_normal(truth.shape)
            bo = BatchedSketchingObjective(circ, _targets(circ, truth))
            _host(bo, x0, args.iters)
            _device(bo, x0, args.iters)
            host, dev = [], []
            for _ in range(args.reps):     # interleaved: both loops see the same clocks and the same neighbours
                t, rh = _host(bo, x0, args.iters)
                host.append(t)
                t, rd = _device(bo, x0, args.iters)
                dev.append(t)
            bo.close()
            it_h, it_d = max(int(rh["nit"].max()), 1), max(int(rd["nit"].max()), 1)
            print(json.dumps({"shape": name, "lanes": lanes, "maxiter": args.iters, "reps": len(host),
                              "iterations_host": it_h, "iterations_device": it_d, "nfev_host": int(rh["nfev"]), "nfev_device": int(rd["nfev"]),
                              "host_loop_ms_per_iter": 1e3 * statistics.median(host) / it_h,
                              "device_loop_ms_per_iter": 1e3 * statistics.median(dev) / it_d,
                              "host_loop_spread_ms": [1e3 * min(host) / it_h, 1e3 * max(host) / it_h],
                              "device_loop_spread_ms": [1e3 * min(dev) / it_d, 1e3 * max(dev) / it_d],
                              "cost_host_max": float(rh["fun"].max()), "cost_device_max": float(rd["fun"].max()),
                              "max_abs_cost_difference": float(np.abs(rh["fun"] - rd["fun"]).max())}), flush=True)


if __name__ == "__main__":
    main()
