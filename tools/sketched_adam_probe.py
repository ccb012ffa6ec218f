#!/usr/bin/env python
"""Sketched AQC: the same number of ADAM iterations through the host loop (AqcOptimizer("adam") on SketchingObjectiveEx: draws, QR,
uploads and the theta update on the host, two synchronisations per iteration) and through the device-resident loop
(model_sketching.aqc_sketching.stochastic_aqc), timed in one process, interleaved, median of --reps after a warm-up.

Shapes: the tutorial's 5-qubit ansatz (cyclic spin, 180 blocks, 16 `alt` vectors) and n = 10, 40 blocks, k = 16.  Prints one JSON
line per shape: both medians, the device loop's kernel time per iteration from the workspace's profile, the cost reached."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aqc_research_amd import ParametricCircuit  # noqa: E402
from aqc_research_amd.circuit_structures import create_ansatz_structure  # noqa: E402
from aqc_research_amd.engine import HipContext, Workspace  # noqa: E402
from aqc_research_amd.model_sketching.aqc_sketching import AltIndexSchedule, stochastic_aqc  # noqa: E402
from aqc_research_amd.model_sketching.sk_core import SketchingObjectiveEx, skvecs_generator  # noqa: E402
from aqc_research_amd.optimizer import AqcOptimizer  # noqa: E402

SHAPES = {"mat5_cyc180_k16": (5, "cyclic_spin", 180, 16), "mat10_l40_k16": (10, "spin", 40, 16)}


def _host(circ, target, kind, k, th0, iters):
    objv = SketchingObjectiveEx(circ, skvecs_generator(kind, k, target))
    t0 = time.perf_counter()
    res = AqcOptimizer(optimizer_name="adam", maxiter=iters, learn_rate=0.1).optimize(objv, circ, th0)
    return time.perf_counter() - t0, res["cost"]


def _device(circ, target, kind, k, th0, iters, seed):
    t0 = time.perf_counter()
    res = stochastic_aqc(circ, target, kind, k, th0, maxiter=iters, learn_rate=0.1, seed=seed, chunk=iters)
    return time.perf_counter() - t0, res["cost"]


def _kernel_ms_per_iteration(circ, target, kind, k, th0, iters):
    ws = Workspace(HipContext.of(circ), batch=1, ncols=k)
    ws.sketch_target(target)
    idx = AltIndexSchedule(circ.dimension, k, 1).take(iters + 1) if kind == "alt" else None
    ws.sketch_adam(kind, th0, iters, 0.1, alt_idx=idx)   # warm-up
    ws.profile(True)
    ws.sketch_adam(kind, th0, iters, 0.1, reset=1, alt_idx=idx)
    total = sum(ws.profile_get(kd)[1] for kd in range(10))
    ws.close()
    return total / (iters + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--kind", default="alt", choices=["rand", "alt", "eigen"])
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    for name in args.shapes.split(","):
        n, layout, depth, k = SHAPES[name]
        rng = np.random.default_rng(7)
        circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, layout, "full", depth))
        d = 1 << n
        target = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))[0])
        th0 = np.pi * (2 * rng.random(circ.num_thetas) - 1)
        np.random.seed(1)
        _host(circ, target, args.kind, k, th0, args.iters)
        _device(circ, target, args.kind, k, th0, args.iters, 0)
        host, dev, cost_h, cost_d = [], [], 0.0, 0.0
        for r in range(max(args.reps, 10)):     # interleaved: both loops see the same clocks and the same neighbours
            t, cost_h = _host(circ, target, args.kind, k, th0, args.iters)
            host.append(t)
            t, cost_d = _device(circ, target, args.kind, k, th0, args.iters, r)
            dev.append(t)
        kern = _kernel_ms_per_iteration(circ, target, args.kind, k, th0, args.iters)
        print(json.dumps({"shape": name, "kind": args.kind, "iterations": args.iters, "reps": len(host),
                          "host_loop_ms_per_iter": 1e3 * statistics.median(host) / args.iters,
                          "device_loop_ms_per_iter": 1e3 * statistics.median(dev) / args.iters,
                          "host_loop_spread_ms": [1e3 * min(host) / args.iters, 1e3 * max(host) / args.iters],
                          "device_loop_spread_ms": [1e3 * min(dev) / args.iters, 1e3 * max(dev) / args.iters],
                          "device_kernel_ms_per_iter": kern, "cost_host": cost_h, "cost_device": cost_d}), flush=True)


if __name__ == "__main__":
    main()
