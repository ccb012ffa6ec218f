#!/usr/bin/env python
"""Coordinate-descent AQC beyond 6 qubits: one sweep of the wide walk (Workspace.cd_minimize, route "wide": one launch per parameter
and one per segment; core_op_matrix.coord_descent_single_sweep is the same code at one lane) at one lane and at --lanes lanes, timed in
one process, median of --reps after a warm-up, with min - max.

Shapes: 8 qubits / 24 blocks and 10 qubits / 40 blocks (spin layout, random unitary-like targets V(random thetas)); the lanes run at 8
qubits (per sweep, all lanes).  Also timed: --tutorial-sweeps sweeps of the 5-qubit tutorial ansatz (cyclic spin, 180 blocks) through
the driver on the persistent route against coord_descent_sweeps, interleaved: the cost of the stop rules there.  Every timing includes
the upload of the thetas and the fetch of the results.  Prints one JSON line per measurement, with the launches per sweep counted from
the shape."""
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
from aqc_research_amd.core_op_matrix import coord_descent_sweeps  # noqa: E402
from aqc_research_amd.engine import BUF_X, BUF_Y, HipContext, Workspace  # noqa: E402

SHAPES = {"mat8_l24": (8, "spin", 24), "mat10_l40": (10, "spin", 40)}


def _targets(circ, truth):
    ws = Workspace(HipContext.of(circ), batch=len(truth), ncols=circ.dimension)
    ws.set_identity(BUF_X)
    ws.set_thetas(truth)
    ws.apply(False, BUF_X, BUF_Y)
    out = ws.download(BUF_Y)
    ws.close()
    return out


def _stats(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--lanes", type=int, default=16)
    ap.add_argument("--tutorial-sweeps", type=int, default=1000)
    args = ap.parse_args()
    if args.reps < 1:
        ap.error("--reps must be positive")
    rng = np.random.default_rng(5)
    for name in args.shapes.split(","):
        n, layout, depth = SHAPES[name]
        circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, layout, "full", depth))
        T, L = circ.num_thetas, circ.num_blocks
        th0 = np.pi * (2 * rng.random(T) - 1)
        u = _targets(circ, np.pi * (2 * rng.random((1, T)) - 1))[0]
        ws = Workspace(HipContext.of(circ), batch=1, ncols=circ.dimension)
        ws.upload(BUF_Y, u)
        wide = lambda: ws.cd_minimize(th0, 1, route="wide", fobj_thr=0.0, dtheta_thr=0.0)           # noqa: E731
        f_wide = float(wide()["cost"][0])
        tw = [_timed(wide)[0] for _ in range(args.reps)]
        ws.close()
        print(json.dumps({"measurement": "one sweep, one lane", "shape": name, "num_thetas": T, "reps": args.reps,
                          "launches_per_sweep_wide_walk": T + n + L, "wide": _stats(tw), "objective_wide": f_wide}), flush=True)
    # the wide walk with lanes, 8 qubits
    n, layout, depth = SHAPES["mat8_l24"]
    circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, layout, "full", depth))
    B = args.lanes
    ths = np.pi * (2 * rng.random((B, circ.num_thetas)) - 1)
    ws = Workspace(HipContext.of(circ), batch=B, ncols=circ.dimension)
    ws.upload(BUF_Y, _targets(circ, np.pi * (2 * rng.random((B, circ.num_thetas)) - 1)))
    wide = lambda: ws.cd_minimize(ths, 1, route="wide", fobj_thr=0.0, dtheta_thr=0.0)               # noqa: E731
    wide()
    tw = [_timed(wide)[0] for _ in range(args.reps)]
    ws.close()
    print(json.dumps({"measurement": "one sweep, all lanes", "shape": "mat8_l24", "lanes": B, "reps": args.reps, "wide": _stats(tw)}), flush=True)
    # the rules on the persistent route: the tutorial's 1000 sweeps
    circ = ParametricCircuit(5, "cx", create_ansatz_structure(5, "cyclic_spin", "full", 180))
    th0 = np.pi * (2 * rng.random(circ.num_thetas) - 1)
    u = _targets(circ, np.pi * (2 * rng.random((1, circ.num_thetas)) - 1))[0]
    S = args.tutorial_sweeps
    ws = Workspace(HipContext.of(circ), batch=1, ncols=32)
    ws.upload(BUF_Y, u)
    plain = lambda: coord_descent_sweeps(circ, th0.copy(), u, S)                                    # noqa: E731
    ruled = lambda: ws.cd_minimize(th0, S, chunk=64, fobj_thr=0.0, dtheta_thr=0.0)                  # noqa: E731
    f_plain, r = plain(), ruled()
    tp, tr = [], []
    for _ in range(max(args.reps // 2, 3)):
        tp.append(_timed(plain)[0])
        tr.append(_timed(ruled)[0])
    ws.close()
    print(json.dumps({"measurement": f"{S} sweeps, one lane, persistent route", "shape": "mat5_cyc180", "reps": len(tp),
                      "coord_descent_sweeps": _stats(tp), "driver_chunk64": _stats(tr), "sweeps_run_by_driver": int(r["nit"][0]),
                      "profiles_equal": bool(np.array_equal(f_plain[0], r["profile"][0]))}), flush=True)


if __name__ == "__main__":
    main()
