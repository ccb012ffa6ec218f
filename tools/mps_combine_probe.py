#!/usr/bin/env python
"""Linear combinations of MPS states on the device (mps_engine.linear_combinations -> aqc_mps_combine): ms per call.
Not a test: nothing here is a threshold.

Per configuration "KxB" (--configs, default 2x16 2x32 4x16: sums of K states of bond cap B, summed bond K B) at --qubits (default 32),
on seeded random MPS resident on the device (bond dimensions min(B, 2^q, 2^(n-q)), N(0, 1) tensors scaled to norm 1, not canonical),
for 1 output and for --outputs (default 16) outputs per call (rows of a seeded complex coefficient matrix over the same K states), at
trunc_thr = 0 and at --trunc-thr (default 1e-6): wall time of the call -- assembly of the direct sums, right factors, the sweep of
form / SVD / split launches, device synchronise, one new state per output -- median of --reps (default 5) after a warm-up, with
min - max, against what could be done before, measured in the same run on the same states, one output at a time: ``to_qiskit()`` of
the terms, the direct sum in NumPy, ``compress`` of that tuple (--baseline-reps, default 5; 0 leaves it out).  With them the bonds
left and the largest difference of the bond vectors between the call and the host loop.  One JSON line per configuration.

The split of a call into its launches is read from a kernel trace of a run of its own (--reps 1 --baseline-reps 0 --fused-only)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aqc_research_amd import mps_engine as me  # noqa: E402
from aqc_research_amd.mps_engine import DeviceMPS  # noqa: E402


def _random_mps(n, cap, seed):
    rng = np.random.default_rng(seed)
    dims = [min(cap, 2 ** min(q, n - q, 30)) for q in range(n + 1)]
    ts, left = [], np.ones((1, 1), dtype=np.complex128)
    for q in range(n):   # scaled site by site so that no partial product over- or underflows
        t = rng.standard_normal((2, dims[q], dims[q + 1])) + 1j * rng.standard_normal((2, dims[q], dims[q + 1]))
        left = np.einsum("cxu,xy,cyv->uv", t.conj(), left, t, optimize=True)
        s = np.sqrt(np.trace(left).real)
        ts.append(t / s)
        left = left / (s * s)
    return [(t[0], t[1]) for t in ts], [np.ones(dims[q + 1]) for q in range(n - 1)]


def _timed(fn, reps):
    fn()   # warm-up: code objects, first allocation
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}


def _direct_sum(tuples, coeffs):
    """The direct sum of the terms as a QiskitMPS tuple with unit bond vectors (the exported sites are Gamma lambda: taken whole)."""
    n = len(tuples[0][0])
    sites = [[np.stack([g0, g1]) * (np.asarray(lam[q]) if q < n - 1 else 1.0) for q, (g0, g1) in enumerate(gam)] for gam, lam in tuples]
    gam = []
    for q in range(n):
        rows = sum(t[q].shape[1] for t in sites) if q > 0 else 1
        cols = sum(t[q].shape[2] for t in sites) if q < n - 1 else 1
        site = np.zeros((2, rows, cols), dtype=np.complex128)
        r0 = c0 = 0
        for k, t in enumerate(sites):
            block = coeffs[k] * t[q] if q == 0 else t[q]
            site[:, r0:r0 + block.shape[1], c0:c0 + block.shape[2]] = block
            r0 += block.shape[1] if q > 0 else 0
            c0 += block.shape[2] if q < n - 1 else 0
        gam.append((site[0], site[1]))
    return gam, [np.ones(g[0].shape[1]) for g in gam[:-1]]


def _host_loop(states, matrix, thr, keep=False):
    """What a caller had before, one output at a time: download the terms, the direct sum in NumPy, compress of the tuple."""
    out = []
    for row in matrix:
        made = me.compress(_direct_sum([m.to_qiskit() for m in states], row), thr)
        if keep:
            out.append(made)
        else:
            made.close()
    return out


def _call(states, matrix, thr, method):
    for m in me.linear_combinations(states, matrix, thr, method=method):
        m.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--qubits", type=int, default=32)
    ap.add_argument("--configs", nargs="+", default=["2x16", "2x32", "4x16"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-reps", type=int, default=5)
    ap.add_argument("--outputs", type=int, default=16)
    ap.add_argument("--trunc-thr", type=float, default=1e-6)
    ap.add_argument("--fused-only", action="store_true", help="only the call on all outputs at trunc_thr = 0 (for a kernel trace)")
    args = ap.parse_args()
    n = args.qubits
    for config in args.configs:
        terms, cap = (int(x) for x in config.split("x"))
        states = [DeviceMPS.from_qiskit(_random_mps(n, cap, 1000 * k + cap), assume_canonical=True) for k in range(1, terms + 1)]
        rng = np.random.default_rng(7 * terms + cap)
        matrix = rng.standard_normal((args.outputs, terms)) + 1j * rng.standard_normal((args.outputs, terms))
        try:
            dims = np.stack([m.bond_dims for m in states])
            rec = {"qubits": n, "terms": terms, "bond_cap": cap, "summed_bond": int(dims.sum(axis=0)[1:n].max()), "rule": me.combine_route(dims),
                   "outputs": args.outputs}
            for thr in ((0.0,) if args.fused_only else (0.0, args.trunc_thr)):
                tag = "exact" if thr == 0.0 else "trunc"
                for count in sorted({args.outputs} if args.fused_only else {1, args.outputs}):
                    rows = matrix[:count]
                    rec[f"{tag}_call_{count}"] = _timed(lambda: _call(states, rows, thr, None), args.reps)
                    if args.baseline_reps > 0 and not args.fused_only:
                        rec[f"{tag}_host_loop_{count}"] = _timed(lambda: _host_loop(states, rows, thr), args.baseline_reps)
                        rec[f"{tag}_host_loop_over_call_{count}"] = rec[f"{tag}_host_loop_{count}"]["median_ms"] / rec[f"{tag}_call_{count}"]["median_ms"]
                if not args.fused_only:
                    made, info = me.linear_combinations(states, matrix, thr, details=True)
                    ref = _host_loop(states, matrix, thr, keep=True)
                    try:
                        rec[f"{tag}_svd_sweeps"] = {"min": int(info["sweeps"].min()), "median": float(np.median(info["sweeps"])), "max": int(info["sweeps"].max())}
                        rec[f"{tag}_max_bond_left"] = int(max(int(m.bond_dims.max()) for m in made))
                        rec[f"{tag}_bonds_equal_host_loop"] = all(a.bond_dims.tolist() == b.bond_dims.tolist() for a, b in zip(made, ref))
                        if rec[f"{tag}_bonds_equal_host_loop"]:
                            rec[f"{tag}_max_abs_lambda_call_minus_host_loop"] = float(max(
                                np.max(np.abs(x - y)) for a, b in zip(made, ref) for x, y in zip(a.to_qiskit()[1], b.to_qiskit()[1])))
                    finally:
                        for m in made + ref:
                            m.close()
            print(json.dumps(rec), flush=True)
        finally:
            for s in states:
                s.close()


if __name__ == "__main__":
    main()
