#!/usr/bin/env python
"""Schmidt spectra of MPS states on the device (mps_observables.schmidt_values -> aqc_mps_ent_schmidt): ms per call.
Not a test: nothing here is a threshold.

Per bond cap (--bonds, default 16, 32, 64) at --qubits (default 32), on seeded random MPS resident on the device (bond dimensions
min(cap, 2^q, 2^(n-q)), N(0, 1) tensors scaled to norm 1), for 1 state and for --states (default 16) states per call: wall time of the
call -- QR chains, cut products, batched SVD, device synchronise, download -- median of --reps (default 5) after a warm-up, with
min - max, under the fused and the canonical route, against what could be done before, measured in the same run: one
``clone().canonicalize().to_qiskit()`` per state (--baseline-reps, default 5; 0 leaves it out).  With them the sweeps of the cut SVDs
and the largest difference between the routes.  One JSON line per bond cap.

The split of a fused call into its launches is read from a kernel trace of a run of its own (--reps 1 --baseline-reps 0 --fused-only)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aqc_research_amd import mps_observables as mo  # noqa: E402
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


def _by_canonicalize(states):
    """The loop a caller had before: the bond vectors of a canonicalised clone, one state at a time."""
    out = []
    for m in states:
        c = m.clone()
        try:
            out.append(c.canonicalize().to_qiskit()[1])
        finally:
            c.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--qubits", type=int, default=32)
    ap.add_argument("--bonds", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-reps", type=int, default=5)
    ap.add_argument("--states", type=int, default=16)
    ap.add_argument("--fused-only", action="store_true", help="only the fused call on all states (for a kernel trace)")
    args = ap.parse_args()
    n = args.qubits
    for cap in args.bonds:
        states = [DeviceMPS.from_qiskit(_random_mps(n, cap, 1000 * k + cap)) for k in range(1, args.states + 1)]
        try:
            rec = {"qubits": n, "bond_cap": cap, "max_bond": int(states[0].bond_dims.max()), "rule": mo.entanglement_route(states[0].bond_dims),
                   "states": len(states)}
            methods = [k for k in ("fused", "canonical") if k == "canonical" or rec["max_bond"] <= mo.FUSED_CAP]
            if args.fused_only:
                methods = methods[:1]
            for count in sorted({len(states)} if args.fused_only else {1, len(states)}):
                group = states[:count]
                for method in methods:
                    rec[f"{method}_{count}"] = _timed(lambda: mo.schmidt_values(group, method=method), args.reps)
                if args.baseline_reps > 0 and not args.fused_only:
                    rec[f"loop_{count}"] = _timed(lambda: _by_canonicalize(group), args.baseline_reps)
                    if "fused" in methods:
                        rec[f"loop_over_fused_{count}"] = rec[f"loop_{count}"]["median_ms"] / rec[f"fused_{count}"]["median_ms"]
            if "fused" in methods:
                vals, info = mo.schmidt_values(states, method="fused", details=True)
                rec["svd_sweeps"] = {"min": int(info["sweeps"].min()), "median": float(np.median(info["sweeps"])), "max": int(info["sweeps"].max())}
                if "canonical" in methods:
                    rec["max_abs_fused_minus_canonical"] = float(np.max(np.abs(vals - mo.schmidt_values(states, method="canonical"))))
            print(json.dumps(rec), flush=True)
        finally:
            for s in states:
                s.close()


if __name__ == "__main__":
    main()
