#!/usr/bin/env python
"""Measurement of MPS states on the device (mps_sampling.sample / amplitudes -> aqc_mps_sample / aqc_mps_amplitudes): ms per call.
Not a test: nothing here is a threshold.

Per bond cap (--bonds, default 16, 32, 64) at --qubits (default 32), on a seeded random MPS resident on the device (bond dimensions
min(cap, 2^q, 2^(n-q)), N(0, 1) tensors scaled to norm 1), wall time of the call -- environments, walk, device synchronise, download of
the bits -- median of --reps (default 5) after a warm-up, with min - max:
  * ``sample`` at --shots (default 2^10, 2^14, 2^18), under the fused and the gemm route;
  * ``amplitudes`` of --strings (default 2^14) sampled bit strings, under both routes.
The baseline is what could be done before for one amplitude: ``DeviceMPS.basis_state(n, index)`` plus one ``dot`` (a chain of launches
and a stream synchronisation per bit string), timed over --baseline-strings (default 64) strings and reported per string.  One JSON line
per bond cap."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aqc_research_amd import mps_sampling as ms  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--qubits", type=int, default=32)
    ap.add_argument("--bonds", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--shots", type=int, nargs="+", default=[1 << 10, 1 << 14, 1 << 18])
    ap.add_argument("--strings", type=int, default=1 << 14)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-strings", type=int, default=64)
    args = ap.parse_args()
    n = args.qubits
    for cap in args.bonds:
        m = DeviceMPS.from_qiskit(_random_mps(n, cap, 2000 + cap))
        try:
            rec = {"qubits": n, "bond_cap": cap, "max_bond": int(m.bond_dims.max()), "rule": ms.route(m.bond_dims)}
            methods = [k for k in ("fused", "gemm") if k == "gemm" or rec["max_bond"] <= ms.FUSED_CAP]
            for shots in args.shots:
                for method in methods:
                    rec[f"sample_{shots}_{method}"] = _timed(lambda: ms.sample(m, shots, seed=1, method=method), args.reps)
            strings = ms.sample(m, args.strings, seed=2)
            for method in methods:
                rec[f"amplitudes_{args.strings}_{method}"] = _timed(lambda: ms.amplitudes(m, strings, method=method), args.reps)
            if len(methods) == 2:
                a, b = (ms.sample(m, args.shots[0], seed=1, method=k, details=True) for k in methods)
                rec["bits_equal_fused_gemm"] = bool(np.array_equal(a["bits"], b["bits"]))
                rec["max_abs_amplitude_fused_minus_gemm"] = float(np.max(np.abs(a["amplitudes"] - b["amplitudes"])))

            def one_by_one():
                out = []
                for row in strings[:args.baseline_strings]:
                    index = sum(int(b) << q for q, b in enumerate(row))
                    basis = DeviceMPS.basis_state(n, index)
                    try:
                        out.append(basis.dot(m))
                    finally:
                        basis.close()
                return np.array(out)

            if args.baseline_strings > 0:
                t = _timed(one_by_one, 1)
                rec["basis_state_dot_ms_per_string"] = t["median_ms"] / min(args.baseline_strings, len(strings))
                got = ms.amplitudes(m, strings[:args.baseline_strings])
                rec["max_abs_amplitude_minus_dot"] = float(np.max(np.abs(got - one_by_one())))
            print(json.dumps(rec), flush=True)
        finally:
            m.close()


if __name__ == "__main__":
    main()
