#!/usr/bin/env python
"""Matrix elements of operators between MPS states on the device (mps_observables.operator_matrix / expectations / variance_by_walk ->
aqc_mps_melem): ms per call.  Not a test: nothing here is a threshold.

Per bond cap (--bonds, default 16, 32, 64) at --qubits (default 32), on seeded random MPS resident on the device (bond dimensions
min(cap, 2^q, 2^(n-q)), N(0, 1) tensors scaled to norm 1), wall time of the call -- uploads of the tables, walks, device synchronise,
download -- median of --reps (default 5) after a warm-up, with min - max, under the fused and the gemm route:
  * "matrix":      the 16 x 16 matrix <v_i|H|v_j> of the open XXZ chain (``operator_matrix``), against the only route there was before:
                   ``pauli_strings(kets, the 3 (n - 1) bond strings, bras=...)`` over the 256 pairs, weighted and summed
  * "expectation": one <psi|H|psi> (``expectations``) against ``energy`` (which walks the supports only and is expected to win)
  * "variance":    ``variance_by_walk`` against ``variance`` (through H psi), at the bond caps of --variance-bonds (default 16)
One JSON line per bond cap."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aqc_research_amd import mps_observables as mo  # noqa: E402
from aqc_research_amd.mps_engine import MPO, DeviceMPS  # noqa: E402

DELTA = 0.7


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
    ap.add_argument("--variance-bonds", type=int, nargs="+", default=[16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--states", type=int, default=16, help="side of the matrix")
    args = ap.parse_args()
    n = args.qubits
    h = MPO.xxz(n, DELTA)
    terms = [(-0.25 * (DELTA if c == "Z" else 1.0), (2 * c, (q, q + 1))) for q in range(n - 1) for c in "XYZ"]
    weights = np.array([t[0] for t in terms])
    strings = mo._strings([t[1] for t in terms], n)
    for cap in args.bonds:
        states = [DeviceMPS.from_qiskit(_random_mps(n, cap, 1000 * k + cap)) for k in range(1, args.states + 1)]
        m = states[0]
        try:
            rec = {"qubits": n, "bond_cap": cap, "max_bond": int(m.bond_dims.max()), "rule": mo.melem_route(None, m.bond_dims, h.bond_dims),
                   "strings": len(terms), "pairs": len(states) ** 2}
            methods = [k for k in ("fused", "gemm") if k == "gemm" or rec["rule"] == "fused"]
            bras = [b for b in states for _ in states]
            kets = [k for _ in states for k in states]

            def by_strings():
                return (mo.pauli_strings(kets, strings, bras=bras) * weights).sum(axis=-1).reshape(len(states), len(states))

            for method in methods:
                rec[f"matrix_{method}"] = _timed(lambda: mo.operator_matrix(h, states, method=method), args.reps)
                rec[f"expectation_{method}"] = _timed(lambda: mo.expectations(m, [h], method=method), args.reps)
            rec["matrix_by_pauli_strings"] = _timed(by_strings, args.reps)
            rec["expectation_by_energy"] = _timed(lambda: mo.energy(m, terms), args.reps)
            mat = mo.operator_matrix(h, states)
            rec["max_abs_matrix_minus_strings"] = float(np.max(np.abs(mat - by_strings())))
            rec["abs_expectation_minus_energy"] = float(abs(mo.expectations(m, [h])[0].real - mo.energy(m, terms)))
            if len(methods) == 2:
                rec["max_abs_fused_minus_gemm"] = float(np.max(np.abs(mo.operator_matrix(h, states, method="fused") - mo.operator_matrix(h, states, method="gemm"))))
            best = min(rec[f"matrix_{k}"]["median_ms"] for k in methods)
            rec["matrix_speedup_over_strings"] = rec["matrix_by_pauli_strings"]["median_ms"] / best
            rec["matrix_ranges_apart"] = max(rec[f"matrix_{k}"]["max_ms"] for k in methods if rec[f"matrix_{k}"]["median_ms"] == best) < rec["matrix_by_pauli_strings"]["min_ms"]
            if cap in args.variance_bonds:
                for method in methods:
                    rec[f"variance_by_walk_{method}"] = _timed(lambda: mo.variance_by_walk(m, h, method=method), args.reps)
                rec["variance"] = _timed(lambda: mo.variance(m, h), args.reps)
                rec["abs_variance_by_walk_minus_variance"] = float(abs(mo.variance_by_walk(m, h) - mo.variance(m, h)))
            print(json.dumps(rec), flush=True)
        finally:
            for s in states:
                s.close()


if __name__ == "__main__":
    main()
