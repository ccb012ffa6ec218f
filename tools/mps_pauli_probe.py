#!/usr/bin/env python
"""Pauli strings between MPS states on the device (mps_observables.pauli_strings / overlaps -> aqc_mps_pauli): ms per call.
Not a test: nothing here is a threshold.

Per bond cap (--bonds, default 16, 32, 64) at --qubits (default 32), on seeded random MPS resident on the device (bond dimensions
min(cap, 2^q, 2^(n-q)), N(0, 1) tensors scaled to norm 1), wall time of the call -- environments, walks, device synchronise, download
-- median of --reps (default 5) after a warm-up, with min - max, under the fused and the gemm route:
  * "zz":       the n (n - 1) / 2 strings Z_i Z_j, against pair_density_matrices of all pairs and against one
                ``DeviceMPS.dot_ops(self, self, [(i, Z), (j, Z)])`` per string (what could be done before; --baseline-reps, default 2)
  * "xxz":      the (n - 1) x 3 bond terms XX, YY, ZZ of the open XXZ chain
  * "random":   1024 random strings of full weight
  * "overlaps": a 16 x 16 matrix <phi_a|psi_b>, against 256 ``DeviceMPS.dot`` calls
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
from aqc_research_amd.mps_engine import DeviceMPS  # noqa: E402

_Z = np.diag([1.0, -1.0]).astype(np.complex128)


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--baseline-reps", type=int, default=2)
    ap.add_argument("--states", type=int, default=16, help="side of the overlap matrix")
    args = ap.parse_args()
    n = args.qubits
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    lists = {
        "zz": mo._strings([("ZZ", p) for p in pairs], n),
        "xxz": mo._strings([(2 * c, (q, q + 1)) for q in range(n - 1) for c in "XYZ"], n),
        "random": np.random.default_rng(7).integers(1, 4, size=(1024, n)).astype(np.uint8),
    }
    for cap in args.bonds:
        states = [DeviceMPS.from_qiskit(_random_mps(n, cap, 1000 * k + cap)) for k in range(1, args.states + 1)]
        m = states[0]
        try:
            rec = {"qubits": n, "bond_cap": cap, "max_bond": int(m.bond_dims.max()), "rule": mo.pauli_route(None, m.bond_dims)}
            methods = [k for k in ("fused", "gemm") if k == "gemm" or rec["max_bond"] <= mo.FUSED_CAP]
            for name, strings in lists.items():
                for method in methods:
                    rec[f"{name}_{method}"] = dict(_timed(lambda: mo.pauli_strings(m, strings, method=method), args.reps), strings=len(strings))
            for method in methods:
                rec[f"overlaps_{method}"] = dict(_timed(lambda: mo.overlaps(states, states, method=method), args.reps), pairs=len(states) ** 2)
            if len(methods) == 2:
                rec["max_abs_fused_minus_gemm"] = max(
                    float(np.max(np.abs(mo.pauli_strings(m, s, method="fused") - mo.pauli_strings(m, s, method="gemm")))) for s in lists.values())
            rec["zz_by_pair_density_matrices"] = dict(_timed(lambda: mo.pair_density_matrices(m, pairs), args.reps), pairs=len(pairs))

            def zz_by_dot_ops():
                return [m.dot_ops(m, [(i, _Z), (j, _Z)]) for i, j in pairs]

            def gram_by_dot():
                return [[a.dot(b) for b in states] for a in states]

            if args.baseline_reps > 0:
                rec["zz_by_dot_ops"] = dict(_timed(zz_by_dot_ops, args.baseline_reps), calls=len(pairs))
                rec["overlaps_by_dot"] = dict(_timed(gram_by_dot, args.baseline_reps), calls=len(states) ** 2)
                zz = mo.pauli_strings(m, lists["zz"])
                rec["max_abs_zz_minus_dot_ops"] = float(np.max(np.abs(zz - np.array(zz_by_dot_ops()))))
                rec["max_abs_overlaps_minus_dot"] = float(np.max(np.abs(mo.overlaps(states, states) - np.array(gram_by_dot()))))
                rec["zz_speedup_over_dot_ops"] = rec["zz_by_dot_ops"]["median_ms"] / rec[f"zz_{rec['rule']}"]["median_ms"]
            print(json.dumps(rec), flush=True)
        finally:
            for s in states:
                s.close()


if __name__ == "__main__":
    main()
