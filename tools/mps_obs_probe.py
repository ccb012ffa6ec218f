#!/usr/bin/env python
"""Pair density matrices of MPS states on the device (mps_observables.pair_density_matrices -> aqc_mps_obs_pairs): ms per call.
Not a test: nothing here is a threshold.

Per bond cap (--bonds, default 16, 32, 64) at --qubits (default 32), on a seeded random MPS resident on the device (bond dimensions
min(cap, 2^q, 2^(n-q)), N(0, 1) tensors scaled to norm 1), wall time of the call -- environments, chains, device synchronise, download
of the sums -- median of --reps (default 5) after a warm-up, with min - max:
  * "nearest":  the n - 1 nearest-neighbour pairs        * "all":  all n (n - 1) / 2 pairs
each under the fused and the gemm route.  The baseline is what could be done before: the ZZ correlation matrix through one
``DeviceMPS.dot_ops(self, self, [(i, Z), (j, Z)])`` per pair (a chain of launches and a stream synchronisation each), timed once per
--baseline-reps (default 2); it yields one number per pair where a pair density matrix yields sixteen.  One JSON line per bond cap."""
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
    args = ap.parse_args()
    n = args.qubits
    lists = {"nearest": [(q, q + 1) for q in range(n - 1)], "all": [(i, j) for i in range(n) for j in range(i + 1, n)]}
    for cap in args.bonds:
        m = DeviceMPS.from_qiskit(_random_mps(n, cap, 1000 + cap))
        try:
            rec = {"qubits": n, "bond_cap": cap, "max_bond": int(m.bond_dims.max()), "rule": mo.route(m.bond_dims)}
            for name, pairs in lists.items():
                for method in ("fused", "gemm"):
                    if method == "fused" and rec["max_bond"] > mo.FUSED_CAP:
                        continue
                    rec[f"{name}_{method}"] = dict(_timed(lambda: mo.pair_density_matrices(m, pairs, method=method), args.reps), pairs=len(pairs))
            if "all_fused" in rec:
                a, b = mo.pair_density_matrices(m, lists["all"], method="fused"), mo.pair_density_matrices(m, lists["all"], method="gemm")
                rec["max_abs_fused_minus_gemm"] = float(np.max(np.abs(a - b)))

            def zz_by_dot_ops():
                return [m.dot_ops(m, [(i, _Z), (j, _Z)]) for i, j in lists["all"]]

            if args.baseline_reps > 0:
                rec["zz_matrix_by_dot_ops"] = dict(_timed(zz_by_dot_ops, args.baseline_reps), calls=len(lists["all"]))
                zz = np.array(zz_by_dot_ops()).real
                rho = mo.pair_density_matrices(m, lists["all"])
                rec["max_abs_zz_difference"] = float(np.max(np.abs(mo.pauli_expectation(rho, "zz") - zz)))
            print(json.dumps(rec), flush=True)
        finally:
            m.close()


if __name__ == "__main__":
    main()
