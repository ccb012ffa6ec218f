#!/usr/bin/env python
"""Dense vectors into MPS states on the device (mps_engine.from_vectors -> aqc_mps_from_vec): ms per call.
Not a test: nothing here is a threshold.

2nd-order XXZ Trotter states (--layers, default 3, at evolution times 0.6, 0.7, ... one per vector, so the spectra decay) from a Neel
state at --qubits (default 16 20 24), built with the dense stage kernels (core_operations.v_mul_vec).  Per size, bond cap (--bonds,
default 16 32), threshold (--thresholds, default 0 1e-6) and for 1 and --vectors (default 8) vectors per call: wall time of the call --
upload of the vectors, per site the partial-factor / tree / SVD / split / projection launches, device synchronise, one new state per
lane -- median of --reps (default 5) after a warm-up, with min - max, on the fused route, against what could be done before, measured
in the same run on the same vectors: the host route (mps_operations.vector_to_canonical_mps, a loop of LAPACK SVDs, and an upload),
vector by vector (--host-reps, default 1, warmed up at 16 qubits only; 0 leaves it out; sizes above --host-max, default 24, skip it, sizes
above --host-many-max, default 20, run it on 1 vector only).
With them the bonds left, the sweeps of the SVDs, the partial factors per site, whether the bonds equal the host route's and the
overlap of the two results.  One JSON line per setting.

The split of a fused call into its kernels is read from a kernel trace of a run of its own (--reps 1 --host-reps 0 --fused-only)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aqc_research_amd import TrotterAnsatz  # noqa: E402
from aqc_research_amd import mps_engine as me  # noqa: E402
from aqc_research_amd.circuit_structures import make_trotter_like_circuit  # noqa: E402
from aqc_research_amd.core_operations import v_mul_vec  # noqa: E402
from aqc_research_amd.model_sp_lhs.trotter import init_ansatz_to_trotter, neel_state_index  # noqa: E402


def _timed(fn, reps, warm=True):
    if warm:
        fn()   # warm-up: code objects, first allocation
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}


def _states(n, layers, count):
    circ = TrotterAnsatz(n, make_trotter_like_circuit(n, layers), second_order=True)
    start = np.zeros(2 ** n, dtype=np.complex128)
    start[neel_state_index(n)] = 1.0
    out = np.empty((count, 2 ** n), dtype=np.complex128)
    for l in range(count):
        th = init_ansatz_to_trotter(circ, np.zeros(circ.num_thetas), evol_time=0.6 + 0.1 * l, delta=1.0)
        v_mul_vec(circ, th, start, out[l])
    return out


def _call(vecs, thr, cap, method):
    made = me.from_vectors(vecs, thr, cap, method=method)
    for m in made if isinstance(made, list) else [made]:
        m.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--qubits", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--bonds", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--thresholds", type=float, nargs="+", default=[0.0, 1e-6])
    ap.add_argument("--vectors", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--host-max", type=int, default=24)
    ap.add_argument("--host-many-max", type=int, default=20, help="above this size the host route runs on 1 vector only")
    ap.add_argument("--fused-only", action="store_true", help="only the fused call on all vectors (for a kernel trace)")
    args = ap.parse_args()
    for n in args.qubits:
        vecs = _states(n, args.layers, args.vectors)
        for cap in args.bonds:
            for thr in args.thresholds:
                rec = {"qubits": n, "layers": args.layers, "max_bond": cap, "trunc_thr": thr, "vectors": args.vectors, "rule": me.from_vector_route(n, cap)}
                for count in sorted({args.vectors} if args.fused_only else {1, args.vectors}):
                    group = vecs[0] if count == 1 else vecs[:count]
                    rec[f"fused_{count}"] = _timed(lambda: _call(group, thr, cap, "fused"), args.reps)
                    if args.host_reps > 0 and not args.fused_only and n <= (args.host_max if count == 1 else args.host_many_max):
                        rec[f"host_{count}"] = _timed(lambda: _call(group, thr, cap, "host"), args.host_reps, warm=n <= 16)
                        rec[f"host_over_fused_{count}"] = rec[f"host_{count}"]["median_ms"] / rec[f"fused_{count}"]["median_ms"]
                if not args.fused_only:
                    made, info = me.from_vectors(vecs, thr, cap, method="fused", details=True)
                    try:
                        rec["bonds_left"] = info["bonds"][0].tolist()
                        rec["parts"] = info["parts"].tolist()
                        rec["svd_sweeps"] = {"min": int(info["sweeps"].min()), "median": float(np.median(info["sweeps"])), "max": int(info["sweeps"].max())}
                        rec["dropped"] = float(info["dropped"][0].sum())
                        rec["norm_error"] = abs(float(np.sqrt(abs(made[0].dot(made[0])))) - float(np.linalg.norm(vecs[0])))
                        if args.host_reps > 0 and n <= args.host_max:
                            host = me.from_vectors(vecs[0], thr, cap, method="host")
                            rec["bonds_equal_host"] = made[0].bond_dims.tolist() == host.bond_dims.tolist()
                            rec["abs_overlap_with_host"] = float(abs(made[0].dot(host)))
                            host.close()
                    finally:
                        for m in made:
                            m.close()
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
