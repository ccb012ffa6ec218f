#!/usr/bin/env python
"""MPS states into dense vectors on the device (mps_engine.to_vectors -> aqc_mps_to_vec): ms per call.
Not a test: nothing here is a threshold.

2nd-order XXZ Trotter states (--layers, default 6, at evolution times 0.6, 0.7, ... one per state) from a Neel state at --qubits
(default 16 20 24), built on the device with mps_engine.v_mul_mps_many at max_bond --bonds (default 16 32 64), trunc_thr 0.  Per size
and cap, for 1 and --states (default 8) states per call: wall time of the call -- the launches, the device synchronise and the
download of the 2^n amplitudes per state -- median of --reps (default 5) after a warm-up, with min - max, on three roads in the same
run:
  fused   to_vectors(states, method="fused")
  gemm    to_vectors(states, method="gemm")
  before  mps_operations.mps_to_vector(s.to_qiskit()) state by state: n site downloads, Python tuples, an upload into a dense
          workspace, its chain of products, a download -- the yardstick
With them the bonds of the first state, max |fused - before| and max |fused - gemm|, and the device time of the outer product of the
fused call (HIP events, aqc_mps_to_vec_outer_ms) with its written bytes over that time as a share of the 6.29 TB/s copy rate.

--blocks adds one call of amplitude_blocks at --block-qubits (default 32), max_bond 32, --block-rows (default 1024) random rows of
high bits and --block-low (default 10) low qubits against mps_sampling.amplitudes on the same rows x 2^low bit strings.
One JSON line per setting."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aqc_research_amd import TrotterAnsatz, _lib  # noqa: E402
from aqc_research_amd import mps_engine as me  # noqa: E402
from aqc_research_amd import mps_operations, mps_sampling  # noqa: E402
from aqc_research_amd.circuit_structures import make_trotter_like_circuit  # noqa: E402
from aqc_research_amd.model_sp_lhs.trotter import init_ansatz_to_trotter, neel_state_index  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s


def _timed(fn, reps, warm=True):
    if warm:
        fn()   # warm-up: code objects, first allocation
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}


def _states(n, layers, cap, count):
    circ = TrotterAnsatz(n, make_trotter_like_circuit(n, layers), second_order=True)
    thetas = np.stack([init_ansatz_to_trotter(circ, np.zeros(circ.num_thetas), evol_time=0.6 + 0.1 * l, delta=1.0) for l in range(count)])
    start = me.DeviceMPS.basis_state(n, neel_state_index(n))
    try:
        return me.v_mul_mps_many(circ, thetas, [start] * count, 0.0, cap)
    finally:
        start.close()


def _close(states):
    for m in states:
        m.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--qubits", type=int, nargs="*", default=[16, 20, 24])
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--bonds", type=int, nargs="+", default=[16, 32, 64])
    ap.add_argument("--states", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", action="store_true")
    ap.add_argument("--block-qubits", type=int, default=32)
    ap.add_argument("--block-rows", type=int, default=1024)
    ap.add_argument("--block-low", type=int, default=10)
    args = ap.parse_args()
    outer_ms = _lib.lib().aqc_mps_to_vec_outer_ms
    for n in args.qubits:
        for cap in args.bonds:
            states = _states(n, args.layers, cap, args.states)
            try:
                rec = {"qubits": n, "layers": args.layers, "max_bond": cap, "bonds": states[0].bond_dims.tolist(), "rule": me.to_vector_route(states[0].bond_dims)}
                for count in sorted({1, args.states}):
                    group = states[:count]
                    out = np.empty((count, 2 ** n), dtype=np.complex128)
                    rec[f"fused_{count}"] = _timed(lambda: me.to_vectors(group, method="fused", out=out), args.reps)
                    outer = []
                    for _ in range(args.reps):
                        me.to_vectors(group, method="fused", out=out)
                        outer.append(outer_ms())
                    ms = statistics.median(outer)
                    rec[f"outer_{count}"] = {"median_ms": ms, "min_ms": min(outer), "max_ms": max(outer),
                                             "share_of_copy_rate": count * 2 ** n * 16 / (1e-3 * ms) / COPY_RATE if ms > 0 else None}
                    rec[f"gemm_{count}"] = _timed(lambda: me.to_vectors(group, method="gemm", out=out), args.reps)
                    rec[f"before_{count}"] = _timed(lambda: [mps_operations.mps_to_vector(s.to_qiskit()) for s in group], args.reps)
                    rec[f"before_over_fused_{count}"] = rec[f"before_{count}"]["median_ms"] / rec[f"fused_{count}"]["median_ms"]
                    rec[f"gemm_over_fused_{count}"] = rec[f"gemm_{count}"]["median_ms"] / rec[f"fused_{count}"]["median_ms"]
                fused = me.to_vectors(states[0], method="fused")
                rec["fused_minus_before"] = float(np.max(np.abs(fused - mps_operations.mps_to_vector(states[0].to_qiskit()))))
                rec["fused_minus_gemm"] = float(np.max(np.abs(fused - me.to_vectors(states[0], method="gemm"))))
                rec["norm"] = float(np.linalg.norm(fused))
                print(json.dumps(rec), flush=True)
            finally:
                _close(states)
    if args.blocks:
        n, k, rows = args.block_qubits, args.block_low, args.block_rows
        states = _states(n, args.layers, 32, 1)
        try:
            rng = np.random.default_rng(32)
            high = rng.integers(0, 2, size=(rows, n - k)).astype(np.uint8)
            low = ((np.arange(2 ** k)[:, None] >> np.arange(k)[None, :]) & 1).astype(np.uint8)
            strings = np.ascontiguousarray(np.concatenate([np.broadcast_to(low[None], (rows, 2 ** k, k)), np.broadcast_to(high[:, None], (rows, 2 ** k, n - k))],
                                                          axis=2).reshape(rows * 2 ** k, n))
            rec = {"qubits": n, "max_bond": 32, "bonds": states[0].bond_dims.tolist(), "rows": rows, "low_qubits": k}
            rec["blocks"] = _timed(lambda: me.amplitude_blocks(states[0], k, high), args.reps)
            rec["blocks_outer_ms"] = outer_ms()
            rec["amplitudes"] = _timed(lambda: mps_sampling.amplitudes(states[0], strings), args.reps)
            rec["amplitudes_over_blocks"] = rec["amplitudes"]["median_ms"] / rec["blocks"]["median_ms"]
            got, want = me.amplitude_blocks(states[0], k, high), mps_sampling.amplitudes(states[0], strings).reshape(rows, 2 ** k)
            rec["blocks_minus_amplitudes"] = float(np.max(np.abs(got - want)))
            rec["largest_row_norm"] = float(np.max(np.linalg.norm(want, axis=1)))
            print(json.dumps(rec), flush=True)
        finally:
            _close(states)


if __name__ == "__main__":
    main()
