"""Rate of the batched block-Jacobi SVD (aqc_svd_batch) against a loop of svd() over the same matrices: batches of 256 square matrices
at 64, 128 and 256, Haar vectors with a flat and with the ``graded`` spectrum (1 .. 1e-12).  Not a test and not part of bench.py.

Per size and spectrum, after one warm-up call, the median of ``--repeats`` calls of
  core   the device core alone (HIP events around the zeroing of the outputs and the kernel: aqc_svd_batch_core_ms),
  call   svd_batch() end to end on host arrays (allocations, uploads, downloads included); call - core is what the copies cost,
  loop   svd() on each of the first ``--loop`` matrices, one after the other, scaled to the batch (svd() also works from host arrays).
Flops are counted from the code, not measured: a sweep forms the Gram matrix of every block pair (9 ceil(rows / 4) MFMAs) and, where
the pair has not converged, applies J to W and V (48 MFMAs per 16-row tile), 2048 flop per v_mfma_f64_16x16x4_f64.  The kernel
reports sweeps, not rotated pairs, so ``Gram`` is exact and ``all`` (every pair rotated in every sweep) an upper bound; the share of
the 78.6 TFLOP/s matrix peak is given for both.

    python tools/svd_batch_probe.py [--sizes 64,128,256] [--count 256] [--repeats 5] [--loop 16]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from aqc_research_amd import _lib
from aqc_research_amd.mps_engine import svd, svd_batch

PEAK_TFLOPS, MFMA_FLOP, BLOCK = 78.6, 16 * 16 * 4 * 2, 16


def haar(n, rng):
    q, r = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def batch(n, count, spectrum, rng):
    s = np.ones(n) if spectrum == "flat" else np.geomspace(1.0, 1e-12, n)
    return np.stack([(haar(n, rng) * s) @ np.conj(haar(n, rng).T) for _ in range(count)])


def mfmas_per_sweep(n):
    """(Gram, Gram + J products on every pair) for an n x n matrix"""
    nb = (n + BLOCK - 1) // BLOCK
    pairs = nb * (nb - 1) // 2 + (nb if nb % 2 else 0)      # with an odd count every block also plays alone once per sweep
    pairs = max(pairs, 1)
    gram = pairs * 9 * ((n + 3) // 4)
    return gram, gram + pairs * 48 * 2 * ((n + 15) // 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,128,256")
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop", type=int, default=16)
    args = ap.parse_args()
    core_ms = _lib.lib().aqc_svd_batch_core_ms
    for n in [int(v) for v in args.sizes.split(",")]:
        for spectrum in ("flat", "graded"):
            a = batch(n, args.count, spectrum, np.random.default_rng(n + (spectrum == "graded")))
            svd_batch(a)                                                         # warm-up
            core, call = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                u, s, vh, sweeps, status = svd_batch(a)
                call.append((time.perf_counter() - t0) * 1e3)
                core.append(core_ms())
            nl = min(args.loop, args.count)
            svd(a[0])
            loop, loop_sweeps = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                loop_sweeps = [svd(a[i])[3] for i in range(nl)]
                loop.append((time.perf_counter() - t0) * 1e3 * args.count / nl)
            core_m, call_m, loop_m = statistics.median(core), statistics.median(call), statistics.median(loop)
            err = max(float(np.abs((u[i] * s[i]) @ vh[i] - a[i]).max()) for i in range(0, args.count, max(args.count // 8, 1)))
            gram, full = mfmas_per_sweep(n)
            tot = float(np.sum(sweeps))
            tf_gram, tf_all = gram * tot * MFMA_FLOP / (core_m * 1e-3) / 1e12, full * tot * MFMA_FLOP / (core_m * 1e-3) / 1e12
            print(f"{args.count} x {n} x {n} {spectrum}: status {sorted(set(int(v) for v in status))}, sweeps {int(sweeps.min())}..{int(sweeps.max())} "
                  f"(svd(): {min(loop_sweeps)}..{max(loop_sweeps)}), max |A - U S Vh| {err:.1e}\n"
                  f"    core {core_m:9.2f} ms ({min(core):.2f} .. {max(core):.2f})  = {args.count / core_m * 1e3:10.0f} SVDs/s\n"
                  f"    call {call_m:9.2f} ms ({min(call):.2f} .. {max(call):.2f})  = {args.count / call_m * 1e3:10.0f} SVDs/s; copies and allocations {call_m - core_m:.2f} ms\n"
                  f"    loop {loop_m:9.2f} ms ({min(loop):.2f} .. {max(loop):.2f})  = {args.count / loop_m * 1e3:10.0f} SVDs/s  (svd() on {nl} matrices, scaled)\n"
                  f"    call / loop speed-up {loop_m / call_m:.2f}, core / loop {loop_m / core_m:.2f}\n"
                  f"    fp64 matrix flops: Gram {gram * tot * MFMA_FLOP:.3e} ({tf_gram:.2f} TFLOP/s, {tf_gram / PEAK_TFLOPS:.4f} of peak), "
                  f"all pairs rotated {full * tot * MFMA_FLOP:.3e} (<= {tf_all:.2f} TFLOP/s, {tf_all / PEAK_TFLOPS:.4f} of peak)", flush=True)


if __name__ == "__main__":
    main()
