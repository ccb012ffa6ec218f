#!/usr/bin/env python
"""Exact XXZ evolution on the device (xxz.xxz_evolve -> aqc_xxz_evolve): what a call costs, what a term of the series costs, and
how good the x10 Trotter "ground truth" of the time-evolution driver is.  Not a test: nothing here is a threshold.

Per shape (--qubits, default 16, 20, 24), from the Neel state at delta = 1:
  * one lane, each of the eight horizon times 1.2 .. 9.6 in a call of its own: wall time of the call (it ends in a device
    synchronise and the download), median of --reps after a warm-up, with min - max; the series length K;
  * the cost of a term from the slope of call time over K across those eight calls (upload, download and allocation do not depend
    on K, so they are the intercept and drop out), and the rate of the byte model at that cost;
  * eight lanes, the eight horizons from one shared state in one call, and the same with all times halved: again the slope;
  * upload and download on their own: a host-to-device and a device-to-host copy of the same bytes from pageable memory (hipMemcpy, as the entry points do it);
  * the time trotter_state takes for the x10 ground truth (steps = 10 x 3 x horizon) of the same horizons.
Byte model of one term, per amplitude: 16 B each for cur, prev, next, and out read + written = 80 B that must move ("streamed");
on top the kernel re-reads cur from partner tiles, on average 1/2 + (n - 12) / 2 times for n > 11 ("issued" = streamed + those).
Then fidelity(t1_gt by Trotter x10, exact) per horizon at --fidelity-qubits (default 12, 16, 20).  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aqc_research_amd import _lib  # noqa: E402
from aqc_research_amd.model_sp_lhs.time_evol import fidelity, precise_multiplier  # noqa: E402
from aqc_research_amd.model_sp_lhs.trotter import neel_state_index, trotter_state  # noqa: E402
from aqc_research_amd.xxz import xxz_evolve  # noqa: E402

HORIZONS = np.round(1.2 * np.arange(1, 9), 3)
STEPS_PER_HORIZON = 3
TILE_BITS = 11


def _stats(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}


def _timed(fn, reps):
    fn()   # warm-up: code objects, first allocation
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return ts, out


def _bytes_per_term(n, lanes):
    streamed = 80.0 * lanes * 2.0**n
    rereads = 16.0 * lanes * 2.0**n * (0.5 + 0.5 * (n - TILE_BITS - 1)) if n > TILE_BITS else 0.0
    return streamed, streamed + rereads


def _hip_runtime():
    """The HIP runtime the library itself is linked against, already loaded into this process."""
    import ctypes

    _lib.lib()
    with open("/proc/self/maps") as maps:
        paths = {line.split()[-1] for line in maps if "libamdhip64" in line}
    if not paths:
        raise RuntimeError("libamdhip64 is not loaded")
    return ctypes.CDLL(sorted(paths)[0])


def _copies(nbytes, reps):
    """hipMemcpy of nbytes from and to pageable host memory (a NumPy array), as the one-shot entry points do it."""
    import ctypes

    hip = _hip_runtime()
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    host = np.zeros(nbytes // 8, dtype=np.float64)
    dev = ctypes.c_void_p()
    if hip.hipMalloc(ctypes.byref(dev), nbytes) != 0:
        raise RuntimeError("hipMalloc failed")

    def copy(kind):   # 1: host to device, 2: device to host; hipMemcpy returns when the copy is done
        a, b = (dev, host.ctypes.data) if kind == 1 else (host.ctypes.data, dev)
        if hip.hipMemcpy(a, b, nbytes, kind) != 0:
            raise RuntimeError("hipMemcpy failed")

    try:
        return _stats(_timed(lambda: copy(1), reps)[0]), _stats(_timed(lambda: copy(2), reps)[0])
    finally:
        hip.hipFree(dev)


def _neel(n):
    v = np.zeros(2**n, dtype=np.complex128)
    v[neel_state_index(n)] = 1
    return v


def _emit(**rec):
    print(json.dumps(rec), flush=True)


def _term_rates(n, lanes, ms_per_term):
    streamed, issued = _bytes_per_term(n, lanes)
    return {"ms_per_term": ms_per_term, "streamed_TBps": streamed / (ms_per_term * 1e-3) / 1e12, "issued_TBps": issued / (ms_per_term * 1e-3) / 1e12}


def probe_shape(n, reps):
    ini = _neel(n)
    ks, ms = [], []
    for t in HORIZONS:
        ts, (_, info) = _timed(lambda: xxz_evolve(ini, 1.0, float(t), details=True), reps)
        k = int(info["terms"][0])
        ks.append(k)
        ms.append(1e3 * statistics.median(ts))
        _emit(what="evolve", qubits=n, lanes=1, time=float(t), terms=k, **_stats(ts))
    slope, intercept = np.polyfit(ks, ms, 1)
    _emit(what="per_term", qubits=n, lanes=1, fit="call ms over K, eight horizons", intercept_ms=float(intercept), **_term_rates(n, 1, float(slope)))
    ts_full, (_, info_full) = _timed(lambda: xxz_evolve(ini, 1.0, HORIZONS, details=True), reps)
    ts_half, (_, info_half) = _timed(lambda: xxz_evolve(ini, 1.0, 0.5 * HORIZONS, details=True), reps)
    k_full, k_half = int(info_full["terms"].max()), int(info_half["terms"].max())
    _emit(what="evolve", qubits=n, lanes=8, time="1.2 .. 9.6", terms=k_full, **_stats(ts_full))
    _emit(what="evolve", qubits=n, lanes=8, time="0.6 .. 4.8", terms=k_half, **_stats(ts_half))
    slope8 = 1e3 * (statistics.median(ts_full) - statistics.median(ts_half)) / (k_full - k_half)
    _emit(what="per_term", qubits=n, lanes=8, fit="two calls", **_term_rates(n, 8, float(slope8)))
    up, down = _copies(16 * 2**n, reps)
    _, down8 = _copies(16 * 8 * 2**n, reps)
    _emit(what="upload", qubits=n, lanes="1, and 8 from a shared state", **up)
    _emit(what="download", qubits=n, lanes=1, **down)
    _emit(what="download", qubits=n, lanes=8, **down8)
    for h, t in enumerate(HORIZONS, start=1):
        steps = precise_multiplier() * STEPS_PER_HORIZON * h
        ts, _ = _timed(lambda: trotter_state(n, evol_time=float(t), num_steps=steps), max(1, reps // 2))
        _emit(what="trotter_x10", qubits=n, time=float(t), steps=steps, **_stats(ts))


def probe_fidelity(n):
    exact = xxz_evolve(_neel(n), 1.0, HORIZONS)
    for h, t in enumerate(HORIZONS, start=1):
        steps = precise_multiplier() * STEPS_PER_HORIZON * h
        gt = trotter_state(n, evol_time=float(t), num_steps=steps)
        t1 = trotter_state(n, evol_time=float(t), num_steps=STEPS_PER_HORIZON * h)
        f = fidelity(gt, exact[h - 1])
        _emit(what="fidelity", qubits=n, time=float(t), steps_x10=steps, one_minus_fid_gt_vs_exact=1.0 - f,
              fid_t1_vs_exact=fidelity(t1, exact[h - 1]), fid_t1_vs_gt=fidelity(t1, gt))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--qubits", default="16,20,24")
    ap.add_argument("--fidelity-qubits", default="12,16,20")
    args = ap.parse_args()
    if args.reps < 1:
        ap.error("--reps must be positive")
    for n in (int(v) for v in args.qubits.split(",") if v):
        probe_shape(n, args.reps)
    for n in (int(v) for v in args.fidelity_qubits.split(",") if v):
        probe_fidelity(n)


if __name__ == "__main__":
    main()
