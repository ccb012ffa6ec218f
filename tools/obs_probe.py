#!/usr/bin/env python
"""Reduced density matrices on the device (observables.pair_density_matrices -> aqc_obs_rdm): what a pass over the state costs.
Not a test: nothing here is a threshold.

Per shape (--qubits, default 16, 20, 24; --lanes, default 1, 8), on seeded random states, wall time of the call (upload, passes,
device synchronise, download of the small matrices), median of --reps (default 3) after a warm-up, with min - max:
  * "one":      the single pair (0, 1): one pass with one subset
  * "nearest":  the n - 1 nearest-neighbour pairs (light passes: a few subsets each)
  * "all":      all n (n - 1) / 2 pairs (heavy passes: up to 12 subsets each)
  * "energy":   xxz.xxz_energy on the same state, which uploads the same bytes and reads the vector once
A call's upload does not depend on the pair list, so the cost of a pass is a difference of calls:
  ms per light pass = (nearest - one) / (passes(nearest) - 1),  ms per heavy pass = (all - one) / (passes(all) - 1),
and "one - energy" compares the one-subset pass with the energy pass directly.  The byte model of a pass is the state read once,
16 B x lanes x 2^n, quoted against the 6.29 TB/s copy rate of DESIGN.md 6l.  One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from aqc_research_amd import observables as obs  # noqa: E402
from aqc_research_amd.xxz import xxz_energy  # noqa: E402

COPY_TBS = 6.29


def _timed(fn, reps):
    fn()   # warm-up: code objects, first allocation
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts)}


def _counts(n, pairs):
    p = obs.plan(n, pairs)
    return len(p["passes"]), sum(len(s) for s in p["subsets"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--qubits", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--lanes", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    for n in args.qubits:
        lists = {"one": [(0, 1)], "nearest": [(q, q + 1) for q in range(n - 1)], "all": [(i, j) for i in range(n) for j in range(i + 1, n)]}
        counts = {name: _counts(n, pairs) for name, pairs in lists.items()}
        for lanes in args.lanes:
            rng = np.random.default_rng(100 * n + lanes)
            states = rng.standard_normal((lanes, 2**n)) + 1j * rng.standard_normal((lanes, 2**n))
            states /= np.linalg.norm(states, axis=1, keepdims=True)
            states = np.ascontiguousarray(states)
            rec = {"qubits": n, "lanes": lanes, "state_mib": 16.0 * lanes * 2.0**n / 2**20}
            rec["energy"] = _timed(lambda: xxz_energy(states, 1.0), args.reps)
            for name, pairs in lists.items():
                rec[name] = dict(_timed(lambda: obs.pair_density_matrices(states, pairs), args.reps), passes=counts[name][0], subsets=counts[name][1])
            one = rec["one"]["median_ms"]
            rec["one_minus_energy_ms"] = one - rec["energy"]["median_ms"]
            for name, key in (("nearest", "ms_per_light_pass"), ("all", "ms_per_heavy_pass")):
                extra = rec[name]["passes"] - 1
                if extra > 0:
                    ms = (rec[name]["median_ms"] - one) / extra
                    rec[key] = ms
                    rec[key.replace("ms_per", "tb_per_s")] = 16.0 * lanes * 2.0**n / (ms * 1e-3) / 1e12 if ms > 0 else None
            rec["copy_rate_tb_per_s"] = COPY_TBS
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
