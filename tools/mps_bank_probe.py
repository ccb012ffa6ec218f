#!/usr/bin/env python3
"""One evaluation of the surrogate objective's amplitudes with a general state preparation beyond dense reach: V^H|target> and the
n + 1 overlaps <S X_i 0|V^H target>, timed two ways -- the lanes' bank (LockstepLanes.apply_vh_bank: V^H and all overlaps in one
native call, one launch of lanes_bank_dot_kernel) and the single-lane engine (v_dagger_mul_mps + one DeviceMPS.dot per state, each a
transfer-matrix chain of launches with a host sync).  The per-state dot loop is also timed alone on a fixed V^H|target>.
Warm-up, then the median of the repeats; prints one JSON line (milliseconds).  The two routes' amplitudes are compared as well.
Usage: python tools/mps_bank_probe.py [n] [repeats]"""
import json
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, ".")
from aqc_research_amd import TrotterAnsatz                                    # noqa: E402
from aqc_research_amd.circuit_structures import make_trotter_like_circuit     # noqa: E402
from aqc_research_amd.model_sp_lhs.objective_base import MpsStateHandler     # noqa: E402
from aqc_research_amd.mps_engine import LockstepLanes, v_dagger_mul_mps, v_mul_mps   # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 32
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
thr = 1e-12


class Circ:   # duck-typed preparation S: H on every qubit, a CX chain, two non-adjacent gates, RY
    def __init__(self):
        self.num_qubits, self.data, self.global_phase = n, [], 0.0

    def add(self, name, qubits, params=()):
        self.data.append(SimpleNamespace(operation=SimpleNamespace(name=name, params=list(params)), qubits=list(qubits)))


qc = Circ()
for q in range(n):
    qc.add("h", [q])
for q in range(n - 1):
    qc.add("cx", [q, q + 1])
qc.add("cx", [3, n // 3 + 2])
qc.add("cp", [n - 5, n // 2], [0.8])
for q in range(n):
    qc.add("ry", [q], [0.1 * (q % 7) - 0.3])

rng = np.random.default_rng(5)
circ = TrotterAnsatz(n, make_trotter_like_circuit(n, 1), second_order=False)
th_true = 0.3 * np.pi * (2 * rng.random(circ.num_thetas) - 1)
th = th_true + 0.03 * rng.standard_normal(th_true.size)
prep = MpsStateHandler(n, 1, qc)
states = prep.device_states
target = v_mul_mps(circ, th_true, states[5], trunc_thr=thr, method="single")
lk = LockstepLanes(n, 2).set_targets(target).set_bank(states)
th2 = np.stack([th, th])


def bank():
    return lk.apply_vh_bank(circ, th2, trunc_thr=thr, half=True)[0]


def single():
    vh = v_dagger_mul_mps(circ, th, target, trunc_thr=thr, method="single")
    out = np.array([x.dot(vh) for x in states])
    vh.close()
    return out


fixed_vh = v_dagger_mul_mps(circ, th, target, trunc_thr=thr, method="single")


def dots_only():
    return np.array([x.dot(fixed_vh) for x in states])


def median_ms(fn):
    for _ in range(3):
        fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()          # every route ends in a host read of its results (a device synchronisation)
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


a, b = bank(), single()
res = {"n": n, "states": len(states), "max_bond_states": prep.max_bond, "max_bond_target": int(target.bond_dims.max()),
       "max_abs_diff_routes": float(np.abs(a - b).max()), "repeats": repeats}
for name, fn in (("bank_ms", bank), ("single_lane_ms", single), ("dot_loop_only_ms", dots_only)):
    med, lo, hi = median_ms(fn)
    res[name] = med
    res[name.replace("_ms", "_min_max_ms")] = [lo, hi]
print(json.dumps(res))
lk.close()
