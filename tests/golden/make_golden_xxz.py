#!/usr/bin/env python3
"""
Generates ``xxz.npz`` in this directory by importing and running the *reference* (qiskit-community/aqc-research v0.1.0, its
checkout named by AQC_REFERENCE): its own ``make_hamiltonian(n, delta)`` and ``exact_evolution`` outputs, the ground truth of
tests/test_xxz_ref.py.  Runs only where the reference is present; the tests read the committed ``.npz`` alone.

Import accommodations as in make_golden.py (no reference code is modified or copied): the ``np.cfloat`` alias is restored, and
qiskit / qiskit-aer are registered as empty placeholder modules so that modules which import them at top level load.  No
placeholder is ever executed: ``make_hamiltonian`` and ``exact_evolution`` with a vector are NumPy / SciPy arithmetic.

Usage:  AQC_REFERENCE=<checkout> python tests/golden/make_golden_xxz.py
"""
import os
import sys
import types

import numpy as np

REF = os.environ.get("AQC_REFERENCE")
if not REF:
    sys.exit("set AQC_REFERENCE to the checkout of the reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
np.cfloat = np.complex128  # NumPy >= 2


def _placeholder(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


class _Missing:  # any attempt to *use* a qiskit object fails loudly
    def __init__(self, *a, **k):
        raise RuntimeError("qiskit is not available here")


_placeholder("qiskit", QuantumCircuit=_Missing)
_placeholder("qiskit.quantum_info", Operator=_Missing, Statevector=_Missing)
_placeholder("qiskit.circuit")
_placeholder("qiskit.circuit.library", QFT=_Missing)
_placeholder("qiskit_aer", AerSimulator=_Missing)
_placeholder("qiskit.algorithms")
_placeholder("qiskit.algorithms.optimizers", L_BFGS_B=_Missing, ADAM=_Missing, COBYLA=_Missing, BOBYQA=_Missing)
_placeholder("qiskit.algorithms.optimizers.optimizer", OptimizerResult=_Missing)
sys.modules["qiskit"].quantum_info = sys.modules["qiskit.quantum_info"]

sys.path.insert(0, REF)
import aqc_research.model_sp_lhs.trotter.trotter as ref_trotter  # noqa: E402

QUBITS, DELTAS, TIMES = (2, 3, 5), (1.0, 0.4), (0.7, 2.4)


def main():
    data, names = {}, []
    for n in QUBITS:
        dim = 2**n
        neel = np.zeros(dim, dtype=np.complex128)
        neel[sum(1 << q for q in range(0, n, 2))] = 1
        rng = np.random.default_rng(5000 + n)
        rand = rng.standard_normal(dim) + 1j * rng.standard_normal(dim)
        rand /= np.linalg.norm(rand)
        for delta in DELTAS:
            key = f"n{n}_d{delta}"
            h = np.asarray(ref_trotter.make_hamiltonian(n, delta), dtype=np.complex128)
            data[f"{key}/n"], data[f"{key}/delta"], data[f"{key}/h"] = np.int64(n), np.float64(delta), h
            data[f"{key}/neel"], data[f"{key}/rand"] = neel, rand
            for t in TIMES:
                for tag, vec in (("neel", neel), ("rand", rand)):
                    data[f"{key}/{tag}_t{t}"] = np.asarray(ref_trotter.exact_evolution(h, vec.copy(), float(t)), dtype=np.complex128)
            names.append(key)
    data["names"], data["times"] = np.array(names), np.asarray(TIMES)
    path = os.path.join(HERE, "xxz.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
