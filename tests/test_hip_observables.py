"""GPU: reduced density matrices on the matrix cores (aqc_research_amd/observables.py, csrc/aqc_obs.hip) against the NumPy statement
(tests/obs_ref.py), against the XXZ energy of the package, and against properties that need no reference; the driver's option.

Sizes: n = 2 .. 16 reaches every path of the kernel -- below 4 qubits (virtual qubits), below a tile (zero fill), exactly a tile
(n = 11), the first pass with a high bit (n = 12) and several passes.  Up to n = 20 a block of the pass kernel owns one tile group
(2^(n-11) <= 512 = the grid's cap); n = 22 gives every block four, so the walk g, g + 512, ... runs: the prefetch of the next tile, the
barrier before the tile in LDS is overwritten, group numbers >= 512 in the non-tile bits, accumulation over tiles, and a second lane
entering after such a walk.

Tolerances are derived, not measured.  An entry of a pair's matrix is a sum of N = 2^(n-2) products a conj(b) of amplitudes of a
normalised state, sum |a||b| <= 1; any summation order errs by at most (N + 2) 2^-53 on it, on each side of a comparison:
    n <= 16:  2 (2^14 + 2) 2^-53 = 3.7e-12  ->  4e-12       n = 20:  2 (2^18 + 2) 2^-53 = 5.9e-11       n = 22:  2 (2^20 + 2) 2^-53 = 2.4e-10
The tests print what they observe; DESIGN.md 6n records it."""
import functools

import numpy as np
import pytest

from tests import obs_ref, xxz_ref

pytestmark = pytest.mark.gpu

RDM_TOL = 4e-12
RDM_TOL_20 = 2 * (2**18 + 2) * 2.0**-53


def _maxdiff(a, b) -> float:
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))))


@functools.lru_cache(maxsize=None)
def _states(n, lanes):
    return xxz_ref.random_states(n, lanes, 8100 + n)


def _neel(n):
    v = np.zeros(2**n, dtype=np.complex128)
    v[xxz_ref.neel_index(n)] = 1
    return v


@pytest.mark.parametrize("n", range(2, 17))
def test_pair_matrices_match_statement(n):
    from aqc_research_amd.observables import pair_density_matrices

    states = _states(n, 3)
    before = states.copy()
    pairs = obs_ref.all_pairs(n)
    got = pair_density_matrices(states)
    assert got.shape == (3, len(pairs), 4, 4) and got.dtype == np.complex128
    err = _maxdiff(got, obs_ref.pair_rdms(states, pairs))
    print(f"n = {n}: max |rho - statement| = {err:.3g}")
    assert err <= RDM_TOL, (n, err)
    # exactly Hermitian, real diagonal
    assert np.array_equal(got, got.conj().transpose(0, 1, 3, 2))
    assert np.all(got.imag[..., np.arange(4), np.arange(4)] == 0.0)
    # a lane of the stack is the one-state call, and a second call repeats the bits
    for lane in range(3):
        one = pair_density_matrices(states[lane])
        assert one.shape == (len(pairs), 4, 4)
        assert np.array_equal(one, got[lane]), (n, lane)
    assert np.array_equal(pair_density_matrices(states), got)
    assert np.array_equal(states, before)


@pytest.mark.parametrize("n", (3, 8, 12, 13))
def test_pair_orders_and_small_sets(n):
    from aqc_research_amd.observables import pair_density_matrices, reduced_density_matrix

    states = _states(n, 2)
    pairs = obs_ref.all_pairs(n)
    swapped = [(j, i) for i, j in pairs]
    fwd, rev = pair_density_matrices(states, pairs), pair_density_matrices(states, swapped)
    swap = [0, 2, 1, 3]
    assert np.array_equal(rev, fwd[..., swap, :][..., :, swap])
    assert _maxdiff(rev, obs_ref.pair_rdms(states, swapped)) <= RDM_TOL
    mixed = [(n - 1, 0), (0, n - 1), (1, 2), (n - 1, n - 2)]   # both orders in one list, a repeated pair
    assert _maxdiff(pair_density_matrices(states[0], mixed), obs_ref.pair_rdms(states[0], mixed)) <= RDM_TOL
    sets = [(0,), (n - 1,), (n // 2,), (0, 1, 2), (n - 1, 0, n // 2), (1, n - 1, 0)]
    if n >= 4:
        sets += [(0, 1, 2, 3), (n - 1, 0, n - 2, 1), (3, n // 2 + 1, 0, n - 1)]
    if n == 13:
        sets += [(0, 6, 11, 12), (12, 11, 6, 0), (12, 5, 9)]
    for qubits in sets:
        got = reduced_density_matrix(states, qubits)
        k = len(qubits)
        assert got.shape == (2, 2**k, 2**k)
        for lane in range(2):
            err = _maxdiff(got[lane], obs_ref.rdm(states[lane], qubits))
            assert err <= RDM_TOL, (n, qubits, lane, err)
        assert np.array_equal(got, got.conj().transpose(0, 2, 1))
        assert np.array_equal(reduced_density_matrix(states[1], qubits), got[1])


def test_twenty_qubits():
    from aqc_research_amd.observables import pair_density_matrices

    n = 20
    psi = _states(n, 1)[0]
    pairs = [(0, 19), (18, 19), (4, 5), (10, 11), (5, 12), (11, 12)]
    got = pair_density_matrices(psi, pairs)
    err = _maxdiff(got, obs_ref.pair_rdms(psi, pairs))
    print(f"n = {n}: max |rho - statement| = {err:.3g}")
    assert err <= RDM_TOL_20, err
    total = float(np.sum(np.abs(psi) ** 2))
    traces = np.trace(got, axis1=1, axis2=2)
    assert np.all(traces.imag == 0.0) and np.max(np.abs(traces.real - total)) <= RDM_TOL_20
    assert np.array_equal(got, got.conj().transpose(0, 2, 1))


_HIGH = (16, 17, 18, 19, 20, 21)
WALK_LISTS = {
    # one pass of 5 subsets (a wave with two of them) and one of a single subset, split over the four waves
    "five+one": [(i, j) for a, i in enumerate(_HIGH) for j in _HIGH[a + 1:]] + [(0, 16), (17, 1), (2, 18), (19, 3), (5, 6), (6, 7)],
    # one pass of 3 subsets (a subset per wave) and two of 2 subsets, each split over two waves
    "three+two+two": [(0, 21), (21, 20), (5, 6), (10, 11), (11, 12), (3, 17), (17, 19), (6, 15), (15, 16), (7, 8), (8, 9), (9, 10), (13, 14),
                      (12, 13)],
}
WALK_SUBSETS = {"five+one": [5, 1], "three+two+two": [3, 2, 2]}


@pytest.mark.parametrize("name", sorted(WALK_LISTS))
def test_blocks_that_walk_several_tile_groups(name):
    """n = 22: 2048 tile groups over 512 blocks, two lanes."""
    from aqc_research_amd.observables import pair_density_matrices, plan

    n, pairs = 22, WALK_LISTS[name]
    assert [len(s) for s in plan(n, pairs)["subsets"]] == WALK_SUBSETS[name]   # the passes this case is about
    tol = 2 * (2**20 + 2) * 2.0**-53
    states = _states(n, 2)
    before = states[:, ::4097].copy()
    got = pair_density_matrices(states, pairs)
    err = _maxdiff(got, obs_ref.pair_rdms(states, pairs))
    print(f"n = {n}, {name}: max |rho - statement| = {err:.3g}")
    assert err <= tol, (name, err)
    assert np.array_equal(got, got.conj().transpose(0, 1, 3, 2))
    assert np.array_equal(pair_density_matrices(states[1], pairs), got[1])   # the second lane of the stack is the one-state call
    assert np.array_equal(states[:, ::4097], before)


@pytest.mark.parametrize("n", (2, 11, 12, 16))
def test_bond_energies_sum_to_the_xxz_energy(n):
    """n - 1 bonds of operator norm 1/2 + |delta|/4 on matrices within 4e-12, and xxz_energy's own error of that order: 4e-12 R."""
    from aqc_research_amd.observables import bond_energies
    from aqc_research_amd.xxz import spectral_radius, xxz_energy

    states = _states(n, 3)
    for delta in (1.0, -0.7, 0.0):
        bonds = bond_energies(states, delta)
        assert bonds.shape == (3, n - 1)
        err = _maxdiff(bonds.sum(axis=1), xxz_energy(states, delta))
        print(f"n = {n}, delta = {delta}: |sum of bonds - energy| = {err:.3g}")
        assert err <= RDM_TOL * spectral_radius(n, delta), (n, delta, err)
        assert np.array_equal(bond_energies(states[1], delta), bonds[1])


def test_neel_state_under_the_xxz_chain():
    from aqc_research_amd.observables import bond_energies, correlation_matrix, magnetisation
    from aqc_research_amd.xxz import xxz_evolve

    n = 12
    neel = _neel(n)
    z0 = magnetisation(neel)
    assert z0.shape == (n,) and np.array_equal(z0, np.array([-1.0, 1.0] * (n // 2)))   # qubits 0, 2, ... are |1>
    assert np.array_equal(magnetisation(neel, "x"), np.zeros(n))
    e0 = bond_energies(neel, 1.0)
    assert np.array_equal(e0, np.full(n - 1, 0.25))
    evolved = xxz_evolve(neel, 1.0, 1.2)
    z1, e1 = magnetisation(evolved), bond_energies(evolved, 1.0)
    print(f"t = 1.2: staggered magnetisation {np.mean(z1 * z0):.6f}, sum Z drift {abs(z1.sum() - z0.sum()):.3g}, "
          f"energy drift {abs(e1.sum() - e0.sum()):.3g}")
    assert abs(z1.sum() - z0.sum()) <= 1e-11 and abs(e1.sum() - e0.sum()) <= 1e-11
    assert np.max(np.abs(z1)) < 1.0 and np.mean(z1 * z0) < 0.9       # the order has started to melt
    both = np.stack([neel, evolved])
    zz = correlation_matrix(both, "zz")
    assert zz.shape == (2, n, n) and np.array_equal(zz, zz.transpose(0, 2, 1))
    assert np.array_equal(zz[:, np.arange(n), np.arange(n)], np.ones((2, n)))
    assert np.array_equal(zz[0], np.outer(z0, z0))
    conn = correlation_matrix(both, "zz", connected=True)
    assert np.array_equal(conn[0], np.zeros((n, n)))                  # a product state
    # the single-site values come from other pairs than magnetisation's: 2^10 products each, (2^10 + 2) 2^-53 a side, squared terms twice
    assert np.max(np.abs(np.diagonal(conn[1]) - (1 - z1**2))) <= 1e-12
    xy, yx = correlation_matrix(evolved, "xy"), correlation_matrix(evolved, "yx")
    assert np.array_equal(xy, yx.T) and np.array_equal(np.diagonal(xy), np.zeros(n))
    # a seven-qubit chain: an odd number of qubits, the last one read from its left neighbour
    odd = _states(7, 1)[0]
    want = [obs_ref.expectation(obs_ref.rdm(odd, (q,)), "y") for q in range(7)]
    assert _maxdiff(magnetisation(odd, "y"), want) <= RDM_TOL


def test_driver_records_observables(monkeypatch):
    from aqc_research_amd.model_sp_lhs import time_evol as te
    from aqc_research_amd.observables import bond_energies, magnetisation

    n = 4
    kw = dict(num_qubits=n, num_horizons=1, num_layers_inc=1, maxiter=3, fidelity_thr=0.9)
    plain = te.run_simulation(te.UserOptions(**kw))[0]
    assert "observables" not in plain
    opts = te.UserOptions(observables=True, **kw)
    rec = te.run_simulation(opts)[0]
    ob = rec["observables"]
    assert sorted(ob) == ["bond_energies", "bond_energies_gt", "magnetisation", "magnetisation_gt"]
    assert ob["magnetisation"].shape == ob["magnetisation_gt"].shape == (n,)
    assert ob["bond_energies"].shape == ob["bond_energies_gt"].shape == (n - 1,)
    gt = te.generate_target(opts, 0).t1_gt
    assert np.array_equal(ob["magnetisation_gt"], magnetisation(gt))
    assert np.array_equal(ob["bond_energies_gt"], bond_energies(gt, opts.delta))
    # |tr O (rho - sigma)| <= ||O|| ||rho - sigma||_1 = 2 sqrt(1 - F) for pure states and ||Z|| = 1
    assert np.max(np.abs(ob["magnetisation"] - ob["magnetisation_gt"])) <= 2 * np.sqrt(1 - min(1.0, rec["fid_a1_vs_gt"])) + 1e-12
    # states of an MPS objective within dense reach carry their dense vector
    from aqc_research_amd.mps_operations import DenseBackedMPS

    wrapped = te._observables_entry(opts, DenseBackedMPS(gt, 1e-14), gt)
    assert np.array_equal(wrapped["magnetisation"], ob["magnetisation_gt"]) and np.array_equal(wrapped["bond_energies_gt"], ob["bond_energies_gt"])
    with pytest.raises(ValueError):
        te._observables_entry(opts, (None, None), gt)
    monkeypatch.setattr(te, "_DENSE_MAX_QUBITS", 3)
    with pytest.raises(ValueError):
        te.generate_target(te.UserOptions(observables=True, objective="sur_fast_mps_trotter", **kw), 0)


@pytest.mark.parametrize("extra", ({}, {"vectorised_lbfgs": True}), ids=("lockstep", "vectorised"))
def test_driver_records_observables_of_the_best_restart(extra):
    """Random restarts (num_seeds > 1) take another job of the driver: the entry describes the best restart's state at its thetas."""
    from aqc_research_amd.model_sp_lhs import time_evol as te
    from aqc_research_amd.model_sp_lhs.trotter import trotter_ansatz
    from aqc_research_amd.mps_operations import no_truncation_threshold
    from aqc_research_amd.observables import bond_energies, magnetisation

    n = 4
    kw = dict(num_qubits=n, num_horizons=1, num_layers_inc=1, maxiter=3, fidelity_thr=0.9, num_seeds=2, **extra)
    assert "observables" not in te.run_simulation(te.UserOptions(**kw))[0]
    opts = te.UserOptions(observables=True, **kw)
    rec = te.run_simulation(opts)[0]
    ob = rec["observables"]
    gt = te.generate_target(opts, 0).t1_gt
    circ = trotter_ansatz(n, rec["num_layers"], opts.second_order_trotter)
    a1 = te._evolved_state(opts, circ, rec["thetas"], no_truncation_threshold())
    assert ob["magnetisation"].shape == (n,) and ob["bond_energies"].shape == (n - 1,)
    assert np.array_equal(ob["magnetisation"], magnetisation(a1)) and np.array_equal(ob["bond_energies"], bond_energies(a1, opts.delta))
    assert np.array_equal(ob["magnetisation_gt"], magnetisation(gt)) and np.array_equal(ob["bond_energies_gt"], bond_energies(gt, opts.delta))


def test_errors_and_a_correct_call_afterwards():
    from ctypes import POINTER, c_int32

    from aqc_research_amd import _lib
    from aqc_research_amd.engine import live_buffers
    from aqc_research_amd.observables import (
        magnetisation, pair_density_matrices, pauli_expectation, reduced_density_matrix,
    )

    good = _states(5, 2)
    with pytest.raises(TypeError):
        pair_density_matrices(good.astype(np.complex64))
    with pytest.raises(TypeError):
        pair_density_matrices(np.asfortranarray(good))
    with pytest.raises(ValueError):
        pair_density_matrices(np.zeros(24, dtype=np.complex128))
    with pytest.raises(ValueError):
        pair_density_matrices(good, [(2, 2)])
    with pytest.raises(ValueError):
        pair_density_matrices(good, [(0, 5)])
    with pytest.raises(ValueError):
        pair_density_matrices(good, [])
    with pytest.raises(ValueError):
        reduced_density_matrix(np.zeros(64, dtype=np.complex128), (0, 1, 2, 3, 4))
    with pytest.raises(ValueError):
        pauli_expectation(pair_density_matrices(good[0], [(0, 1)]), "xw")
    # the library's own refusals, behind the Python checks
    L = _lib.lib()
    out = np.zeros((2, 1, 16, 16), dtype=np.complex128)
    i32 = lambda a: a.ctypes.data_as(POINTER(c_int32))   # noqa: E731
    for k, nsets, qubits, word in ((2, 1, [1, 1], b"twice"), (2, 1, [0, 5], b"out of range"), (2, 0, [0, 1], b"at least one"),
                                   (5, 1, [0, 1, 2, 3, 4], b"min(4, n)"), (0, 1, [0], b"min(4, n)")):
        q = np.array(qubits, dtype=np.int32)
        assert L.aqc_obs_rdm(0, 5, 2, _lib.dptr(good), k, nsets, i32(q), _lib.dptr(out)) == 1
        assert word in L.aqc_last_error(), L.aqc_last_error()
    q = np.array([0, 1, 2], dtype=np.int32)
    tiny = np.zeros((1, 4), dtype=np.complex128)
    assert L.aqc_obs_rdm(0, 2, 1, _lib.dptr(tiny), 3, 1, i32(q), _lib.dptr(out)) == 1      # k > n
    assert L.aqc_obs_rdm(0, 5, 0, _lib.dptr(good), 2, 1, i32(q), _lib.dptr(out)) == 1      # no lanes
    with pytest.raises(RuntimeError):
        pair_density_matrices(good, device=99)
    live = live_buffers()
    got = pair_density_matrices(good)
    assert _maxdiff(got, obs_ref.pair_rdms(good, obs_ref.all_pairs(5))) <= RDM_TOL
    assert magnetisation(good).shape == (2, 5)
    assert live_buffers() == live
