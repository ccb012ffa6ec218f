"""GPU: the masks and the issue order of the fused pass over the target (project_fused_kernel).

Its loads of y, M_end, psi and the offset tables are unconditional: a lane or wave without a column c / a block of u reads index 0 of
the same item and the value is replaced by 0 with a select.  The shapes below hit every mask and every grid shape of the launch; each
is asserted from ``projected_info`` to be the case it is meant to be (they were found with ``HipContext.plan_projected`` on the host).
Per shape: amplitudes and gradients of ``objective_launch`` against the two launches (AQC_PROJECTED_FUSED=0, the 1e-13 of
``test_fused_pass_equals_the_two_launches``) and against the oracle (``TOL``).

Lane 2's target is a normalised state times 2^40: a value that leaks through a mask, or a load clamped into another lane, is then
2^40 times too large to pass, while the exact power of two lets the lane's results be scaled back and held to the same tolerances
(amplitudes and gradients are linear in the target).
"""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import TOL, maxdiff
from oracle import aqc_oracle as orc

pytestmark = pytest.mark.gpu

_ROUTE_ENV = ("AQC_PROJECTED_FUSED", "AQC_PROJECTED_VDAG", "AQC_PROJECTED_FUSED_MAX_SHARES")
_BIG = 2.0 ** 40


@contextlib.contextmanager
def _env(**kv):
    """Environment variables for the workspaces created inside (None: unset)."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(circ, tile, th, tg, flips, **route):
    from aqc_research_amd.engine import BUF_X, BUF_Y, HipContext, Workspace

    env = dict({k: None for k in _ROUTE_ENV}, AQC_SPARSE_SWEEP="1", AQC_LAZY_Z="1", AQC_SPARSE_MIN_ITEMS="1", AQC_PROJECTED_VDAG_MIN_ELEMS="1")
    env.update(route)
    with _env(**env):
        ws = Workspace(HipContext(circ), batch=th.shape[0], tile_bits_apply=tile, tile_bits_sweep=tile)
        info = ws.projected_info()
        ws.upload(BUF_Y, tg)
        ws.set_basis(BUF_X, 0)
        ws.gather_setup(flips)
        ws.set_thetas(th)
        ws.objective_launch(BUF_X)
        out = (ws.gather_fetch().copy(), ws.get_grads().copy())
        ws.close()
    return info, out


def _check(n, blocks, tile, want, whole_walk=False):
    """One shape: the fused pass against the two launches and the oracle.  With 3 lanes the walk over the blocks of i_T is split into
    as many shares as it has blocks (gridDim.z > 1, one block each, project_csum_kernel); ``whole_walk`` runs it unsplit and in two
    shares as well, which is where a block has a successor to request."""
    from aqc_research_amd import ParametricCircuit
    from aqc_research_amd.circuit_structures import create_ansatz_structure

    rng = np.random.default_rng(4200 + 100 * n + blocks)
    circ = ParametricCircuit(n, "cx", create_ansatz_structure(n, "spin", "full", blocks))
    B = 3
    th = np.stack([orc.rand_thetas(circ.num_thetas, rng) for _ in range(B)])
    tg = np.stack([orc.rand_state(n, rng) for _ in range(B)])
    tg[2] *= _BIG
    scale = np.array([1.0, 1.0, 1.0 / _BIG])[:, None]
    flips = np.array([0] + [1 << q for q in range(n)], dtype=np.int64)
    info, fused = _run(circ, tile, th, tg, flips)
    assert info, "the shape was chosen for the route by projection"
    for key, val in want.items():
        assert info[key] == val, (key, info)
    assert info["shared_with_first_stage"] <= 4 and info["summed_bits"] <= 10   # (what the fused pass takes)
    runs = {"two": _run(circ, tile, th, tg, flips, AQC_PROJECTED_FUSED="0")[1]}
    if whole_walk:
        runs["whole"] = _run(circ, tile, th, tg, flips, AQC_PROJECTED_FUSED_MAX_SHARES="1")[1]
        runs["halves"] = _run(circ, tile, th, tg, flips, AQC_PROJECTED_FUSED_MAX_SHARES="2")[1]
    amps, grads = fused[0] * scale, fused[1] * scale
    for name, (a, g) in runs.items():
        da, dg = maxdiff(amps, a * scale), maxdiff(grads, g * scale)
        print(f"n={n} blocks={blocks} tile={tile} fused vs {name}: amplitudes {da:.3e} gradients {dg:.3e}")
        assert da < 1e-13 and dg < 1e-13, name
    x = np.zeros(1 << n, complex)
    x[0] = 1.0
    for b in (1, 2):
        vh = orc.v_dagger_mul_vec(circ, th[b], tg[b] * scale[b, 0])
        da, dg = maxdiff(amps[b], vh[flips]), maxdiff(grads[b], orc.grad_of_dot_product(circ, th[b], x, vh))
        print(f"n={n} blocks={blocks} tile={tile} lane {b} vs oracle: amplitudes {da:.3e} gradients {dg:.3e}")
        assert da < TOL and dg < TOL


# (qubits, blocks, tile bits, what projected_info must say, also run with the walk unsplit and in two shares)
_CASES = {
    # columns c >= 4 of the 16 do not exist (r16 >= 2^cb), all 256 values of u do
    "cvalid_mask": (12, 16, 10, {"shared_with_first_stage": 2, "summed_bits": 8, "touched_qubits": 4}, False),
    # 32 values of u: waves 1..7 have no block, wave 0 has both; columns c >= 8 masked as well; 8 blocks of i_T
    "uvalid_mask": (12, 20, 8, {"shared_with_first_stage": 3, "summed_bits": 5, "touched_qubits": 7}, True),
    # 128 values of u: the upper four waves masked; two blocks of i_T
    "uvalid_half": (12, 10, 9, {"shared_with_first_stage": 2, "summed_bits": 7, "touched_qubits": 5}, False),
    # 512 summed values at the smallest register that has them: two workgroups per item (blockIdx.y), project_sum_kernel
    "partial_projections": (13, 11, 10, {"shared_with_first_stage": 1, "summed_bits": 9, "touched_qubits": 4}, False),
    # |T| = 4: the walk is ONE block, no successor to request, no M_end to prefetch
    "single_block": (12, 16, 11, {"shared_with_first_stage": 3, "summed_bits": 8, "touched_qubits": 4}, False),
    # four blocks of i_T: four shares of one, two of two, one of four
    "split_walk": (13, 22, 10, {"shared_with_first_stage": 3, "summed_bits": 7, "touched_qubits": 6}, True),
    # the headline geometry, once
    "headline": (16, 40, 12, {"shared_with_first_stage": 4, "summed_bits": 8, "touched_qubits": 8}, True),
}


@pytest.mark.parametrize("case", sorted(_CASES))
def test_fused_pass_masks_and_grid_shapes(case):
    n, blocks, tile, want, whole = _CASES[case]
    _check(n, blocks, tile, want, whole)


def test_fused_pass_with_four_blocks_per_wave():
    """project_fused_kernel<4> shares the source (AQC_PROJECTED_FUSED_QB=4), in a process of its own."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("from tests.test_hip_fused_loads import _CASES, _check\n"
            "for c in ('uvalid_mask', 'partial_projections'):\n"
            "    n, blocks, tile, want, whole = _CASES[c]\n"
            "    _check(n, blocks, tile, want, whole)\n")
    env = dict(os.environ, AQC_PROJECTED_FUSED_QB="4")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
