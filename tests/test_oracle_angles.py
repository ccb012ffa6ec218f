"""CPU: the theta patterns of tests/angle_cases.py and, on both oracles, the two identities the device's sign normalisation rests on."""
import numpy as np
import pytest

from oracle import aqc_oracle as orc
from oracle import aqc_ref as cref
from tests import angle_cases as ac
from tests.helpers import maxdiff


@pytest.mark.parametrize("name,pattern", sorted(ac.USES))
def test_every_case_of_the_gpu_file_reaches_the_sign_path(name, pattern):
    a, th, par = ac.case(name, pattern)
    assert th.shape == (ac.USES[(name, pattern)], a.num_thetas) and par.shape == th.shape[:1]
    if pattern == "wide":
        assert (par == 1).any()
    if pattern == "lanes_mixed":
        assert (par == 0).any() and (par == 1).any()
    if pattern == "flip_all" and a.n == 9:
        assert (par == 1).all()          # 3 n + 4 L = 75 counted parameters, all negative


@pytest.mark.parametrize("name", ["cx9", "cp10", "trot1_8", "trot2_8"])
def test_one_flip_roles(name):
    a = ac.ansatz(name)
    roles = ["front", "block"] + (["tail"] if a.tail_blocks else []) + (["cp"] if a.tpb == 5 else [])
    for role in roles:
        base, th, t = ac.one_flip_pair(a, role, 3)
        ac.check_reaches_sign_path(a, "one_flip", th, ac.parity(a, th), role)
        assert ac.parity(a, base) == 0 and not ac.negative_mask(a, base).any()
        in_tail = 3 * a.n <= t < 3 * a.n + a.tpb * a.tail_blocks
        assert in_tail == (role == "tail") and ac.half_angle_mask(a)[t] == (role != "cp")
    for role in {"tail", "cp"} - set(roles):
        with pytest.raises(ValueError):
            ac.role_index(a, role, np.random.default_rng(0))


@pytest.mark.parametrize("name", ["cx5", "cz5", "cp5", "mps_trot2_6"])
def test_two_pi_on_one_parameter(name):
    """V(theta + 2 pi e_t) = -V(theta) for a half-angle parameter (+V for one of a tail record of a second-order Trotter ansatz: that
    rotation is applied twice) and = V(theta) for the CPhase angle -- on the NumPy and on the compiled oracle, for V x, V^H y and the
    gradient, whose inner products see the sign twice."""
    a = ac.ansatz(name)
    rng = np.random.default_rng(17)
    th = orc.rand_thetas(a.num_thetas, rng)
    x, y = orc.rand_state(a.n, rng), orc.rand_state(a.n, rng)
    half, counted = ac.half_angle_mask(a), ac.counted_mask(a)
    for o in (orc, cref):
        vx, vhy = o.v_mul_vec(a, th, x), o.v_dagger_mul_vec(a, th, y)
        g = o.grad_of_dot_product(a, th, x, vhy)
        for t in range(a.num_thetas):
            th2 = th.copy()
            th2[t] += 2 * np.pi
            s = -1.0 if counted[t] else 1.0
            assert ac.parity(a, th2) == (1 if counted[t] else 0)
            assert (np.cos(0.5 * th2[t]) < 0) or not half[t]
            vhy2 = o.v_dagger_mul_vec(a, th2, y)
            assert maxdiff(o.v_mul_vec(a, th2, x), s * vx) < 1e-13 and maxdiff(vhy2, s * vhy) < 1e-13
            assert maxdiff(o.grad_of_dot_product(a, th2, x, vhy2), s * g) < 1e-13     # <V x|y> itself changes sign with V
