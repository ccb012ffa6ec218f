"""Named theta patterns outside [-pi, pi] and the lane sign the device is supposed to compute for them.  No GPU.

A rotation by theta enters every kernel through (cos, sin) of theta/2.  The coefficient builder (csrc/aqc_kernels.hip put_pair)
normalises each pair to cos >= 0 and hands the dropped sign on: coef_kernel multiplies the signs of a record, sign_kernel counts the
negative records of a lane -- leaving out the first `tail_blocks` block records of a second-order Trotter ansatz, which are executed
twice -- and the last stage of V x / V^H y multiplies by the result.  On [-pi, pi] no cosine is negative and none of this runs.

`thetas(circ, pattern, seed, ...)` returns the angles AND, per lane, the parity of that sign worked out here from the angles alone:
the number of half-angle parameters with cos(theta/2) < 0 outside the tail records, modulo 2.  The CPhase angle is a full angle and
never counts.  The GPU tests assert on this number, before anything is launched, that the path they are about is really taken.

Patterns (all seeded):
  wide          uniform in [-3 pi, 3 pi]: two thirds of the half-angle cosines are negative (pi < |theta| < 3 pi)
  flip_all      every angle in (pi, 3 pi) or (-3 pi, -pi), at least 0.1 away from the ends: every half-angle cosine is negative, so
                the parity is that of the COUNT of counted parameters, 3 n + 4 (L - tail_blocks) -- a property of the circuit, not of
                the draw.  It is odd for the 9-qubit circuits of the tests and even for the 10-qubit / 8-qubit-Trotter ones; on the
                latter flip_all still runs the c < 0 branch on every parameter and the count over n negative front records.
  exact         drawn from {0, -0.0, +-pi/2, +-pi, +-3pi/2, +-2pi, +-3pi, +-4pi}
  far           uniform in [-100, 100]
  one_flip      a [-pi, pi] base with 2 pi added to ONE parameter chosen by `role`: "front", "block" (outside the Trotter tail), "tail"
                (a block inside the first tail_blocks records; second-order Trotter only) or "cp" (the CPhase angle: no sign)
  lanes_mixed   4 lanes: base, one_flip("front"), wide, flip_all -- lane 0 is even and lane 1 odd whatever the seed

Seeds: `wide` needs a seed whose lanes include an odd one.  `check_reaches_sign_path` asserts it; the seeds the tests pass were chosen
so that it holds (with 4 lanes 15 draws in 16 do), and test_oracle_angles.py checks every (circuit, seed) pair the GPU file uses.
"""
import numpy as np

from oracle import aqc_oracle as orc

PATTERNS = ("wide", "flip_all", "exact", "far", "one_flip", "lanes_mixed")
ROLES = ("front", "block", "tail", "cp")
EXACT = np.array([0.0, -0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 1.5 * np.pi, -1.5 * np.pi, 2 * np.pi, -2 * np.pi,
                  3 * np.pi, -3 * np.pi, 4 * np.pi, -4 * np.pi])


def half_angle_mask(circ) -> np.ndarray:
    """(T,) bool: True where the parameter enters as theta/2 (every parameter but a CPhase angle)."""
    a = orc.as_ansatz(circ)
    m = np.ones(a.num_thetas, dtype=bool)
    if a.tpb == 5:
        m[3 * a.n + 4::5] = False
    return m


def counted_mask(circ) -> np.ndarray:
    """(T,) bool: the half-angle parameters whose dropped sign reaches V -- those of the tail records are applied twice."""
    a = orc.as_ansatz(circ)
    m = half_angle_mask(a)
    m[3 * a.n: 3 * a.n + a.tpb * a.tail_blocks] = False
    return m


def negative_mask(circ, th) -> np.ndarray:
    """Same shape as th: True where the parameter is a half angle and cos(theta/2) < 0."""
    return (np.cos(0.5 * np.asarray(th, float)) < 0.0) & half_angle_mask(circ)


def parity(circ, th):
    """Per lane: number of counted half-angle parameters with cos(theta/2) < 0, modulo 2 (lane sign = (-1)^parity)."""
    return (negative_mask(circ, th) & counted_mask(circ)).sum(axis=-1) % 2


def role_index(circ, role, rng) -> int:
    """A parameter index of the given role, drawn with `rng`."""
    a = orc.as_ansatz(circ)
    n, tpb, L, tail = a.n, a.tpb, a.num_blocks, a.tail_blocks
    if role == "front":
        return int(rng.integers(0, 3 * n))
    if role == "block":
        if L <= tail:
            raise ValueError("no block outside the Trotter tail")
        return 3 * n + tpb * int(rng.integers(tail, L)) + int(rng.integers(0, 4))
    if role == "tail":
        if tail == 0:
            raise ValueError("only a second-order Trotter ansatz has tail records")
        return 3 * n + tpb * int(rng.integers(0, tail)) + int(rng.integers(0, 4))
    if role == "cp":
        if tpb != 5:
            raise ValueError("only the cp entangler has a CPhase angle")
        return 3 * n + 5 * int(rng.integers(0, L)) + 4
    raise ValueError(f"unknown role {role!r}")


def _one(a, pattern, rng, role):
    T = a.num_thetas
    if pattern == "base":
        return orc.rand_thetas(T, rng)
    if pattern == "wide":
        return 3 * np.pi * (2 * rng.random(T) - 1)
    if pattern == "flip_all":
        mag = np.pi + 0.1 + (2 * np.pi - 0.2) * rng.random(T)
        return np.where(rng.random(T) < 0.5, -mag, mag)
    if pattern == "exact":
        return EXACT[rng.integers(0, EXACT.size, T)].copy()
    if pattern == "far":
        return 100.0 * (2 * rng.random(T) - 1)
    if pattern == "one_flip":
        th = orc.rand_thetas(T, rng)
        th[role_index(a, role, rng)] += 2 * np.pi
        return th
    raise ValueError(f"unknown pattern {pattern!r}")


def thetas(circ, pattern, seed, lanes=None, role=None):
    """(thetas, parity): thetas (T,) with lanes=None, else (lanes, T); parity an int or an int array (lanes,).  `lanes_mixed` is always
    4 lanes.  `one_flip` needs a role; with lanes every lane flips a parameter of that role of its own."""
    a = orc.as_ansatz(circ)
    rng = np.random.default_rng([int(seed), PATTERNS.index(pattern)])
    if pattern == "lanes_mixed":
        if lanes not in (None, 4):
            raise ValueError("lanes_mixed has 4 lanes")
        th = np.stack([_one(a, "base", rng, None), _one(a, "one_flip", rng, "front"), _one(a, "wide", rng, None), _one(a, "flip_all", rng, None)])
    elif lanes is None:
        th = _one(a, pattern, rng, role)
    else:
        th = np.stack([_one(a, pattern, rng, role) for _ in range(int(lanes))])
    p = parity(a, th)
    return th, (int(p) if th.ndim == 1 else p.astype(np.int64))


def one_flip_pair(circ, role, seed):
    """(base, flipped, index): the [-pi, pi] base of one_flip and the same thetas with 2 pi added to the parameter of `role`."""
    a = orc.as_ansatz(circ)
    th, _ = thetas(a, "one_flip", seed, role=role)
    base = np.random.default_rng([int(seed), PATTERNS.index("one_flip")])
    base = orc.rand_thetas(a.num_thetas, base)
    t = np.flatnonzero(th != base)
    assert t.size == 1 and th[t[0]] == base[t[0]] + 2 * np.pi
    return base, th, int(t[0])


def check_reaches_sign_path(circ, pattern, th, par, role=None) -> None:
    """The conditions under which a test of `pattern` really runs the sign path; from the angles alone, nothing is launched."""
    a = orc.as_ansatz(circ)
    th2, par2 = np.atleast_2d(th), np.atleast_1d(par)
    neg = negative_mask(a, th2)
    assert np.array_equal(par2, parity(a, th2))
    if pattern == "wide":
        assert (par2 == 1).any(), "wide: no odd lane, choose another seed"
        frac = neg.sum() / (half_angle_mask(a).sum() * th2.shape[0])
        assert 0.4 < frac < 0.9, frac      # 2/3 expected
    elif pattern == "flip_all":
        assert (neg == half_angle_mask(a)[None]).all()
        assert (np.abs(th2) > np.pi + 0.09).all() and (np.abs(th2) < 3 * np.pi - 0.09).all()
        assert (par2 == counted_mask(a).sum() % 2).all()
    elif pattern == "lanes_mixed":
        assert th2.shape[0] == 4 and par2[0] == 0 and par2[1] == 1 and not neg[0].any() and neg[1].sum() == 1
    elif pattern == "one_flip":
        tail = slice(3 * a.n, 3 * a.n + a.tpb * a.tail_blocks)
        for lane, p in zip(neg, par2):
            if role == "cp":
                assert p == 0 and not lane.any()
            elif role == "tail":
                assert p == 0 and lane[tail].sum() == 1 and lane.sum() == 1      # a negative tail record, an even lane
            else:
                assert p == 1 and lane.sum() == 1 and not lane[tail].any()
    elif pattern == "exact":
        assert np.isin(np.abs(th2), np.abs(EXACT)).all() and (np.abs(th2) > np.pi).any()
    elif pattern == "far":
        assert np.abs(th2).max() > 50.0 and neg.any()


# ---- the circuits of tests/test_hip_angle_range.py and the seeds its patterns are drawn with ------------------------------------
# name -> (entangler, qubits, blocks, trotter, second_order).  Spin layouts of 12 blocks at 9 qubits (two stages of 2^6 tiles on the
# VALU families) and 10 qubits (two stages of 2^8 tiles on the matrix cores); Trotter at 8 qubits, 2 layers: 42 blocks, a tail of 12.
def _mps_blocks():
    rng = np.random.default_rng(606)
    return np.stack([rng.permutation(6)[:2] for _ in range(9)], axis=1).astype(np.int64)


CIRCUITS = {
    **{f"{e}{n}": (e, n, orc.spin_blocks(n, 12), False, False) for e in ("cx", "cz", "cp") for n in (9, 10)},
    "trot1_8": ("cx", 8, orc.trotter_blocks(8, 2), True, False),
    "trot2_8": ("cx", 8, orc.trotter_blocks(8, 2), True, True),
    **{f"{e}5": (e, 5, orc.spin_blocks(5, 9), False, False) for e in ("cx", "cz", "cp")},
    "cx13": ("cx", 13, orc.spin_blocks(13, 20), False, False),
    "cp14": ("cp", 14, orc.spin_blocks(14, 22), False, False),
    "trot2_13": ("cx", 13, orc.trotter_blocks(13, 1), True, True),
    "cd5": ("cx", 5, orc.spin_blocks(5, 12), False, False),
    "cd7": ("cx", 7, orc.spin_blocks(7, 12), False, False),
    "mps_cx6": ("cx", 6, _mps_blocks(), False, False),
    "mps_trot2_6": ("cx", 6, orc.trotter_blocks(6, 1), True, True),
    "trot2_12": ("cx", 12, orc.trotter_blocks(12, 2), True, True),
}
# (circuit, pattern) -> lanes drawn in the GPU file
USES = {
    **{(c, p): 4 for c in ("cx9", "cz9", "cp9", "cx10", "cz10", "cp10", "trot1_8", "trot2_8") for p in ("wide", "flip_all", "exact", "far", "lanes_mixed")},
    **{(c, p): 4 for c in ("cx5", "cz5", "cp5", "cx13", "cp14", "trot2_13") for p in ("wide", "lanes_mixed")},
    ("cd5", "wide"): 3, ("cd7", "wide"): 3, ("mps_cx6", "wide"): 3, ("mps_trot2_6", "wide"): 3, ("trot2_12", "lanes_mixed"): 4,
}
# Seed 1 everywhere except where its draw of `wide` has no odd lane (check_reaches_sign_path); tests/test_oracle_angles.py checks
# every entry of USES with the seed given here.
SEEDS = {("cp9", "wide"): 2}


def ansatz(name) -> orc.Ansatz:
    e, n, blocks, trot, o2 = CIRCUITS[name]
    return orc.Ansatz(n, e, blocks, trot, o2)


def seed_for(name, pattern) -> int:
    return SEEDS.get((name, pattern), 1)


def case(name, pattern):
    """(ansatz, thetas (lanes, T), parity (lanes,)) of an entry of USES, checked to reach the sign path."""
    a = ansatz(name)
    th, par = thetas(a, pattern, seed_for(name, pattern), lanes=USES[(name, pattern)])
    check_reaches_sign_path(a, pattern, th, par)
    return a, th, par
