"""The lane-contract helper (tests/lane_contract.py) on NumPy fakes: an honest batched function passes every check, and each planted
fault is caught by the check it belongs to and by no earlier guard.  Without this a green run of test_hip_lane_contract.py would say
nothing."""
import numpy as np
import pytest

from tests.lane_contract import LaneContractError, check_lanes, default_permutation, nan_filled, substitute, take

LANES, DIM = 7, 6


def _inputs(seed=11, lanes=LANES):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((lanes, DIM)), rng.standard_normal((lanes, 2)) + 1j * rng.standard_normal((lanes, 2))


def _lane(x, c):
    """One lane of the fake operation: a vector and a scalar."""
    return np.cumsum(x) * c[0].real + c[1], np.dot(x, x) + abs(c[0])


def honest(inputs):
    x, c = inputs
    return {"vec": np.stack([_lane(x[l], c[l])[0] for l in range(len(x))]), "num": np.array([_lane(x[l], c[l])[1] for l in range(len(x))])}


def _reference(inputs, lane):
    vec, num = _lane(inputs[0][lane], inputs[1][lane])
    return {"vec": vec, "num": num}


def _neighbour(x, l):
    """What a leaking lane reads from outside: the largest element of the whole batch, so that the leak does not depend on where
    the lanes are (P passes) and only the neighbours' data shows it."""
    return np.full(x.shape[1], np.max(x))


def leaks_zero_times_neighbour(inputs):
    out = honest(inputs)
    x = inputs[0]
    out["vec"] = out["vec"] + np.stack([0.0 * _neighbour(x, l) for l in range(len(x))])
    return out


def leaks_tiny_neighbour(inputs):
    out = honest(inputs)
    x = inputs[0]
    out["vec"] = out["vec"] + np.stack([1e-17 * _neighbour(x, l) for l in range(len(x))])
    return out


def depends_on_index(inputs):
    out = honest(inputs)
    out["num"] = out["num"] * (1.0 + np.arange(len(out["num"])) * 2.0**-50)
    return out


class Flickers:
    """The last bit of one element changes from call to call."""

    def __init__(self):
        self.calls = 0

    def __call__(self, inputs):
        out = honest(inputs)
        self.calls += 1
        if self.calls % 2 == 0:
            out["vec"][3, 2] = np.nextafter(out["vec"][3, 2].real, np.inf) + 1j * out["vec"][3, 2].imag
        return out


def _run(fn, inputs=None, **kw):
    inputs = _inputs() if inputs is None else inputs
    kw.setdefault("tol", 1e-13)
    other = tuple(1000.0 * col for col in _inputs(99))        # data of a different kind: another scale
    return check_lanes(fn, inputs, other=other, reference=_reference, **kw)


def test_honest_function_passes_every_check():
    calls = []

    def counted(inputs):
        calls.append(1)
        return honest(inputs)

    out = _run(counted, also=(honest,))
    assert set(out) == {"vec", "num"} and out["vec"].shape == (LANES, DIM)
    assert len(calls) == 5                                    # clean, repeat, permuted, other, poison
    # the other structures of inputs and outputs
    check_lanes(lambda x: np.cumsum(x, axis=1), _inputs()[0], other=_inputs(5)[0])
    check_lanes(lambda cols: (cols[0] * 2.0, cols[0].sum(axis=1)), [_inputs()[0]], other=[_inputs(5)[0]])
    objs = [{"v": v} for v in _inputs()[0]]
    donors = [{"v": v} for v in _inputs(5)[0]]
    nans = [{"v": np.full(DIM, np.nan)} for _ in objs]
    check_lanes(lambda states: np.stack([s["v"] ** 2 for s in states]), objs, other=donors, poison=nans)
    with pytest.raises(TypeError):
        check_lanes(lambda states: np.stack([s["v"] ** 2 for s in states]), objs, other=donors)      # no default poison for objects


def test_zero_times_neighbour_is_caught_by_n_and_passes_f():
    _run(leaks_zero_times_neighbour, checks="RPF")
    with pytest.raises(LaneContractError) as e:
        _run(leaks_zero_times_neighbour)
    assert e.value.check == "N"
    assert "output 'vec'" in str(e.value) and "lane 0" in str(e.value) and "0x7ff8" in str(e.value)


def test_tiny_neighbour_is_caught_by_f():
    with pytest.raises(LaneContractError) as e:
        _run(leaks_tiny_neighbour)
    assert e.value.check == "F"
    text = str(e.value)
    assert "output 'vec'" in text and "element (" in text and text.count("0x") == 4         # complex: both parts of both values


def test_dependence_on_the_lane_index_is_caught_by_p():
    with pytest.raises(LaneContractError) as e:
        _run(depends_on_index, tol=1e-12)
    assert e.value.check == "P" and "output 'num'" in str(e.value)


def test_flicker_between_calls_is_caught_by_r():
    with pytest.raises(LaneContractError) as e:
        _run(Flickers())
    assert e.value.check == "R" and "lane 3" in str(e.value) and "element (2,)" in str(e.value)
    # a variant that disagrees is R as well
    with pytest.raises(LaneContractError) as e:
        _run(honest, also=(depends_on_index,))
    assert e.value.check == "R" and "variant 1" in str(e.value)


def test_identical_lanes_fire_the_distinct_guard():
    x, c = _inputs()
    x[LANES - 1], c[LANES - 1] = x[0], c[0]
    with pytest.raises(LaneContractError) as e:
        _run(honest, (x, c))
    assert e.value.check == "distinct" and "0 and 6" in str(e.value)


def test_the_other_guards():
    x, c = _inputs()
    x[2, 1] = np.inf
    with pytest.raises(LaneContractError) as e:
        _run(honest, (x, c))
    assert e.value.check == "finite" and "lane 2" in str(e.value)
    with pytest.raises(LaneContractError) as e:
        _run(lambda inputs: {k: v * (1 + 1e-9) for k, v in honest(inputs).items()})
    assert e.value.check == "reference"


def test_tolerated_output_and_restricted_lanes():
    """An output listed in rel_tol may move within its bound and no further; compare_lanes restricts R and P."""
    flips = []

    def jitter(inputs):
        out = honest(inputs)
        flips.append(1)
        out["num"] = out["num"] * (1.0 + (len(flips) % 2) * 2.0**-52)
        return out

    _run(jitter, rel_tol={"num": 4 * 2.0**-52})
    with pytest.raises(LaneContractError) as e:
        _run(jitter, rel_tol={"num": 2.0**-54})
    assert e.value.check == "R" and "beyond" in str(e.value)

    def wrong_in_lane_4(inputs):
        out = honest(inputs)
        out["num"][4] += len(flips)
        flips.append(1)
        return out

    _run(wrong_in_lane_4, checks="R", probes=(0, 3, 6), compare_lanes=(0, 3, 6))
    with pytest.raises(LaneContractError):
        _run(wrong_in_lane_4, checks="R", probes=(0, 3, 6))


def test_permutation_and_recipes():
    for lanes in (2, 3, 4, 5, 65, 129, 257, 65538):
        perm = default_permutation(lanes)
        assert sorted(perm.tolist()) == list(range(lanes)) and perm[0] != 0 and perm[-1] != lanes - 1
    inputs = _inputs()
    moved = take(inputs, [2, 0])
    assert np.array_equal(moved[0], inputs[0][[2, 0]]) and moved[0].flags.c_contiguous
    sub = substitute(inputs, _inputs(99), [1, 5])
    assert np.array_equal(sub[0][0], inputs[0][0]) and np.array_equal(sub[1][5], _inputs(99)[1][5])
    bad = nan_filled(inputs, [1])
    assert np.all(np.isnan(bad[0][1])) and np.all(np.isnan(bad[1][1])) and np.all(np.isfinite(bad[0][0]))
    assert np.all(np.isfinite(inputs[0]))                      # recipes never touch the caller's arrays
