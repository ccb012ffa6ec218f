"""The wide-lane helper (tests/wide_lanes.py) on NumPy fakes: an honest batched function passes at 32769 and at 65538 lanes, and each
planted fault is caught by the check it belongs to with the lane named.  Without this a green run of test_hip_wide_lanes.py would
say nothing."""
import numpy as np
import pytest

from tests.wide_lanes import POOL, LaneContractError, Wide, check_wide, probe_lanes

DIM = 6
COUNTS = (32769, 65538)


def _pool(seed=11, lanes=POOL):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((lanes, DIM)), rng.standard_normal((lanes, 2)) + 1j * rng.standard_normal((lanes, 2))


def _batch(x, c):
    """The fake operation on every lane: a vector and a scalar per lane."""
    return {"vec": np.cumsum(x, axis=1) * c[:, :1].real + c[:, 1:], "num": np.einsum("ld,ld->l", x, x) + np.abs(c[:, 0])}


def honest(wide):
    return _batch(*wide.full())


def _reference(inputs, lane):
    out = _batch(inputs[0][lane:lane + 1], inputs[1][lane:lane + 1])
    return {"vec": out["vec"][0], "num": out["num"][0]}


def _run(fn, lanes, **kw):
    kw.setdefault("tol", 1e-13)
    return check_wide(fn, lanes, _pool(), reference=_reference, **kw)


def _faulty(fault):
    def run(wide):
        out = honest(wide)
        for arr in out.values():
            fault(arr, wide.lanes)
        return out

    return run


def _wrap_at(mark):
    def fault(arr, lanes):
        arr[mark:] = arr[:lanes - mark].copy()

    return fault


def _last_lane_zero(arr, lanes):
    arr[lanes - 1] = 0


def _exchanged(arr, lanes):
    a, b = lanes // 2, lanes // 2 + 3                                          # other pool members: 3 is no multiple of 7
    arr[[a, b]] = arr[[b, a]]


def _one_ulp(arr, lanes):
    if arr.ndim == 2:
        v = arr[lanes - 5, 2]
        arr[lanes - 5, 2] = np.nextafter(v.real, np.inf) + 1j * v.imag


@pytest.mark.parametrize("lanes", COUNTS)
def test_honest_function_passes(lanes):
    calls = []

    def counted(wide):
        calls.append(wide.lanes)
        return honest(wide)

    out = _run(counted, lanes)
    assert set(out) == {"vec", "num"} and out["vec"].shape == (lanes, DIM) and calls == [lanes, lanes]
    wide = Wide(lanes, _pool())
    assert np.array_equal(wide.column(0)[lanes - 1], _pool()[0][(lanes - 1) % POOL]) and wide.full()[1].shape == (lanes, 2)


@pytest.mark.parametrize("lanes", COUNTS)
def test_honest_function_passes_with_probe_lanes(lanes):
    """The lean scheme: the probe lanes have inputs of their own, are held to the reference and are left out of P; an output that only
    the probe lanes have is held to the reference too."""
    where = probe_lanes(lanes)
    assert {0, 1, 32766, 32767, 32768, lanes - 2, lanes - 1} <= set(where) and len(where) == (5 if lanes == 32769 else 8)
    own = _pool(77, len(where))

    def run(wide):
        out = honest(wide)
        out["probe:twice"] = 2.0 * out["vec"][list(wide.probe_lanes)]
        return out

    def reference(inputs, lane):
        ref = _reference(inputs, lane)
        return dict(ref, **{"probe:twice": 2.0 * ref["vec"]})

    out = check_wide(run, lanes, _pool(), probes=(where, own), reference=reference, tol=1e-13)
    assert np.array_equal(out["vec"][32767], _reference(own, where.index(32767))["vec"]) and out["probe:twice"].shape == (len(where), DIM)

    def forgets_a_probe(wide):                                                 # lane 32767 gets its pool member's result
        out = run(wide)
        for name in ("vec", "num"):
            out[name][32767] = out[name][32767 % POOL + POOL]
        return out

    with pytest.raises(LaneContractError) as e:
        check_wide(forgets_a_probe, lanes, _pool(), probes=(where, own), reference=reference, tol=1e-13)
    assert e.value.check == "reference" and "lane 32767" in str(e.value)


@pytest.mark.parametrize("lanes", COUNTS)
def test_lanes_served_from_behind_the_32768_mark(lanes):
    with pytest.raises(LaneContractError) as e:
        _run(_faulty(_wrap_at(32768)), lanes)
    assert e.value.check == "P" and "lane 32768," in str(e.value) and "output 'vec'" in str(e.value)


def test_lanes_served_from_behind_the_65536_mark():
    with pytest.raises(LaneContractError) as e:
        _run(_faulty(_wrap_at(65536)), 65538)
    assert e.value.check == "P" and "lane 65536," in str(e.value)


@pytest.mark.parametrize("lanes", COUNTS)
def test_last_lane_left_at_zero(lanes):
    with pytest.raises(LaneContractError) as e:
        _run(_faulty(_last_lane_zero), lanes)
    assert e.value.check == "P" and f"lane {lanes - 1}," in str(e.value)


@pytest.mark.parametrize("lanes", COUNTS)
def test_two_lanes_of_different_pool_members_exchanged(lanes):
    with pytest.raises(LaneContractError) as e:
        _run(_faulty(_exchanged), lanes)
    assert e.value.check == "P" and f"lane {lanes // 2}," in str(e.value)


@pytest.mark.parametrize("lanes", COUNTS)
def test_one_element_of_a_far_lane_off_by_one_ulp(lanes):
    with pytest.raises(LaneContractError) as e:
        _run(_faulty(_one_ulp), lanes)
    text = str(e.value)
    assert e.value.check == "P" and f"lane {lanes - 5}," in text and "output 'vec'" in text and "element (2,)" in text and text.count("0x") == 4


def test_an_output_that_is_the_same_for_every_pool_member():
    def run(wide):
        out = honest(wide)
        out["num"] = np.zeros_like(out["num"])
        return out

    with pytest.raises(LaneContractError) as e:
        _run(run, 32769)
    assert e.value.check == "distinct" and "output 'num'" in str(e.value)
    out = check_wide(run, 32769, _pool(), distinct=("vec",))                    # (not asked of an output that is not listed)
    assert not out["num"].any()


def test_the_other_guards():
    class Flickers:
        calls = 0

        def __call__(self, wide):
            out = honest(wide)
            self.calls += 1
            if self.calls == 2:
                out["num"][40000] = np.nextafter(out["num"][40000], np.inf)
            return out

    with pytest.raises(LaneContractError) as e:
        _run(Flickers(), 65538)
    assert e.value.check == "R" and "lane 40000," in str(e.value)

    def not_finite(wide):
        out = honest(wide)
        out["vec"][50000, 1] = np.nan
        return out

    with pytest.raises(LaneContractError) as e:
        _run(not_finite, 65538)
    assert e.value.check == "finite" and "lane 50000," in str(e.value)
    with pytest.raises(LaneContractError) as e:
        _run(lambda wide: {k: v * (1 + 1e-9) for k, v in honest(wide).items()}, 32769)
    assert e.value.check == "reference"

    def jitter(wide):                                                         # a sum by atomics: within its relative bound, not beyond
        out = honest(wide)
        out["num"][1::2] *= 1.0 + 2.0**-52
        out["vec"][20001::2, 3] *= 1.0 + 2.0**-52                            # (within the bound everywhere ...
        out["vec"][30003, 4] *= 1.0 + 2.0**-40                               # ... but for this element)
        return out

    _run(jitter, 32769, rel_tol={"num": 4 * 2.0**-52, "vec": 2.0**-39})
    with pytest.raises(LaneContractError) as e:
        _run(jitter, 32769, rel_tol={"num": 2.0**-54, "vec": 2.0**-39})
    assert e.value.check == "P" and "output 'num'" in str(e.value) and "beyond" in str(e.value)
    with pytest.raises(LaneContractError) as e:                               # the element named is the one beyond the bound, not the first that differs
        _run(jitter, 32769, rel_tol={"num": 4 * 2.0**-52, "vec": 4 * 2.0**-52})
    assert e.value.check == "P" and "lane 30003," in str(e.value) and "flat element 4:" in str(e.value)
