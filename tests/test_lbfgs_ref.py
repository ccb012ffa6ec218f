"""CPU: tests/lbfgs_ref.py -- the device L-BFGS rule in NumPy, written from the kernels -- against batched_lbfgs, the host loop
written before them, on the oracle's objectives of every case tests/test_hip_optimisers_wide.py runs on the device.  Both are
float64 NumPy with the same operation order: a difference above 1e-12 is a disagreement about the rule."""
import numpy as np
import pytest

from tests import lbfgs_cases as lc
from tests.helpers import maxdiff
from tests.lbfgs_ref import lbfgs_ref

KW = dict(gtol=1e-7, ftol=1e-12)


def _problem(name):
    _, fun, truth, _, starts = lc.problem(name)
    return fun, truth, starts


def _host_loop(fun, x0, **kw):
    """batched_lbfgs on ``fun``, with the trials of every iteration counted: it evaluates the start, then per iteration the trials
    (update_state False) and the accepted points once more (True)."""
    from aqc_research_amd.batched_optimizer import batched_lbfgs

    calls = []

    def counted(x, update):
        calls.append(bool(update))
        return fun(x)

    res = batched_lbfgs(counted, x0, **kw)
    assert calls[0] and res["nfev"] == len(calls)
    trials, n = [], 0
    for update in calls[1:]:
        if update:
            trials.append(n)
            n = 0
        else:
            n += 1
    assert n == 0
    return res, trials


def _compare(fun, x0, **kw):
    ref = lbfgs_ref(fun, x0, **kw)
    host, trials = _host_loop(fun, np.array(x0), **kw)
    dx, df = maxdiff(ref["x"], host["x"]), maxdiff(ref["fun"], host["fun"])
    print(f"nit {ref['nit']} trials {[t['trials'].tolist() for t in ref['trace']]} |x - x_host| = {dx:.2e} |f - f_host| = {df:.2e}")
    assert (ref["nit"] == host["nit"]).all()
    assert [int(t["trials"].max()) for t in ref["trace"]] == trials
    assert ref["nfev"] == lc.nfev_of(ref["trace"]) == host["nfev"] - len(trials)      # the host evaluates accepted points again
    assert (ref["active"] == ~host["lanes_converged"]).all()
    assert dx <= 1e-12 and df <= 1e-12
    return ref


@pytest.mark.parametrize("name,maxiter,memory", lc.SETTINGS)   # every setting the GPU module runs
def test_the_rule_is_the_host_loops_rule(name, maxiter, memory):
    fun, _, starts = _problem(name)
    ref = _compare(fun, starts, maxiter=maxiter, memory=memory, **KW)
    assert (ref["nit"] == maxiter).all() and len(ref["trace"]) == maxiter


def test_a_lane_that_stops_early_and_one_that_never_starts():
    fun, truth, starts = _problem("B")
    x0 = np.array(starts)
    x0[1] = truth[1] + 1e-4 * np.random.default_rng(1).standard_normal(truth.shape[1])
    ref = _compare(fun, x0, maxiter=8, memory=3, gtol=5.3e-5, ftol=1e-12)
    assert ref["nit"].tolist() == [8, 2, 8]
    for t in ref["trace"][2:]:       # an inactive lane: no trial of its own, a zeroed pair, and it stays where it stopped
        assert t["trials"][1] == 0 and not t["good"][1] and t["step"][1] == 0.0 and not t["active_in"][1]
        assert np.array_equal(t["x"][1], ref["trace"][1]["x"][1])
    x0[1] = truth[1]                 # max|g| ~ 1e-16 at the planted point: inactive from the start
    ref = _compare(fun, x0, maxiter=3, memory=3, **KW)
    assert ref["nit"].tolist() == [3, 0, 3] and np.array_equal(ref["x"][1], truth[1])


def _quadratics(rng, B, T):
    A = np.stack([(lambda m: m @ m.T + 0.5 * np.eye(T))(rng.standard_normal((T, T))) for _ in range(B)])
    xs = rng.standard_normal((B, T))

    def fun(x):
        r = x - xs
        return 0.5 * np.einsum("bt,btu,bu->b", r, A, r), np.einsum("btu,bu->bt", A, r)

    return fun, xs


def test_convex_quadratics_with_known_minimisers():
    fun, xs = _quadratics(np.random.default_rng(2), 4, 12)
    ref = _compare(fun, np.zeros((4, 12)), maxiter=300, memory=10, gtol=1e-10, ftol=0.0)
    assert maxdiff(ref["x"], xs) < 1e-7 and (ref["gmax"] <= 1e-10).all() and not ref["active"].any()
    assert (ref["nit"] < 300).all() and len(set(ref["nit"].tolist())) > 1      # lanes stop on their own, not together
    first = ref["trace"][0]           # first step: steepest descent of at most unit length
    _, g0 = fun(np.zeros((4, 12)))
    assert maxdiff(first["d"], -g0 / np.maximum(np.linalg.norm(g0, axis=1), 1.0)[:, None]) < 1e-15
    assert maxdiff(first["slope"], np.einsum("bt,bt->b", g0, first["d"])) < 1e-12
    for t in ref["trace"]:
        for i, m in enumerate(t["margins"]):      # a lane takes the Armijo test until it accepts
            assert (~np.isnan(m) == (t["trials"] > i)).all()
        assert ((t["step"] == 0.5 ** (t["trials"] - 1.0)) | (t["trials"] == 0)).all()


def test_stop_rules_and_rejected_pairs():
    fun, xs = _quadratics(np.random.default_rng(3), 3, 6)
    x0 = np.zeros((3, 6))
    # ftol: |f - f_new| <= ftol max(1, |f|) ends a lane after the step that made so little progress
    res = lbfgs_ref(fun, x0, maxiter=50, ftol=1e30)
    assert res["nit"].tolist() == [1, 1, 1] and not res["active"].any() and len(res["trace"]) == 1
    # a gradient that points uphill: no trial passes Armijo, the lane gives up after max_backtracks trials where it was
    def liar(x):
        f, g = fun(x)
        return f, -g

    res = lbfgs_ref(liar, x0, maxiter=5, max_backtracks=4)
    t = res["trace"][0]
    assert len(res["trace"]) == 1 and res["nfev"] == 5 and t["trials"].tolist() == [4, 4, 4]
    assert np.array_equal(res["x"], x0) and not t["good"].any() and res["nit"].tolist() == [1, 1, 1] and not res["active"].any()
    assert all((m > 0).all() for m in t["margins"])
    # negative curvature: sy <= 1e-12 yy zeroes the pair, and the next direction is steepest descent at gamma = 1
    def concave(x):
        return -0.5 * np.einsum("bt,bt->b", x, x), -x

    res = lbfgs_ref(concave, np.full((2, 5), 0.1), maxiter=2, memory=4)
    assert not res["trace"][0]["good"].any()
    assert np.array_equal(res["trace"][1]["d"], res["trace"][0]["x"])          # d = -g = x
    _compare(concave, np.full((2, 5), 0.1), maxiter=6, memory=2)
    _compare(liar, x0, maxiter=5, max_backtracks=4)


def test_argument_handling():
    fun, _ = _quadratics(np.random.default_rng(4), 2, 3)
    x0 = np.zeros((2, 3))
    for bad in (dict(memory=0), dict(memory=33), dict(maxiter=0), dict(max_backtracks=0), dict(gtol=-1.0), dict(ftol=float("nan"))):
        with pytest.raises(ValueError):
            lbfgs_ref(fun, x0, **bad)
    with pytest.raises(ValueError):
        lbfgs_ref(fun, np.zeros(3))
    with pytest.raises(TypeError):
        lbfgs_ref(fun, x0, 10)           # everything after x0 is a keyword
    keep = x0.copy()
    res = lbfgs_ref(fun, x0, maxiter=3, memory=1)
    assert np.array_equal(x0, keep) and res["x"] is not x0 and set(res) == {"x", "fun", "jac", "gmax", "nit", "nfev", "active", "trace"}
    assert set(res["trace"][0]) == {"x", "f", "f_in", "gmax", "tested", "d", "slope", "step", "trials", "margins", "good", "active_in", "active"}
    assert lbfgs_ref(fun, x0, maxiter=40, memory=32)["nit"].max() <= 40
