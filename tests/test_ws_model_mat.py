"""CPU self-test of the matrix call-sequence harness (tests/ws_model_mat.py): the sequences the device plays are played on
FakeMatWorkspace, the oracle's rendering of a correct matrix workspace; the generator covers every operation, refusal and
follow-up it is meant to; seven workspaces with one planted fault each are caught by the runner at the step where the fault
matters; and every data-dependent decision the references take on these inputs has a margin no rounding can cross."""
import numpy as np
import pytest

from tests import ws_model as wm
from tests import ws_model_mat as mm
from tests.ws_model import BUF_W, BUF_X, BUF_X2, BUF_Y, BUF_Z, BUF_ZW

CASES = [(name, seed) for name, shape in mm.SHAPES.items() for seed in shape[6]]
TABLE = ("sq6", "sq7", "sk7", "rect7")          # the shapes of the issue's table: full coverage is demanded there
_CACHE = {}


def _shape(name):
    if name not in _CACHE:
        make, ncols, _, lanes, fits, kind, seeds = mm.SHAPES[name]
        circ = make()
        _CACHE[name] = (circ, mm.MatOracle(circ), ncols, lanes, fits, kind, seeds)
    return _CACHE[name]


def _fake(name, cls=mm.FakeMatWorkspace):
    circ, orc, ncols, lanes, fits, kind, _ = _shape(name)
    return lambda: cls(circ, lanes, ncols, orc, fits, kind == "trotter")


def _play(name, ops, cls=mm.FakeMatWorkspace):
    circ, orc, ncols, lanes = _shape(name)[:4]
    return wm.run_sequence(_fake(name, cls), circ, lanes, ops, orc, kit=mm.MatKit(ncols))


def _all_ops(name):
    return [op for seed in _shape(name)[6] for op in mm.sequence(name, seed, _shape(name)[0])]


@pytest.mark.parametrize("name,seed", CASES)
def test_sequences_are_deterministic_legal_and_pass_on_the_oracle_workspace(name, seed):
    circ, _, _, lanes = _shape(name)[:4]
    ops = mm.sequence(name, seed, circ)
    again = mm.sequence(name, seed, circ)
    assert [o[0] for o in ops] == [o[0] for o in again] and wm.describe(ops, len(ops)) == wm.describe(again, len(again))
    assert 12 <= len(ops) <= 52   # (a deck slice, not a length: DESIGN 6t)
    assert mm.checked_preconditions(ops, lanes)
    assert len(_play(name, ops)) >= 3


@pytest.mark.parametrize("name", TABLE)
def test_table_shapes_are_planned_in_two_stages(name):
    """Host-only planner: V^H, the sweep and V of every shape of the table take two stages at the tile the device tests ask for
    (the matrix-core kernels raise sq6's 2^7 tiles to 2^8, which hold all of its six qubits: one stage there)."""
    from aqc_research_amd.engine import HipContext

    make, ncols, tile = mm.SHAPES[name][:3]
    ctx = HipContext(make())
    assert mm.planned_stages(ctx, ncols, tile) == [2, 2, 2]
    assert mm.planned_stages(ctx, ncols, max(tile, 8)) == ([1, 1, 1] if name == "sq6" else [2, 2, 2])


@pytest.mark.parametrize("name", TABLE)
def test_every_operation_occurs_where_it_is_legal(name):
    circ, _, ncols, lanes, fits, _, _ = _shape(name)
    ops = _all_ops(name)
    names = {o[0] for o in ops if not o[1].get("bad")}
    square, cd = ncols == circ.dimension, ncols == circ.dimension and circ.entangler != "cp"
    sketch = 1 < ncols < circ.dimension and ncols & (ncols - 1) == 0
    want = {"set_thetas", "theta_bank", "use_theta_set", "upload", "broadcast", "upload_lane", "copy_in", "copy_out", "download", "apply",
            "grad", "get_grads", "vdot", "vdot_launch", "gather", "eval", "objective_launch", "results_async", "results_fetch", "lbfgs_mat"}
    want |= {"set_identity"} if square else set()
    want |= {"cd_minimize"} if cd else set()
    want |= {"cd_sweeps"} if cd and fits else set()
    want |= {"sketch_target", "sketch_generate", "sketch_draw", "sketch_adam"} if sketch else set()
    assert want <= names, sorted(want - names)
    assert any(o[0] == "eval" and o[1]["th"] is None for o in ops) and any(o[0] == "eval" and o[1]["th"] is not None for o in ops)
    assert {bool(o[1]["inverse"]) for o in ops if o[0] == "apply"} == {True, False}
    assert {bool(o[1]["plain"]) for o in ops if o[0] == "grad" and not o[1].get("bad")} == {True, False}   # aqc_ws_grad and aqc_ws_grad_from
    lbfgs = [o[1] for o in ops if o[0] == "lbfgs_mat" and not o[1].get("bad")]
    assert all(1 <= a["maxiter"] <= 2 for a in lbfgs)
    if cd:
        routes = {o[1]["route"] for o in ops if o[0] == "cd_minimize" and not o[1].get("bad")}
        assert "wide" in routes or not fits
        assert all(o[1]["maxiter"] <= 2 for o in ops if o[0] == "cd_minimize" and not o[1].get("bad"))
    if sketch:
        assert {o[1]["kind"] for o in ops if o[0] == "sketch_generate"} == {"rand", "alt", "eigen"}
        assert all(o[1]["omega"] is not None for o in ops if o[0] == "sketch_generate" and o[1]["kind"] != "alt")
        resets = {int(v) for o in ops if o[0] == "sketch_adam" and not o[1].get("bad") for v in o[1]["reset"]}
        assert resets == {0, 1, 2}, resets
    # an evaluation's results copied behind a long-running call and fetched after it
    names_in_order = [o[0] for o in ops]
    spans = [names_in_order[i + 1:names_in_order.index("results_fetch", i)] for i, o in enumerate(names_in_order) if o == "results_async"]
    assert any(set(span) & set(mm.LONG) for span in spans), "no long-running call between results_async and results_fetch"


def test_one_lane_and_both_routes_are_reached_on_the_small_square_shapes():
    ops = _all_ops("sq6_1")
    assert any(o[0] == "cd_sweep" and not o[1].get("bad") for o in ops)
    routes = {o[1]["route"] for name in ("sq6", "sq6_1") for o in _all_ops(name) if o[0] == "cd_minimize" and not o[1].get("bad")}
    assert {"persistent", "wide"} <= routes, routes
    assert any(o[0] == "cd_sweeps" and o[1]["max_steps"] >= 0 for name in ("sq6", "sq6_1") for o in _all_ops(name) if not o[1].get("bad"))


def test_every_refusal_kind_occurs():
    bad = {(o[0], o[1]["bad"]) for name in mm.SHAPES for o in _all_ops(name) if o[1].get("bad")}
    kinds = {b for _, b in bad}
    for want in ("trotter", "cp entangler", "sketching on a square workspace", "sketching with k not a power of two",
                 "identity on a rectangle", "reset = 0 before any run", "lane", "index", "block range"):
        assert want in kinds, (want, sorted(kinds))
    assert ("lbfgs_mat", "trotter") in bad and ("cd_minimize", "cp entangler") in bad


def test_every_long_call_is_followed_both_ways():
    """... at once by a call that reads the thetas in use, and by set_thetas with the values from before the call, then a read."""
    seen = {}
    for name in mm.SHAPES:
        for seed in _shape(name)[6]:
            ops = mm.sequence(name, seed, _shape(name)[0])
            last_set = bank = None                         # the thetas the host handed over last
            for i, (op, a) in enumerate(ops):
                if op == "set_thetas" or (op == "eval" and a["th"] is not None):
                    last_set = a["th"]
                elif op == "theta_bank":
                    bank = a["bank"]
                elif op == "use_theta_set" and not a.get("bad"):
                    last_set = bank[a["i"]]
                if op not in mm.LONG or a.get("bad"):
                    continue
                before, rest = last_set, ops[i + 1:i + 5]
                names = [o[0] for o in rest]
                assert "apply" in names, (name, seed, i, names)
                k = names.index("apply")
                assert rest[k][1]["src"] == BUF_X2 and rest[k + 1][0] == "download"
                if a["follow"] == "direct":
                    assert "set_thetas" not in names[:k] and "use_theta_set" not in names[:k]
                else:
                    j = names.index("set_thetas")
                    assert j < k and before is not None and np.array_equal(rest[j][1]["th"], before)
                seen.setdefault(op, set()).add(a["follow"])
    for op in mm.LONG:
        assert seen.get(op) == {"direct", "same"}, (op, seen.get(op))


# ---- planted faults: one per workspace, each caught at the step where it matters -----------------------------------------------

class LbfgsLeavesTheLastTrial(mm.FakeMatWorkspace):
    def _lbfgs_exit(self, ref):
        last = ref["trace"][-1]
        self.th = last["x"] + 0.5 * last["d"]      # some trial of the last line search, not the point returned


class WideCdLeavesZMarkedValid(mm.FakeMatWorkspace):
    """After the wide walk has scribbled on Z the workspace still takes it for V^H Y: the next V^H of Y into Z is skipped."""

    def _cd_exit(self, wide, ths, best_th):
        super()._cd_exit(wide, ths, best_th)
        self._z_taken_as_valid = wide

    def apply(self, inverse, src=BUF_Y, dst=BUF_Z):
        if inverse and src == BUF_Y and dst == BUF_Z and getattr(self, "_z_taken_as_valid", False):
            self._touch(BUF_Z, BUF_ZW)
            return
        self._z_taken_as_valid = False
        super().apply(inverse, src, dst)


class RoutesLeaveDifferentThetas(mm.FakeMatWorkspace):
    def _cd_exit(self, wide, ths, best_th):
        kept = self.th.copy()
        super()._cd_exit(wide, ths, best_th)
        self.th = ths[-1].copy() if wide else kept   # the last sweep's on the wide route, untouched on the persistent one


class AdamContinuesFromTheThetasInUse(mm.FakeMatWorkspace):
    def _adam_resume(self, lane):
        return self.th[lane]


class EigenUsesThePreviousThetas(mm.FakeMatWorkspace):
    def _eigen_thetas(self):
        return getattr(self, "_prev_thetas", self.th)


class RefusedIdentityClearsTheBuffer(mm.FakeMatWorkspace):
    def set_identity(self, buf):
        if self.ncols != self.dim:
            self.b[buf][:] = 0
        super().set_identity(buf)


class CdKeepsTheGenerationOfZW(mm.FakeMatWorkspace):
    def _cd_exit(self, wide, ths, best_th):
        keep = self._gen[BUF_ZW]
        super()._cd_exit(wide, ths, best_th)
        self._gen[BUF_ZW] = keep


def _rng_mats(name, seed, count=1):
    circ, _, ncols, lanes = _shape(name)[:4]
    g = mm.MatGen(seed, circ, lanes, ncols, True)
    return g, [g.mats(lanes) for _ in range(count)]


def _fault_sequences():
    g5, (y5, x5, x25) = _rng_mats("sq6", 11, 3)
    g7, (y7, x7, x27) = _rng_mats("sk7", 12, 3)
    gr, (yr, xr) = _rng_mats("rect7", 13, 2)
    th5, th5b, th7, th7b = g5.thetas(), g5.thetas(), g7.thetas(), g7.thetas()
    open5 = [("upload", {"buf": BUF_Y, "data": y5}), ("upload", {"buf": BUF_X, "data": x5}), ("upload", {"buf": BUF_X2, "data": x25}),
             ("set_thetas", {"th": th5})]
    open7 = [("upload", {"buf": BUF_X2, "data": x27}), ("set_thetas", {"th": th7}), ("sketch_target", {"U": g7.unitaries()})]
    probe = [("apply", {"inverse": False, "src": BUF_X2, "dst": BUF_W}), ("download", {"buf": BUF_W, "lane": None})]
    cd = {"th": th5b, "maxiter": 2, "chunk": 1}
    om = g7.rng.standard_normal((3, 128, 8)) + 1j * g7.rng.standard_normal((3, 128, 8))
    adam = {"kind": "alt", "x0": th7b, "niter": 2, "lr": 0.1, "seed": 3, "iter0": 0, "reset": np.ones(3, np.int32), "alt_idx": g7.alt_idx(3)}
    return {
        "lbfgs_mat leaves the last trial in use": (
            "sq6", LbfgsLeavesTheLastTrial, "download",
            open5 + [("lbfgs_mat", {"x0": th5b, "maxiter": 2, "memory": 2, "max_backtracks": 12})] + probe),
        "a wide-route CD call leaves Z marked valid": (
            "sq6", WideCdLeavesZMarkedValid, "download",
            open5 + [("cd_minimize", dict(cd, route="wide")), ("apply", {"inverse": True, "src": BUF_Y, "dst": BUF_Z}),
                     ("download", {"buf": BUF_Z, "lane": None})]),
        "the persistent and wide routes differ in the thetas they leave": (
            "sq6", RoutesLeaveDifferentThetas, "download", open5 + [("cd_minimize", dict(cd, route="persistent"))] + probe),
        "ADAM continuation starts from the thetas in use": (
            "sk7", AdamContinuesFromTheThetasInUse, "sketch_adam.x",
            open7 + [("sketch_adam", adam), ("set_thetas", {"th": th7}),
                     ("sketch_adam", dict(adam, x0=None, iter0=2, reset=np.zeros(3, np.int32)))]),
        "sketch_generate('eigen') uses the thetas of the previous call": (
            "sk7", EigenUsesThePreviousThetas, r"sketch_generate.range",
            open7 + [("sketch_generate", {"kind": "eigen", "seed": 1, "iteration": 1, "omega": om, "alt_idx": None}),
                     ("set_thetas", {"th": th7b}),
                     ("sketch_generate", {"kind": "eigen", "seed": 1, "iteration": 2, "omega": om, "alt_idx": None})]),
        "a refused call changes a buffer": (
            "rect7", RefusedIdentityClearsTheBuffer, "download",
            [("upload", {"buf": BUF_Y, "data": yr}), ("upload", {"buf": BUF_X, "data": xr}),
             ("set_identity", {"buf": BUF_X, "bad": "identity on a rectangle"}), ("download", {"buf": BUF_X, "lane": None})]),
        "a rewritten buffer keeps its generation()": (
            "sq6", CdKeepsTheGenerationOfZW, r"rewrote ZW and left its generation",
            open5 + [("cd_minimize", dict(cd, route="wide"))]),
    }


FAULTS = ["lbfgs_mat leaves the last trial in use", "a wide-route CD call leaves Z marked valid",
          "the persistent and wide routes differ in the thetas they leave", "ADAM continuation starts from the thetas in use",
          "sketch_generate('eigen') uses the thetas of the previous call", "a refused call changes a buffer",
          "a rewritten buffer keeps its generation()"]


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_caught_where_it_matters(fault):
    name, cls, where, ops = _fault_sequences()[fault]
    _play(name, ops)                                        # the sequence is a fair one: the correct workspace passes it
    with pytest.raises(AssertionError) as err:
        _play(name, ops, cls)
    msg = str(err.value)
    last = len(ops) - 1
    assert f"step {last} " in msg and where.replace("\\", "") in msg, msg.splitlines()[0]


# ---- decision margins ------------------------------------------------------------------------------------------------------

def test_every_decision_of_the_references_has_a_margin():
    """Every data-dependent branch of the references -- Armijo accept (lbfgs_ref reports the margins of the tests it took), its
    descent, curvature and relative-decrease tests, best-so-far of coordinate descent and of ADAM -- on every input the random
    sequences and the directed device sequences (ws_model_mat.directed) use: the reference decides with a relative margin of at
    least 1e-6.  Stop thresholds are 0 (gtol, ftol, tol, dtheta_thr, fobj_thr): no stop rule is near its value."""
    worst, rejected = {}, 0
    plays = [(name, mm.sequence(name, seed, _shape(name)[0])) for name in mm.SHAPES for seed in _shape(name)[6]]
    plays += [(name, ops) for name, ops, _ in mm.directed(lambda name: _shape(name)[0]).values()]
    for name, ops in plays:
        circ, orc, ncols, lanes, fits, kind, _ = _shape(name)
        log = []

        class Spy(mm.FakeMatWorkspace):
            def lbfgs_mat(self, x0, **kw):
                x, y = self.b[BUF_X].copy(), self.b[BUF_Y].copy()
                res = super().lbfgs_mat(x0, **kw)       # (raises where the call is refused)
                ref = mm.lbfgs_reference(self.orc, x, y, np.array(x0, float), kw["maxiter"], kw["memory"], kw["max_backtracks"])
                log.append(("armijo", mm.lbfgs_margins(ref), int(sum((it["step"] == 0)[it["active_in"]].sum() for it in ref["trace"]))))
                log.extend((what, m, 0) for what, m in mm.lbfgs_branch_margins(ref).items())
                return res

            def cd_minimize(self, thetas0, maxiter, **kw):
                res = super().cd_minimize(thetas0, maxiter, **kw)
                log.append(("cd best", mm.cd_margins(res["profile"]), 0))
                return res

            def sketch_adam(self, *args, **kw):
                res = super().sketch_adam(*args, **kw)
                log.append(("adam best", mm.adam_margins(res["profile"]), 0))
                return res

        wm.run_sequence(lambda: Spy(circ, lanes, ncols, orc, fits, kind == "trotter"), circ, lanes, ops, orc, kit=mm.MatKit(ncols))
        for what, margins, rej in log:
            rejected += rej
            if len(margins):
                worst[what] = min(worst.get(what, np.inf), float(min(margins)))
    print("smallest relative margins:", worst, "; line searches that ended without an accepted trial:", rejected)
    assert set(worst) == {"armijo", "descent", "curvature", "decrease", "cd best", "adam best"}
    assert all(v >= 1e-6 for v in worst.values()), worst
    assert rejected > 0, "no sequence makes a lane reject its last trial: the case lbfgs_mat's exit is about does not occur"
