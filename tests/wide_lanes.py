"""Lane counts at which an oracle per lane is out of reach: the lane contract of tests/lane_contract.py inside ONE call.

All lanes of a call are built from a pool of POOL = 7 distinct inputs, lane l gets pool member l mod 7.  Seven is coprime to 32768 and
to 65536, so a lane that is dropped, wrapped at either mark or served from a neighbour lands on another pool member.  `check_wide`
holds a callable `run(wide) -> outputs` to this:

    finite      every output of every lane is finite
    distinct    the outputs listed (default: every floating-point output) differ between any two pool members (lanes 0 .. 6): without
                it an output that is zero everywhere would pass
    reference   lanes 0 .. 6 agree with `reference(pool, k)` within `tol` (the feature's own reference and tolerance), and every probe
                lane with `reference(probe_inputs, j)`
    R           the same call again gives the same bits, on every lane
    P           every other lane is np.array_equal to lane l mod 7 of the same call (position, used inside one call)

`probes` = (lanes, inputs) names lanes that do NOT follow the pool: they get inputs of their own (the same structure, one lane per
probe) and are held to the reference instead of to P.  That is the lean scheme of the largest cases, where the inputs and outputs
never exist as full host arrays: `run` builds from `wide` whatever it can afford (`wide.column(i)` expands one column, `wide.full()`
all of them) and returns arrays with a leading axis of all lanes; an output whose name starts with "probe:" has one row per probe
lane instead (a full state read from the probe lanes only).

A failure raises LaneContractError (tests/lane_contract.py) whose `.check` is one of the names above and whose text names the lane,
the output and the first differing element with both bit patterns.
"""
import numpy as np

from tests.lane_contract import LaneContractError, _bits, _first_difference, _named, _named_lane, _split

POOL = 7
PROBE = "probe:"


def probe_lanes(lanes):
    """The lanes on either side of the marks 32768 and 65536 (the second one cannot be a lane of a workspace) and at both ends."""
    want = (0, 1, 32766, 32767, 32768, 32769, lanes - 2, lanes - 1)
    return tuple(sorted({l for l in want if 0 <= l < lanes}))


class Wide:
    """The inputs of one call: `lanes` lanes, lane l = pool member l mod 7, except the probe lanes."""

    def __init__(self, lanes, pool, probes=None):
        self.lanes, self.pool = int(lanes), pool
        self.member = np.arange(self.lanes) % POOL
        self.probe_lanes, self.probe_inputs = ((), None) if probes is None else (tuple(int(l) for l in probes[0]), probes[1])
        self.pooled = np.ones(self.lanes, dtype=bool)                          # the lanes that follow the pool
        if self.probe_lanes:
            self.pooled[list(self.probe_lanes)] = False

    def column(self, i):
        """Column i for all lanes (a fresh array, or a fresh list of per-lane objects)."""
        col = _split(self.pool)[0][i]
        if isinstance(col, np.ndarray):
            out = np.ascontiguousarray(col[self.member])
        else:
            out = [col[k] for k in self.member]
        if self.probe_lanes:
            pcol = _split(self.probe_inputs)[0][i]
            for j, l in enumerate(self.probe_lanes):
                out[l] = pcol[j]
        return out

    def full(self):
        """Every column for all lanes, in the structure of the pool."""
        cols, rebuild = _split(self.pool)
        return rebuild([self.column(i) for i in range(len(cols))])


def _unequal_lanes(a, b):
    """bool[lanes]: where lane l of a and of b differ by np.array_equal's rule (so a NaN differs from itself)."""
    return (~(a == b)).reshape(len(a), -1).any(axis=1)


def _raise_first(check, what, name, ref, got, bad, lanes_of_ref=None):
    l = int(np.flatnonzero(bad)[0])
    lr = l if lanes_of_ref is None else int(lanes_of_ref[l])
    raise LaneContractError(check, f"{what}: lane {l}, output {name!r}, {_first_difference(ref[lr], got[l])}")


def check_wide(run, lanes, pool, *, reference=None, tol=None, probes=None, distinct=None, rel_tol=None):
    """Hold `run` to the contract above at `lanes` lanes; returns the named outputs of the first call.

    pool, probes     inputs in the structures of tests/lane_contract.py: POOL lanes, and (probe lanes, one lane per probe) or None
    reference, tol   (inputs, lane) -> that lane's outputs in the structure `run` returns, without the lane axis (fewer outputs are
                     fine); `tol` is one bound or {output: bound}
    rel_tol          {output: relative bound} for the outputs that are not compared exactly (sums by atomics)
    distinct         the outputs that must differ between any two pool members; default: every floating-point output
    """
    lanes = int(lanes)
    if lanes < 2 * POOL:
        raise ValueError(f"a wide call has at least {2 * POOL} lanes")
    wide = Wide(lanes, pool, probes)
    nprobe = len(wide.probe_lanes)
    # the lane that stands for pool member k: lane k, or the first lane of that member which is no probe
    members = [int(np.flatnonzero(wide.pooled & (wide.member == k))[0]) for k in range(POOL)]
    rel_tol = dict(rel_tol or {})

    def named(outputs):
        if not isinstance(outputs, dict):
            return _named(outputs, lanes)
        every = _named({k: v for k, v in outputs.items() if not str(k).startswith(PROBE)}, lanes)
        every.update(_named({k: v for k, v in outputs.items() if str(k).startswith(PROBE)}, nprobe) if nprobe else {})
        return every

    base = named(run(wide))
    wide_names = [n for n in base if not n.startswith(PROBE)]

    for name, arr in base.items():
        if arr.dtype.kind in "fc":
            bad = ~np.isfinite(arr).reshape(len(arr), -1).all(axis=1)
            if bad.any():
                l = int(np.flatnonzero(bad)[0])
                raise LaneContractError("finite", f"lane {wide.probe_lanes[l] if name.startswith(PROBE) else l}, output {name!r} is not finite")
    for name in ([n for n in wide_names if base[n].dtype.kind in "fc"] if distinct is None else list(distinct)):
        for i, p in enumerate(members):
            for q in members[i + 1:]:
                if np.array_equal(base[name][p], base[name][q]):
                    raise LaneContractError("distinct", f"lanes {p} and {q} (two pool members) have the same output {name!r}")

    if reference is not None:
        if tol is None:
            raise ValueError("a reference needs its tolerance")
        bound = (lambda name: tol[name]) if isinstance(tol, dict) else (lambda name: tol)
        held = [(l, None, pool, k) for k, l in enumerate(members)] + [(l, j, wide.probe_inputs, j) for j, l in enumerate(wide.probe_lanes)]
        for lane, row_of_probe, inputs, which in held:
            want = _named_lane(reference(inputs, which), base)
            for name, ref in want.items():
                if name.startswith(PROBE):
                    if inputs is pool:
                        continue
                    got = base[name][row_of_probe]
                elif name in base:
                    got = base[name][lane]
                else:
                    continue
                if ref.shape != got.shape:
                    raise LaneContractError("reference", f"lane {lane}, output {name!r}: shape {got.shape}, reference {ref.shape}")
                err = float(np.max(np.abs(got - ref))) if ref.size else 0.0
                if not err <= bound(name):
                    raise LaneContractError("reference", f"lane {lane}, output {name!r}: {err:.3g} from the reference, beyond {bound(name):g}")

    def compare(check, what, ref, got, rows, lanes_of_ref=None):
        """Rows `rows` (bool) of every output: got[l] against ref[l] (or ref[lanes_of_ref[l]])."""
        for name in ref:
            if name.startswith(PROBE) and lanes_of_ref is not None:
                continue
            a, b = ref[name], got[name]
            sel = np.ones(len(b), dtype=bool) if name.startswith(PROBE) else rows
            src = a if lanes_of_ref is None else a[lanes_of_ref]
            if name in rel_tol:                                                # the element that breaks the bound, as _compare reports it
                x, y = np.asarray(src).reshape(len(b), -1), np.asarray(b).reshape(len(b), -1)
                beyond = ~(np.abs(x - y) <= rel_tol[name] * np.maximum(np.abs(x), np.abs(y))) & sel[:, None]
                if beyond.any():
                    l, k = (int(v) for v in np.argwhere(beyond)[0])
                    raise LaneContractError(check, f"{what}: lane {l}, output {name!r}, flat element {k}: {x[l, k]!r} ({_bits(x[l, k])}) against "
                                                   f"{y[l, k]!r} ({_bits(y[l, k])}), beyond {rel_tol[name]:g} relative")
                continue
            if a.shape != b.shape or a.dtype != b.dtype:
                raise LaneContractError(check, f"{what}: output {name!r}, shape / dtype {a.shape} {a.dtype} against {b.shape} {b.dtype}")
            bad = _unequal_lanes(src, b) & sel
            if bad.any():
                _raise_first(check, what, name, a, b, bad, lanes_of_ref)

    again = named(run(wide))
    compare("R", "the same call again", base, again, np.ones(lanes, dtype=bool))
    del again
    compare("P", "a lane against lane l mod 7 of the same call", base, base, wide.pooled, np.array(members)[wide.member])
    return base


__all__ = ["POOL", "Wide", "LaneContractError", "check_wide", "probe_lanes"]
