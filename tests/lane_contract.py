"""The lane contract of the batched entry points, as one helper.

For a fixed call shape a lane's outputs are a function of that lane's inputs alone, and the same call gives the same bits.  Nothing
is claimed between different batch sizes.  `check_lanes` holds a callable `run(inputs) -> outputs` to that with four checks, each by
`np.array_equal` (so +0 and -0 are equal) unless an output is listed in `rel_tol`:

    R  repeat      the same call on fresh copies of the inputs, and every callable of `also`, give the same outputs
    P  position    a fixed permutation of the lanes that moves lane 0 and the last lane permutes the outputs the same way
    F  finite      every lane outside `probes` gets other finite inputs (`other`): the probe lanes' outputs stay
    N  poison      every lane outside `probes` gets NaN inputs (`poison`): the probe lanes' outputs stay

Before them three guards keep equality from being vacuous: the compared outputs are finite, the probe lanes' outputs are pairwise
different, and the lanes of `reference_lanes` agree with `reference(inputs, lane)` within `tol`.

`inputs` is a tuple or list of columns, or one column.  A column is an array with a leading lane axis or a list of per-lane objects
(such as DeviceMPS states); arrays are copied before every call, objects are handed on as they are.  `run` gets the same structure and
returns an array, a tuple or list of arrays, or a dict of arrays, each with a leading lane axis.

A failure raises LaneContractError, whose `.check` is one of "finite", "distinct", "reference", "R", "P", "F", "N" and whose text names
the lane, the output and the first differing element with both bit patterns.
"""
import numpy as np

CHECKS = ("R", "P", "F", "N")


class LaneContractError(AssertionError):
    def __init__(self, check, message):
        super().__init__(f"lane contract, check {check}: {message}")
        self.check = check


# ---- inputs: columns with a lane axis
def _split(inputs):
    """(columns, rebuild): the columns of `inputs` and the function that puts columns back into its structure."""
    if isinstance(inputs, np.ndarray):
        return [inputs], lambda cols: cols[0]
    if isinstance(inputs, tuple):
        return list(inputs), tuple
    if isinstance(inputs, list):
        if inputs and all(isinstance(e, (np.ndarray, list)) for e in inputs):
            return list(inputs), list
        return [inputs], lambda cols: cols[0]              # one column of per-lane objects
    raise TypeError("inputs must be an array, a list of per-lane objects, or a tuple / list of such columns")


def num_lanes(inputs):
    cols, _ = _split(inputs)
    counts = {len(c) for c in cols}
    if len(counts) != 1:
        raise ValueError(f"the columns disagree about the number of lanes: {sorted(counts)}")
    return counts.pop()


def take(inputs, lanes):
    """`inputs` with lane i of the result being lane lanes[i] of `inputs` (fresh arrays, fresh lists)."""
    cols, rebuild = _split(inputs)
    idx = [int(l) for l in lanes]
    return rebuild([np.ascontiguousarray(c[idx]) if isinstance(c, np.ndarray) else [c[i] for i in idx] for c in cols])


def fresh(inputs):
    return take(inputs, range(num_lanes(inputs)))


def substitute(inputs, donor, lanes):
    """`inputs` with the lanes of `lanes` taken from `donor` (the same structure and number of lanes)."""
    cols, rebuild = _split(fresh(inputs))
    dcols, _ = _split(donor)
    if len(cols) != len(dcols) or num_lanes(donor) != num_lanes(inputs):
        raise ValueError("the donor does not have the structure of the inputs")
    for c, d in zip(cols, dcols):
        for l in lanes:
            c[l] = d[l]
    return rebuild(cols)


def nan_filled(inputs, lanes):
    """`inputs` with every floating-point element of the lanes of `lanes` set to NaN.  Integer arrays (indices, counts: nothing that
    can hold a NaN, and an invalid index is not data) stay; a column of objects needs a recipe of its own."""
    cols, rebuild = _split(fresh(inputs))
    for c in cols:
        if not isinstance(c, np.ndarray):
            raise TypeError("the default poison fills floating-point arrays; give a `poison` recipe for columns of objects")
        if c.dtype.kind in "fc":
            c[list(lanes)] = np.nan
    return rebuild(cols)


def default_permutation(lanes):
    """A fixed permutation without a fixed point at lane 0 or at the last lane, and not a plain shift where the count allows it:
    lane i of the permuted call is lane (k i + 1) mod lanes of the original, k coprime to lanes near 0.618 lanes."""
    if lanes < 2:
        raise ValueError("a permutation needs two lanes")
    i = np.arange(lanes)
    k = max(1, int(0.618 * lanes))
    while np.gcd(k, lanes) != 1:
        k += 1
    perm = (k * i + 1) % lanes
    if perm[0] == 0 or perm[-1] == lanes - 1:
        perm = (i + 1) % lanes
    return perm


# ---- outputs: named arrays with a lane axis
def _named(outputs, lanes):
    if isinstance(outputs, dict):
        named = {str(k): np.asarray(v) for k, v in outputs.items()}
    elif isinstance(outputs, (tuple, list)):
        named = {f"out{i}": np.asarray(v) for i, v in enumerate(outputs)}
    else:
        named = {"out": np.asarray(outputs)}
    for name, arr in named.items():
        if arr.ndim < 1 or arr.shape[0] != lanes:
            raise ValueError(f"output {name} has shape {arr.shape}: no leading axis of {lanes} lanes")
    return named


def _bits(value):
    value = np.asarray(value)
    if value.dtype.kind == "c":
        return _bits(value.real) + " " + _bits(value.imag)
    return "0x" + value.tobytes()[::-1].hex()


def _first_difference(a, b):
    """None if a and b (one lane of one output) are equal by np.array_equal, else a description of the first differing element."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape / dtype {a.shape} {a.dtype} against {b.shape} {b.dtype}"
    if np.array_equal(a, b):
        return None
    fa, fb = a.reshape(-1), b.reshape(-1)
    k = int(np.flatnonzero(~(fa == fb))[0])
    where = np.unravel_index(k, a.shape) if a.ndim else ()
    return f"element {tuple(int(w) for w in where)}: {fa[k]!r} ({_bits(fa[k])}) against {fb[k]!r} ({_bits(fb[k])})"


def _compare(check, base, got, pairs, rel_tol, what):
    """For every (lane of base, lane of got) of `pairs`: every output equal, or within rel_tol[name] relative where one is given."""
    for name, ref in base.items():
        out = got[name]
        bound = rel_tol.get(name)
        for lb, lg in pairs:
            if bound is None:
                diff = _first_difference(ref[lb], out[lg])
                if diff is not None:
                    raise LaneContractError(check, f"{what}: lane {lb}, output {name!r}, {diff}")
            else:
                x, y = np.asarray(ref[lb], dtype=np.float64), np.asarray(out[lg], dtype=np.float64)
                bad = ~(np.abs(x - y) <= bound * np.maximum(np.abs(x), np.abs(y)))
                if np.any(bad):
                    k = int(np.flatnonzero(bad.reshape(-1))[0])
                    raise LaneContractError(check, f"{what}: lane {lb}, output {name!r}, flat element {k}: {x.reshape(-1)[k]!r} "
                                                   f"({_bits(x.reshape(-1)[k])}) against {y.reshape(-1)[k]!r} ({_bits(y.reshape(-1)[k])}), "
                                                   f"beyond {bound:g} relative")


def check_lanes(run, inputs, *, checks="RPFN", probes=None, other=None, poison=None, reference=None, reference_lanes=(0,), tol=None,
                also=(), permutation=None, rel_tol=None, distinct=None, compare_lanes=None):
    """Hold `run` to the lane contract on `inputs`; returns the named outputs of the clean call.

    checks           the subset of "RPFN" that applies
    probes           the lanes F and N keep; default (0, middle, last), of three lanes (0, last)
    other, poison    the inputs of the F / N call: a donor (the structure of `inputs`; the lanes outside `probes` are taken from it)
                     or a callable (inputs, lanes) -> inputs.  `poison` defaults to NaN in every element of those lanes
    reference        (inputs, lane) -> that lane's outputs in the structure `run` returns, without the lane axis; with `tol`
    also             further callables that must give the outputs of `run` (R), such as the same call on a fresh object
    rel_tol          {output: relative bound} for the outputs that are not compared exactly
    distinct         the outputs that must differ between any two probe lanes; default: every floating-point output
    compare_lanes    the lanes R and P compare; default all (a count past the grid checks its probes only)
    """
    checks = tuple(c for c in CHECKS if c in checks)
    lanes = num_lanes(inputs)
    rel_tol = dict(rel_tol or {})
    if probes is None:
        probes = sorted({0, lanes // 2, lanes - 1}) if lanes > 3 else [0, lanes - 1]    # (three lanes: the middle one is the neighbour)
    probes = [int(p) for p in probes]
    if len(set(probes)) != len(probes) or min(probes) < 0 or max(probes) >= lanes:
        raise ValueError(f"bad probe lanes {probes} of {lanes}")
    others = [l for l in range(lanes) if l not in set(probes)]
    if ("F" in checks or "N" in checks) and not others:
        raise ValueError("F and N need lanes outside the probes")
    if "F" in checks and other is None:
        raise ValueError("F needs the recipe `other`")
    held = list(range(lanes)) if compare_lanes is None else [int(l) for l in compare_lanes]

    base = _named(run(fresh(inputs)), lanes)

    # guards
    seen = sorted(set(held) | set(probes))
    for name, arr in base.items():
        if arr.dtype.kind in "fc":
            for l in seen:
                if not np.all(np.isfinite(arr[l])):
                    raise LaneContractError("finite", f"lane {l}, output {name!r} is not finite")
    names = [n for n, a in base.items() if a.dtype.kind in "fc"] if distinct is None else list(distinct)
    for name in names:
        for i, p in enumerate(probes):
            for q in probes[i + 1:]:
                if np.array_equal(base[name][p], base[name][q]):
                    raise LaneContractError("distinct", f"probe lanes {p} and {q} have the same output {name!r}")
    if reference is not None:
        if tol is None:
            raise ValueError("a reference needs its tolerance")
        for l in reference_lanes:
            want = _named_lane(reference(inputs, l), base)
            for name, ref in want.items():
                got = base[name][l]
                if ref.shape != got.shape:
                    raise LaneContractError("reference", f"lane {l}, output {name!r}: shape {got.shape}, reference {ref.shape}")
                err = float(np.max(np.abs(got - ref))) if ref.size else 0.0
                if not err <= tol:
                    raise LaneContractError("reference", f"lane {l}, output {name!r}: {err:.3g} from the reference, beyond {tol:g}")

    if "R" in checks:
        for k, again in enumerate((run,) + tuple(also)):
            got = _named(again(fresh(inputs)), lanes)
            _compare("R", base, got, [(l, l) for l in held], rel_tol, "the same call again" if k == 0 else f"the same call, variant {k}")
    if "P" in checks:
        perm = default_permutation(lanes) if permutation is None else np.asarray(permutation)
        if sorted(perm.tolist()) != list(range(lanes)) or perm[0] == 0 or perm[-1] == lanes - 1:
            raise ValueError("the permutation must move lane 0 and the last lane")
        got = _named(run(take(inputs, perm)), lanes)
        where = {int(perm[i]): i for i in range(lanes)}
        _compare("P", base, got, [(l, where[l]) for l in held], rel_tol, "lanes permuted")
    for check, recipe, what in (("F", other, "other finite neighbours"), ("N", poison, "NaN neighbours")):
        if check not in checks:
            continue
        if recipe is None:
            changed = nan_filled(inputs, others)
        elif callable(recipe):
            changed = recipe(fresh(inputs), list(others))
        else:
            changed = substitute(inputs, recipe, others)
        if num_lanes(changed) != lanes:
            raise ValueError(f"the recipe of {check} changed the number of lanes")
        got = _named(run(changed), lanes)
        _compare(check, base, got, [(p, p) for p in probes], rel_tol, what)
    return base


def _named_lane(outputs, base):
    """The reference's outputs of one lane under the names of `base`; a reference may give fewer outputs than the call."""
    if isinstance(outputs, dict):
        return {str(k): np.asarray(v) for k, v in outputs.items()}
    if isinstance(outputs, (tuple, list)) and not (len(base) == 1 and "out" in base):
        return {f"out{i}": np.asarray(v) for i, v in enumerate(outputs) if v is not None}
    return {"out": np.asarray(outputs)}
