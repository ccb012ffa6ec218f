"""Host only: the one table of run-time switches (include/aqc_switches.def) is complete, is the only reader of the environment,
and names every ``AQC_*`` variable that the tests, the tools and the benchmark set."""
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every switch in use when the table was written, by reader and time of reading
CREATE = """AQC_KERNEL_FAMILY AQC_KERNEL_V2 AQC_LOW_BITS AQC_TILE_BITS_APPLY AQC_TILE_BITS_SWEEP AQC_THREADS AQC_SWEEP_REG_BITS
AQC_MIRROR_PLAN AQC_VERBOSE AQC_SPARSE_SWEEP AQC_SPARSE_MIN_ITEMS AQC_LAZY_Z AQC_R_ONLY_LAST AQC_R_ONLY_MAX_SUBS AQC_SKIP_ZERO_W
AQC_GRADS_DIRECT AQC_UBUILD_MIRROR AQC_UBUILD_SUBSET AQC_PROJECTED AQC_PROJECTED_BEAM AQC_PROJECTED_VDAG AQC_PROJECTED_VDAG_MIN_ELEMS
AQC_PROJECTED_FUSED AQC_PROJECTED_FUSED_WGS AQC_PROJECTED_FUSED_MAX_SHARES AQC_PROJECTED_FUSED_QB AQC_PROJECTED_PAIRS AQC_GRAPH
AQC_SWEEP_GRID AQC_APPLY_PERSIST AQC_STAMPS AQC_DEBUG_SKIP""".split()
CALL = "AQC_CD_CHAIN AQC_SVD_BLOCKED AQC_SVD_DEBUG AQC_DEVICE AQC_COMM_TIMEOUT_S AQC_COMM_INIT_TIMEOUT_S".split()
PYTHON = {"AQC_HIP_LIB": "import", "AQC_MPS_APPLY": "call", "AQC_MPS_METHOD": "call", "AQC_LOCKSTEP_SURROGATE_EVAL": "call",
          "AQC_COMM_FILE": "call", "AQC_COMM_TAG": "call"}


def _table():
    from aqc_research_amd.switches import table

    return {row["name"]: row for row in table()}


def _text_files(*patterns):
    for pattern in patterns:
        for path in sorted(glob.glob(os.path.join(ROOT, pattern), recursive=True)):
            if os.path.isfile(path):
                raw = open(path, "rb").read()
                if b"\0" not in raw:   # (a built library or object file is not text)
                    yield os.path.relpath(path, ROOT), raw.decode("utf-8", "replace")


def test_listing_enumerates_and_the_module_prints_every_name():
    from aqc_research_amd import _lib

    rows = _table()
    L = _lib.lib()
    assert L.aqc_switch_info(len(rows), None, None, None, None, None) == 1 and L.aqc_switch_info(-1, None, None, None, None, None) == 1
    assert L.aqc_switch_info(0, None, None, None, None, None) == 0
    for row in rows.values():
        assert row["when"] in ("import", "create", "call") and row["reader"] in ("c", "python") and row["default"] and row["doc"], row
    out = subprocess.run([sys.executable, "-m", "aqc_research_amd.switches"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    printed = re.findall(r"^(AQC_[A-Z0-9_]+)\b", out.stdout, re.M)
    assert printed == list(rows)


def test_table_covers_the_switches_in_use():
    rows = _table()
    assert len(CREATE) == 32 and len(set(CREATE) | set(CALL) | set(PYTHON)) == 44
    assert set(rows) == set(CREATE) | set(CALL) | set(PYTHON), set(rows) ^ (set(CREATE) | set(CALL) | set(PYTHON))
    for name in CREATE:
        assert (rows[name]["when"], rows[name]["reader"]) == ("create", "c"), name
    for name in CALL:
        assert (rows[name]["when"], rows[name]["reader"]) == ("call", "c"), name
    for name, when in PYTHON.items():
        assert (rows[name]["when"], rows[name]["reader"]) == (when, "python"), name
    for name in ("AQC_STAMPS", "AQC_DEBUG_SKIP", "AQC_SVD_DEBUG"):
        assert "-DAQC_TUNING" in rows[name]["doc"], name
    assert "AQC_KERNEL_FAMILY" in rows["AQC_KERNEL_V2"]["doc"]


def test_the_environment_is_read_in_one_place():
    """``getenv(`` occurs in csrc/aqc_switches.h only, and every ``AQC_*`` name the package's Python files quote -- which includes every
    one they look up in ``os.environ`` -- is a line of the table."""
    readers = [path for path, text in _text_files("aqc_research_amd/**/*") if "getenv(" in text]
    assert readers == [os.path.join("aqc_research_amd", "csrc", "aqc_switches.h")], readers
    rows = _table()
    quoted = {(path, name) for path, text in _text_files("aqc_research_amd/**/*.py")
              for name in re.findall(r"""["'](AQC_[A-Z0-9_]+)["']""", text)}
    assert {name for _, name in quoted} >= set(PYTHON), "the pattern no longer finds the package's own reads"
    unknown = sorted((path, name) for path, name in quoted if name not in rows)
    assert not unknown, unknown


def test_no_test_tool_or_benchmark_sets_a_name_that_selects_nothing():
    """Every ``AQC_*`` name quoted or assigned (``NAME=``) in the tests, the tools and bench.py is a switch of the table, a constant of
    include/aqc_hip.h, or belongs to the benchmark's and the probes' own variables."""
    rows = _table()
    header = open(os.path.join(ROOT, "include", "aqc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header, flags=re.S)
    constants = set(re.findall(r"\bAQC_[A-Z0-9_]+\b", code))
    assert "AQC_BUF_X" in constants and not constants & set(rows)
    own = ("AQC_BENCH_", "AQC_PROBE_", "AQC_PROF_")
    seen, unknown = set(), []
    for path, text in _text_files("tests/**/*.py", "tools/*", "bench.py"):
        for name in re.findall(r"""["'](AQC_[A-Z0-9_]+)["']""", text) + re.findall(r"\b(AQC_[A-Z0-9_]+)=", text):
            seen.add(name)
            if not (name in rows or name in constants or name.startswith(own) or name == "AQC_REFERENCE"):
                unknown.append((path, name))
    assert "AQC_SPARSE_MIN_ITEMS" in seen and "AQC_KERNEL_FAMILY" in seen, "the pattern no longer finds the names the tests set"
    assert not unknown, sorted(set(unknown))
