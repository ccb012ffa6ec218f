"""CPU-only: csrc/aqc_backwalk.h, the map from a mirrored sub-stage of the backward walk to the partial-R row of the forward sub-stage
it mirrors -- the stand-alone self-test (tests/native/backwalk_selftest.cpp) built by g++ under ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_r_slot_map_selftest_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "backwalk_selftest")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", *SAN, os.path.join(ROOT, "tests", "native", "backwalk_selftest.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stderr
