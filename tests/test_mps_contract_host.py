"""CPU-only: csrc/aqc_mps_contract.h, the transfer-matrix site steps and the overlap chain of the single-lane MPS side -- the stand-alone
self-test (tests/native/mps_contract_selftest.cpp: a CPU executor against dense vectors) built by g++ under ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_site_steps_and_overlap_chain_selftest_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "mps_contract_selftest")
    out = subprocess.run(["g++", "-std=c++17", "-Wall", *SAN, os.path.join(ROOT, "tests", "native", "mps_contract_selftest.cpp"), "-o", exe],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stderr
