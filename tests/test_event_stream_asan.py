"""tests/c/event_stream_asan.cpp: the streaming event detector of the host library under ASan + UBSan, as a stand-alone program
(CPU build only -- the GPU pool runs no sanitizers, and nothing loaded into Python is checked this way)."""
import os
import shutil
import subprocess

import pytest

from tests.util import ROOT


def test_event_stream_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "sigfish_amd", "csrc")
    exe = str(tmp_path / "event_stream_asan")
    units = [os.path.join(csrc, u) for u in ("sfa_host.cpp", "host/blow5.cpp", "host/inflate.cpp", "host/events.cpp", "host/refio.cpp", "host/sam.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
                            "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "event_stream_asan.cpp"), *units, "-lz", "-lpthread"],
                           capture_output=True, timeout=600)
    if build.returncode != 0 and b"sanitize" in build.stderr:
        pytest.skip("toolchain without sanitizer runtimes")
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    run = subprocess.run([exe], capture_output=True, timeout=300)
    assert run.returncode == 0 and b"30 runs, 0 failures" in run.stdout, (run.stdout + run.stderr).decode()[-3000:]
    assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]
