"""Recalibration of raw sessions without a GPU (csrc/recal_rule.hpp, sfa_session_raw_recalibrate, `realtime --recalibrate`):
  * the window rule as a stand-alone C++ program (tests/c/recal_window.cpp, the header the device kernel, the library and the
    command line include) against the Python twin (api.recal_window): every q_avail in 0..80, both values of `ended`, four
    configurations; the same for the expansion of "double" and for the lists that must be refused;
  * every bad --recalibrate list exits non-zero with its message before anything touches a device (there is none here, so a
    device call would be the error reported instead);
  * the new symbol is declared, listed and exported, and sfa_session_raw_info_t kept its size and offsets."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import sigfish_amd as S
from sigfish_amd import _lib
from tests.realtime_util import BIN, write_model
from tests.util import GOLD, ROOT

NORM, QUERY, AT = 25, 70, (30, 40, 70)
CONFIGS = [("none", (), False), ("at", AT, False), ("at_end", (), True), ("both", AT, True)]
SHAPES = [(25, 250), (25, 70), (30, 70), (100, 2048), (64, 70), (70, 70), (25, 26), (25, 50), (25, 51), (1000, 1024), (25, 1 << 30), (1, 1 << 30)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("recal") / "recal_window")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "recal_window.cpp")]
    build = subprocess.run(cmd[:4] + ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] + cmd[4:], capture_output=True, timeout=600)
    if build.returncode != 0 and b"sanitize" in build.stderr:  # a toolchain without sanitizer runtimes: the table is what is tested
        build = subprocess.run(cmd, capture_output=True, timeout=600)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    run = subprocess.run([exe] + [f"{n}:{q}" for n, q in SHAPES], capture_output=True, timeout=120)
    assert run.returncode == 0 and b"runtime error" not in run.stderr and b"AddressSanitizer" not in run.stderr, (run.stdout + run.stderr).decode()[-3000:]
    return run.stdout.decode().splitlines()


def test_window_table_equals_the_python_rule(program):
    want = []
    for name, at, at_end in CONFIGS:
        for ended in (0, 1):
            ws = [S.recal_window(min(q, QUERY), bool(ended), NORM, QUERY, at, at_end) for q in range(81)]
            want.append(f"window {name} ended={ended}: " + " ".join(str(w) for w in ws))
    got = [ln for ln in program if ln.startswith("window ")]
    assert got == want
    # the table says what the rule is for (checked on the Python side, which the lines above tie to the C++ one)
    rule = lambda q, ended, at, at_end: S.recal_window(q, ended, NORM, QUERY, at, at_end)  # noqa: E731
    assert [rule(q, False, (), False) for q in (0, 24, 25, 69, 70)] == [0, 0, 25, 25, 25]  # nothing configured: frozen at norm
    assert [rule(q, False, AT, False) for q in (24, 25, 29, 30, 39, 40, 69, 70)] == [0, 25, 25, 30, 30, 40, 40, 70]
    assert [rule(q, True, (), True) for q in (24, 25, 26, 69, 70)] == [0, 25, 26, 69, 25]  # the short window of an ended read only
    assert [rule(q, True, AT, True) for q in (24, 33, 69, 70)] == [0, 33, 69, 70] and rule(33, False, AT, True) == 30
    for _, at, at_end in CONFIGS:  # W never shrinks while a read grows, nor when it ends where it is
        for q in range(80):
            assert rule(min(q + 1, QUERY), False, at, at_end) >= rule(min(q, QUERY), False, at, at_end)
            assert rule(min(q, QUERY), True, at, at_end) >= rule(min(q, QUERY), False, at, at_end)


def test_double_expands_identically(program):
    got = [ln for ln in program if ln.startswith("double ")]
    want = [f"double {n}:{q}:" + "".join(f" {w}" for w in S.recal_double(n, q)) for n, q in SHAPES]
    assert got == want
    assert S.recal_double(25, 250) == (50, 100, 200, 250) and S.recal_double(25, 50) == (50,) and S.recal_double(70, 70) == ()
    assert S.recal_double(64, 70) == (70,) and len(S.recal_double(25, 1 << 30)) <= 32 and len(S.recal_double(1, 1 << 30)) <= 32


def test_list_checks_of_the_shared_header(program):
    assert program[-1] == "refused not_ascending=1 twice=1 at_norm=1 above=1 many=1 empty=0 full=0"


REFUSED = [(["--norm-events", "25", "-q", "70", "--recalibrate", "40,30,70"], "ascend"), (["--norm-events", "25", "-q", "70", "--recalibrate", "40,40"], "ascend"),
           (["--norm-events", "30", "-q", "70", "--recalibrate", "30,50"], "above the calibration window"), (["--norm-events", "30", "-q", "70", "--recalibrate", "29"], "above the calibration window"),
           (["--norm-events", "25", "-q", "70", "--recalibrate", "40,71"], "above the query size"), (["--recalibrate", "250"], "above the calibration window"),
           (["--norm-events", "25", "-q", "70", "--recalibrate", ",".join(str(26 + k) for k in range(33))], "more than 32 points"),
           (["--norm-events", "25", "--recalibrate", "x"], "takes 'double' or a comma separated list"), (["--norm-events", "25", "--recalibrate", "50,"], "takes 'double' or a comma separated list")]


@pytest.mark.parametrize("extra,msg", REFUSED, ids=["not_ascending", "twice", "at_norm", "below_norm", "above_q", "default_norm_is_q", "33_points", "not_a_number", "trailing_comma"])
def test_bad_lists_exit_before_any_device_call(extra, msg, tmp_path):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    model = write_model(tmp_path / "syn.model", 6)
    files = [os.path.join(GOLD, "data", "nCoV-2019.reference.fasta"), os.path.join(GOLD, "data", "sp1_dna.blow5")]
    r = subprocess.run([BIN, "realtime", "--kmer-model", model, *extra, "--recalibrate-at-end", *files], capture_output=True, timeout=60)
    err = r.stderr.decode()
    assert r.returncode not in (0, None) and r.returncode > 0 and r.stdout == b"", (r.returncode, err)
    assert err.count("[sigfish-amd] ERROR:") == 1 and "--recalibrate" in err and msg in err, err
    assert "accelerator" not in err and "hip" not in err.lower(), err


def test_help_names_the_options():
    r = subprocess.run([BIN, "realtime", "--help"], capture_output=True, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0 and "--recalibrate LIST|double" in out and "--recalibrate-at-end" in out


def test_abi_symbol_and_info_struct(tmp_path):
    header = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    assert "int sfa_session_raw_recalibrate(sfa_session_t *s, const int32_t *at, int32_t n_at, uint32_t flags);" in header
    assert "#define SFA_RECAL_AT_END 0x1" in header and S.RECAL_AT_END == 1 and S.RAW_RECALIBRATED == 16
    assert "sfa_session_raw_recalibrate" in _lib.SYMBOLS
    getattr(_lib.load(), "sfa_session_raw_recalibrate")  # exported
    # the struct as a C compiler lays it out from the header: 40 bytes, norm_window where pad was
    exe, src = str(tmp_path / "layout"), str(tmp_path / "layout.c")
    with open(src, "w") as f:
        f.write('#include <stddef.h>\n#include <stdio.h>\n#include "sigfish_amd.h"\nint main(void) { printf("%d %d %d %d %d\\n", (int)sizeof(sfa_session_raw_info_t), '
                "(int)offsetof(sfa_session_raw_info_t, q_events), (int)offsetof(sfa_session_raw_info_t, norm_mean), (int)offsetof(sfa_session_raw_info_t, status), "
                "(int)offsetof(sfa_session_raw_info_t, norm_window)); return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["40", "16", "24", "32", "36"]
    assert C.sizeof(_lib.SfaSessionRawInfo) == 40 and _lib.SfaSessionRawInfo.norm_window.offset == 36
    assert S.SESSION_RAW_INFO_DTYPE.itemsize == 40 and S.SESSION_RAW_INFO_DTYPE.fields["norm_window"][1] == 36
    assert S.SESSION_RAW_INFO_DTYPE.fields["status"][1] == 32


def test_schedules_of_the_gpu_test_reach_every_case():
    """tests/test_session_recal_gpu.py builds its schedules from event counts of the host detector: that every case it names
    occurs is a statement about its inputs, checked here without a GPU"""
    import numpy as np

    from tests import test_session_recal_gpu as G
    twins, seen = G.run_plan(G.build_plan(np.random.default_rng(8)), G.SHAPE, G.AT, True)
    assert seen == G.CASES, G.CASES - seen
    assert twins[9].window == 0 and twins[3].window == twins[3].q_avail() and twins[11].window == 70


def test_at_end_adds_the_query_size_to_the_replay_points():
    """--recalibrate-at-end is about the line a read ends with: the replay (command line and Python twin) hands its session q as
    the last point, unless it is already, or no window longer than norm exists"""
    from sigfish_amd.realtime import recal_points
    assert recal_points(64, 70, (), True) == (70,) and recal_points(25, 70, (35,), True) == (35, 70) and recal_points(25, 70, (35, 70), True) == (35, 70)
    assert recal_points(70, 70, (), True) == () and recal_points(25, 70, (35,), False) == (35,) and recal_points(25, 250, "double", True) == (50, 100, 200, 250)
    assert recal_points(25, 250, "double", False) == S.recal_double(25, 250) and recal_points(25, 70) == ()
