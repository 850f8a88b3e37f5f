"""Event maps of rows beyond 2048 events in row strips ("map_strips"), the parts that need no GPU: the stand-alone program
tests/c/map_strips.cpp, built with -Wall -Werror and once more under ASan + UBSan.  It checks plan_map_slices_strips (sfa_plan.hpp)
and, with a plain C++ model of the strip fill and the walk through the strips, that handing the bottom row of one strip to the
next as its boundary gives the path of band_traceback and the pairs of path_to_pairs over the whole query (host/sam.cpp).  The byte
counts it prints are compared with the formula as this file states it."""
import os
import shutil
import subprocess

import pytest

from tests.util import ROOT

CSRC = os.path.join(ROOT, "sigfish_amd", "csrc")


def _build(tmp, sanitize):
    exe = str(tmp / ("map_strips_san" if sanitize else "map_strips"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "c", "map_strips.cpp"), os.path.join(CSRC, "host", "sam.cpp")]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """[lines of the plain build, lines of the sanitizer build or None]"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("map_strips")
    exe, build = _build(tmp, False)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    san, build = _build(tmp, True)
    # (the plain build went through, so the source compiles; only a toolchain that says its sanitizer runtime is missing counts as without)
    if build.returncode != 0 and any(m in build.stderr for m in (b"libasan", b"libubsan", b"-lasan", b"-lubsan", b"unrecognized command-line option", b"unsupported option")):
        san = None
    else:
        assert build.returncode == 0, build.stderr.decode()[-2000:]
    outs = []
    for prog in (exe, san):
        if prog is None:
            outs.append(None)
            continue
        run = subprocess.run([prog], capture_output=True, timeout=600)
        assert run.returncode == 0, (run.returncode, (run.stdout + run.stderr).decode()[-3000:])
        assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]
        outs.append(run.stdout.decode().splitlines())
    return outs


def test_both_builds_print_the_same_lines(outputs):
    if outputs[1] is None:
        pytest.skip("toolchain without sanitizer runtimes")
    assert outputs[0] == outputs[1]


def test_no_check_failed(outputs):
    assert not [ln for ln in outputs[0] if ln.startswith("FAIL")]
    assert outputs[0][-1] == "done 0"


def test_byte_counts_of_long_rows(outputs):
    """ceil(qlen / 2048) strips, each (m + 63) records of 64 x 2 words; two hand-over rows of m floats on top, which count."""
    got = {tuple(int(v) for v in ln.split()[1:3]): tuple(int(v) for v in ln.split()[3:]) for ln in outputs[0] if ln.startswith("bytes ")}
    assert sorted(got) == [(q, m) for q in (2049, 4096, 4097) for m in (1, 5000)]
    for (qlen, m), (strips, moves, row) in got.items():
        n = -(-qlen // 2048)
        assert strips == n == {2049: 2, 4096: 2, 4097: 3}[qlen]
        assert moves == n * (m + 63) * 512
        assert row == moves + 2 * 4 * m


def test_the_model_cases_cover_the_hand_over(outputs):
    """Every case agreed with the host routine, and the cases do exercise the hand-over: walks that go below the first strip, cross a
    strip edge on a diagonal move, and (bands narrower than the query is long) end behind the first column."""
    rows = [dict(zip(ln.split()[1::2], ln.split()[2::2])) | {"verdict": ln.split()[-1]} for ln in outputs[0] if ln.startswith("model ")]
    assert len(rows) == 4 * 2 * 4
    assert {(int(r["n"]), int(r["std"])) for r in rows} == {(n, s) for n in (2049, 2080, 4096, 4097) for s in (0, 1)}
    assert {r["band"] for r in rows} == {"0..499", "2500..2999", "1000..1036", "0..2999"}  # from column 0, to the last column, m < 64
    assert all(r["verdict"] == "ok" for r in rows)
    assert all(int(r["below"]) > 0 for r in rows)
    assert sum(int(r["diag_cross"]) > 0 for r in rows) >= 8
    assert any(int(r["first_col"]) > 0 for r in rows) and any(int(r["first_col"]) == 0 for r in rows)


def test_option_is_named_in_the_header():
    header = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    assert '"map_strips"' in header
    assert "there is no device route beyond" not in header


def test_strip_kernels_use_no_scratch():
    """No spill in the strip fill nor in the walk through the strips: the shipped ISA holds no scratch access."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check as I
    from sigfish_amd import _lib
    if not I.objdump():
        pytest.skip("no llvm-objdump")
    funcs = I.disassemble(_lib.LIB_PATH)
    mine = {n: ins for n, ins in funcs.items() if "sdtw_path_strip_kernel" in n or "sdtw_path_walk_strips_kernel" in n}
    assert len(mine) == 5, sorted(mine)  # (subsequence, std_dtw) x (strip 0, strips below) + the walk
    for name, ins in mine.items():
        assert not any(i.startswith("scratch_") for i, _ in ins), name
