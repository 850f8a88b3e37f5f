"""The host rules of a session's group cap without a GPU: the stand-alone program tests/c/group_cover_rules.cpp, built from
sigfish_amd/csrc/group_cover_rules.hpp with -Wall -Werror and once more under ASan + UBSan, against the numpy model of
tests/group_cover_model.py -- live labels, the lowest column of every live label, the depth record of every entry -- for DNA (two
strands) and RNA (one), with non-zero offsets, contigs of 1 .. 7 k-mers, two contigs of odd length (the second job starts at an
odd column), n_groups 1, 31, 32, 33 and 1023, overlapping groups whose lower id is capped, depth cap - 1 beside depth cap, an
empty group; and the three new symbols of the C ABI."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib
from tests import group_cover_model as M
from tests.util import ROOT


def _build(tmp, sanitize):
    exe = str(tmp / ("group_cover_rules_san" if sanitize else "group_cover_rules"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "group_cover_rules.cpp")]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """[plain build, sanitizer build or None]: every request goes through all of them, and their answers must be the same lines"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("group_cover_rules")
    exe, build = _build(tmp, False)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    san, build = _build(tmp, True)
    if build.returncode != 0 and any(m in build.stderr for m in (b"libasan", b"libubsan", b"-lasan", b"-lubsan", b"unrecognized command-line option", b"unsupported option")):
        san = None
    else:
        assert build.returncode == 0, build.stderr.decode()[-2000:]
    return [exe, san]


def _ask(programs, text):
    outs = []
    for exe in programs:
        if exe is None:
            continue
        run = subprocess.run([exe], input=text.encode(), capture_output=True, timeout=300)
        assert run.returncode == 0, (run.returncode, (run.stdout + run.stderr).decode()[-3000:])
        assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]
        outs.append(run.stdout.decode().splitlines())
    assert all(o == outs[0] for o in outs)
    return outs[0]


def _request(strands, lens, offs, n_groups, cap, targets, intervals):
    return (f"labels {strands} {len(lens)} " + " ".join(f"{n} {o}" for n, o in zip(lens, offs)) + f" {n_groups} {cap} {len(targets)} "
            + " ".join(f"{c} {b} {e} {g}" for c, b, e, g in targets) + f" {len(intervals)} " + " ".join(f"{c} {b} {e}" for c, b, e in intervals) + "\n")


def test_selftest_plain_and_under_sanitizers(programs):
    line = _ask(programs, "selftest\n")[-1].split()
    assert line[:2] == ["selftest", "ok"] and int(line[2]) == 33  # 16 checks with one strand, 17 with two


def test_the_program_runs_under_sanitizers(programs):
    if programs[1] is None:
        pytest.skip("toolchain without sanitizer runtimes")
    got = _ask(programs[1:], _request(2, [5], [0], 1, 1, [(0, 1, 4, 0)], [(0, 2, 3)]))
    # '+' columns 0..4 are coordinates 0..4, '-' columns 5..9 are coordinates 5..1: coordinate 2 closes column 2 and column 8
    assert got == ["live 4 1 0 1 0 1 1 1 0 1 0", "first 1 0", "rec 0 3 1 1 0 1", "rec 1 2 0 0 0 0", "base 1 0 0 0 1 1 1 0 0 0", "open 1 0"]


# ---- the header against the numpy model ----
LENS = [1, 2, 3, 4, 5, 6, 7, 31, 33, 70]  # contigs of 1 .. 7 k-mers; 31 and 33 are odd: with one strand the job behind them starts at an odd column
OFFS = [0, 3, 0, 9, 1, 0, 2, 7, 100, 1000]
whole = lambda r, g: (r, OFFS[r], OFFS[r] + LENS[r] + 1, g)


def single_columns(n_groups):
    """group g is ONE coordinate: the coordinates of contigs 7 .. 9 and then of the short ones, in turn, as far as n_groups goes"""
    coords = [(r, OFFS[r] + k) for r in (9, 8, 7, 6, 5, 4, 3, 2, 1, 0) for k in range(LENS[r] + 1)]
    return [(r, x, x + 1, g % n_groups) for g, (r, x) in enumerate(coords[:max(n_groups, 40)])]


CASES = {
    # name: (n_groups, cap, targets, intervals)
    "nothing added": (3, 2, [whole(7, 0), whole(8, 1), (9, 1010, 1040, 2), whole(0, 2), whole(3, 1)], []),
    "one group": (1, 1, [whole(r, 0) for r in range(10)], [(9, 1000, 1001), (9, 1070, 1071), (8, 100, 134), (0, 0, 1), (0, 1, 2), (1, 3, 4)]),
    "cap - 1 and cap side by side": (2, 3, [whole(8, 0), whole(9, 1)], [(8, 110, 120)] * 2 + [(8, 115, 125)] + [(9, 1000, 1071)] * 2 + [(9, 1010, 1011)]),
    "overlapping groups, the lower capped": (4, 1, [(9, 1005, 1030, 1), (9, 1020, 1050, 3), (8, 100, 134, 2), (8, 110, 120, 0), (6, 2, 10, 3), (6, 4, 6, 1)],
                                             [(9, 1015, 1025), (8, 112, 116), (6, 4, 5)]),
    "an empty group and one without live columns": (5, 1, [whole(7, 0), (8, 100, 110, 2), (5, 0, 7, 4)], [whole(7, 0)[:3], (5, 0, 7)]),
    "31 groups": (31, 2, single_columns(31), [(9, 1000, 1071), (9, 1000, 1020), (8, 100, 134), (8, 120, 134), (7, 7, 39)]),
    "32 groups": (32, 2, single_columns(32), [(9, 1000, 1071), (9, 1031, 1033), (8, 100, 134)]),
    "33 groups": (33, 2, single_columns(33), [(9, 1000, 1071), (9, 1031, 1034), (9, 1000, 1001)]),
    "1023 groups": (1023, 1, [(9, 1000 + (g % 71), 1001 + (g % 71), g) for g in range(1023)] + [whole(8, 1022)], [(9, 1003, 1009), (8, 101, 102)]),
    "below the offset": (2, 1, [whole(8, 0), whole(3, 1)], [(8, 0, 101), (3, 0, 9), (9, 5, 1000)]),
}


@pytest.mark.parametrize("strands", [1, 2], ids=["rna_one_strand", "dna_two_strands"])
@pytest.mark.parametrize("name", list(CASES))
def test_live_labels_firsts_and_records_equal_the_models(programs, name, strands):
    n_groups, cap, targets, intervals = CASES[name]
    lines = _ask(programs, _request(strands, LENS, OFFS, n_groups, cap, targets, intervals))
    model = M.GroupCover(LENS, OFFS, strands, n_groups, targets, cap)
    model.add(intervals)
    live, base = model.live_labels(), model.base_labels()
    assert lines[0].split()[0] == "live" and int(lines[0].split()[1]) == int((live != n_groups).sum())
    assert [int(x) for x in lines[0].split()[2:]] == live.tolist(), name
    assert [int(x) for x in lines[1].split()[1:]] == model.firsts().tolist(), name
    rec = model.records()
    for e in range(n_groups + 1):
        assert lines[2 + e].split() == ["rec", str(e)] + [str(int(rec[e][f])) for f in ("columns", "capped", "depth_sum", "depth_min", "depth_max")], (name, e)
    assert [int(x) for x in lines[3 + n_groups].split()[1:]] == base.tolist(), name
    # open_first_cols fed with the LIVE firsts, every even group open: the lowest live column of either class
    on = [c for c in range(model.total) if live[c] != n_groups and live[c] % 2 == 0]
    off = [c for c in range(model.total) if live[c] == n_groups or live[c] % 2 == 1]
    assert lines[4 + n_groups].split() == ["open", str(on[0] if on else -1), str(off[0] if off else -1)], name
    # what the cases claim to reach
    if name == "nothing added":
        assert np.array_equal(live, base)
    if name == "cap - 1 and cap side by side":
        d = model.depth[8]
        assert d[14] == 2 and d[15] == 3 and rec[0]["capped"] == 5 and rec[0]["depth_max"] == 3 and rec[1]["capped"] == 1 and rec[1]["depth_min"] == 2
    if name == "overlapping groups, the lower capped":
        at = next(a for c, s, a in model.jobs if c == 9 and s == "+")
        assert base[at + 22] == 1 and live[at + 22] == n_groups and live[at + 26] == 1 and live[at + 32] == 3  # capped under 1 and 3: the background, not 3
    if name == "an empty group and one without live columns":
        f = model.firsts()
        assert rec[1]["columns"] == 0 and rec[1]["depth_min"] == 2 ** 32 - 1 and f[1] == M.NO_COLUMN and f[0] == M.NO_COLUMN and rec[0]["capped"] == rec[0]["columns"] == 31
    if name in ("31 groups", "32 groups", "33 groups"):
        assert (rec["columns"][:n_groups] > 0).all()  # every entry of the tables is used
    if name == "1023 groups":  # 71 coordinates for 1023 groups: the lowest id of each coordinate has it (group 70's is the one only a reverse row reports), the last entry is contig 8's
        assert (rec["columns"][:70] == 1).all() and (rec["columns"][70:1022] == 0).all() and rec[1022]["columns"] == 33 and live.max() == 1023
    if name == "below the offset":
        assert model.depth[8][0] == 1 and model.depth[8][1:].sum() == 0 and model.depth[3].sum() == 0 and model.depth[9].sum() == 0
    # the model's open pieces as group targets give the live table back as a BASE table (nothing added, through the header's group_labels)
    pieces = model.open_pieces()
    if pieces:
        again = _ask(programs, _request(strands, LENS, OFFS, n_groups, 1, pieces, []))
        assert again[3 + n_groups].split()[1:] == lines[0].split()[2:], name


def test_list_errors_come_first(programs):
    line = _ask(programs, _request(2, LENS, OFFS, 2, 1, [whole(8, 0), (8, 100, 101, 2)], []))[0]
    assert line.startswith("refused target 1:") and "group 2 out of range" in line
    line = _ask(programs, _request(2, LENS, OFFS, 2, 1, [whole(8, 0)], [(8, 100, 101), (8, 100, 136)]))[0]
    assert line.startswith("refused target 1:") and "beyond" in line


# ---- the C ABI ----
NEW = ["sfa_session_group_coverage_config", "sfa_session_group_coverage", "sfa_session_group_coverage_bytes"]


def test_the_library_exports_the_three_functions():
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    for sym in NEW:
        assert sym in _lib.SYMBOLS and getattr(L, sym) is not None, sym
        assert f" {sym}(" in header, sym
    assert "sfa_group_cover_t" in header and S.GROUP_COVER_DTYPE.itemsize == 32


def test_group_coverage_bytes_is_host_arithmetic():
    rng = np.random.default_rng(5)
    lens = [31, 33, 70]
    fw = [rng.normal(size=n).astype(np.float32) for n in lens]
    dna = S.RefModel(["a", "b", "c"], [n + 5 for n in lens], lens, [0, 7, 100], fw, [x.copy() for x in fw])
    rna = S.RefModel(["a", "b", "c"], [n + 5 for n in lens], lens, [0, 7, 100], fw, None)
    words = lambda cols: (cols + 3) // 4 + 1  # 8-byte words of four labels, and the one behind the row
    assert S.session_group_coverage_bytes(dna, 7, 0) == 4 * (sum(lens) + 3) + 8 * words(2 * sum(lens)) + 36 * 8
    assert S.session_group_coverage_bytes(rna, 1023, S.RNA | S.INV) == 4 * (sum(lens) + 3) + 8 * words(sum(lens)) + 36 * 1024
    assert S.session_group_coverage_bytes(dna, 0, 0) == 0 and S.session_group_coverage_bytes(dna, 1024, 0) == 0
