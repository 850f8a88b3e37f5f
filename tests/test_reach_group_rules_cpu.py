"""The host rules of a session's reach groups without a GPU: the stand-alone program tests/c/reach_group_rules.cpp, built from
sigfish_amd/csrc/reach_group_rules.hpp alone with -Wall -Werror and once more under ASan + UBSan -- the model against a brute-force
statement, the prepared runs against the model, the consequences of the rule (group_labels at lead 0, reach_tables' anchors, label
and mask bit), the live rule, the records' body columns, the named cases, 3000 random lists.  The numpy model the GPU tests carry
(tests/reach_group_model.py) on crafted columns; the three new symbols of the C ABI; the host arithmetic of
session_group_reach_bytes; the BED reader."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib
from tests import reach_group_model as M
from tests.util import ROOT


def _build(tmp, sanitize):
    exe = str(tmp / ("reach_group_rules_san" if sanitize else "reach_group_rules"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "reach_group_rules.cpp")]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("reach_group_rules")
    exe, build = _build(tmp, False)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    san, build = _build(tmp, True)
    if build.returncode != 0 and any(m in build.stderr for m in (b"libasan", b"libubsan", b"-lasan", b"-lubsan", b"unrecognized command-line option", b"unsupported option")):
        san = None
    else:
        assert build.returncode == 0, build.stderr.decode()[-2000:]
    return [exe, san]


def test_selftest_plain_and_under_sanitizers(programs):
    outs = []
    for exe in programs:
        if exe is None:
            continue
        run = subprocess.run([exe], input=b"selftest\n", capture_output=True, timeout=600)
        assert run.returncode == 0, (run.returncode, (run.stdout + run.stderr).decode()[-3000:])
        assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]
        outs.append(run.stdout.decode().splitlines())
    assert all(o == outs[0] for o in outs)
    line = outs[0][-1].split()
    assert line[:2] == ["selftest", "ok"] and int(line[2]) > 20000


def test_numpy_model_on_crafted_columns():
    """the model the GPU tests compare the device with, against hand-made answers"""
    lens, offs = [70], [3]
    t = [(0, 40, 50, 10, 5, "+"), (0, 40, 45, 10, 2, "+"), (0, 20, 25, 4, 1, "-")]
    label, anchor = M.tables(t, 8, lens, offs, strands=2)
    as_records = S.api._reach_group_targets(t)  # the same list as REACH_GROUP_TARGET_DTYPE records: the model reads either form
    assert as_records.dtype == S.REACH_GROUP_TARGET_DTYPE and all(np.array_equal(a, b) for a, b in zip(M.tables(as_records, 8, lens, offs, strands=2), (label, anchor)))
    x = lambda c: c - 3  # the '+' column of coordinate c
    assert label[x(29)] == 8 and list(label[x(30):x(45)]) == [2] * 15 and list(label[x(45):x(50)]) == [5] * 5 and label[x(50)] == 8
    assert list(anchor[x(30):x(41)]) == [37] * 11 and anchor[x(44)] == 41 and anchor[x(29)] == -1
    m = lambda c: 70 + (70 - (c - 3))  # the '-' column of coordinate c
    assert label[m(28)] == 1 and label[m(29)] == 8 and label[m(24)] == 1 and label[m(19)] == 8 and label[m(45)] == 8  # ('+' targets admit nothing on '-')
    assert anchor[m(28)] == 24 - 3 and anchor[m(22)] == 22 - 3
    # lead 0, strand 0: the plain group labels (lowest id covers)
    label, anchor = M.tables([(0, 10, 20, 0, 3, None), (0, 15, 30, 0, 1, None)], 4, lens, offs, strands=1)
    assert list(label[x(10):x(15)]) == [3] * 5 and list(label[x(15):x(30)]) == [1] * 15 and list(anchor[x(10):x(30)]) == list(range(7, 27))
    # a '-' target at or below the offset
    label, anchor = M.tables([(0, 0, 3, 9, 0, "-")], 1, lens, offs, strands=2)
    assert list(anchor[m(11):m(3)]) == [S.REACH_BELOW_TRACK] * 8 and list(label[m(11):m(3)]) == [0] * 8 and label[m(12)] == 1  # (coordinates 4 .. 11 lead to 2, below the offset 3)
    # the live rule reads the anchor's depth
    label, anchor = M.tables(t, 8, lens, offs, strands=2)
    depth = np.zeros(71, np.uint32)
    depth[37] = 2
    live = M.live_labels(label, anchor, [depth], 2, 8, lens, strands=2)
    assert list(live[x(30):x(41)]) == [8] * 11 and list(live[x(41):x(45)]) == [2] * 4
    rec = M.records(label, anchor, [depth], 2, 8, lens, offs, strands=2)
    assert rec[2] == (5, 1, 2, 0, 2) and rec[5] == (5, 0, 0, 0, 0) and rec[1] == (0, 0, 0, 0xffffffff, 0) and rec[8][0] == 0


def test_capi_symbols_and_bytes():
    L = _lib.load()
    for name in ("sfa_session_target_groups_reach", "sfa_session_group_reach_tables", "sfa_session_group_reach_bytes"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    assert S.REACH_GROUP_TARGET_DTYPE.itemsize == C.sizeof(_lib.SfaReachGroupTarget) == 24
    assert [S.REACH_GROUP_TARGET_DTYPE.fields[f][1] for f in ("contig", "begin", "end", "lead", "group", "strand", "pad")] == [0, 4, 8, 12, 16, 20, 21]
    lens = np.array([31, 1000, 7], np.int32)
    cref = _lib.SfaRef()
    arr = (C.c_int32 * 3)(*lens)
    cref.num_ref = 3
    cref.ref_lengths = C.cast(arr, C.POINTER(C.c_int32))
    assert L.sfa_session_group_reach_bytes(C.byref(cref), 0) == 6 * 2 * int(lens.sum())
    assert L.sfa_session_group_reach_bytes(C.byref(cref), S.RNA) == 6 * int(lens.sum())
    assert L.sfa_session_group_reach_bytes(None, 0) == 0
    arr_f = lambda n: np.zeros(n, np.float32)
    ref = S.RefModel(["a", "b"], [36, 12], [31, 7], [0, 3], [arr_f(31), arr_f(7)], [arr_f(31), arr_f(7)])
    assert S.session_group_reach_bytes(ref) == 6 * 2 * 38 and S.session_group_reach_bytes(ref, S.RNA) == 6 * 38
    assert S.session_group_reach_bytes(ref) == S.session_reach_bytes(ref) + 2 * 2 * 38
    # null session: refused without a device
    assert L.sfa_session_target_groups_reach(None, None, 0, 1) != 0
    assert L.sfa_session_group_reach_tables(None, None, None, 0) != 0


def test_read_reach_target_groups(tmp_path):
    bed = tmp_path / "t.bed"
    bed.write_text("# c\ntrack x\nchr2\t5\t9\tgeneB\t0\t-\nchr1 1 4 geneA 0 +\nchr2\t20\t30\tgeneB\t0\t.\n")
    t, names = S.read_reach_target_groups(str(bed), ["chr1", "chr2"], 25, stranded=True)
    assert names == ["geneB", "geneA"] and t.dtype == S.REACH_GROUP_TARGET_DTYPE
    assert [tuple(int(v) for v in (r["contig"], r["begin"], r["end"], r["lead"], r["group"], r["strand"])) for r in t] == [
        (1, 5, 9, 25, 0, ord("-")), (0, 1, 4, 25, 1, ord("+")), (1, 20, 30, 25, 0, 0)]
    assert not t["pad"].any()
    t2, names2 = S.read_reach_target_groups(str(bed), ["chr1", "chr2"], 0)
    plain, names3 = S.read_target_groups(str(bed), ["chr1", "chr2"])
    assert names2 == names3 and not t2["strand"].any() and not t2["lead"].any()
    assert all((t2[f] == plain[f]).all() for f in ("contig", "begin", "end", "group"))
    for lead in (-1, (1 << 30) + 1, True, 2.5):
        with pytest.raises(S.SfaError, match="read_reach_target_groups: lead"):
            S.read_reach_target_groups(str(bed), ["chr1", "chr2"], lead)
    short = tmp_path / "s.bed"
    short.write_text("chr1\t1\t4\tgeneA\n")
    with pytest.raises(S.SfaError, match="read_reach_target_groups: .*sixth column"):
        S.read_reach_target_groups(str(short), ["chr1"], 3, stranded=True)
    none = tmp_path / "n.bed"
    none.write_text("chr1\t1\t4\n")
    with pytest.raises(S.SfaError, match="read_reach_target_groups: .*fourth column"):
        S.read_reach_target_groups(str(none), ["chr1"], 3)
    # the tuple form of the setter's list
    arr = S.api._reach_group_targets([(0, 1, 4, 7, 2, "+"), (1, 2, 3, 0, 0, None)])
    assert arr["strand"].tolist() == [ord("+"), 0] and arr["group"].tolist() == [2, 0] and arr["lead"].tolist() == [7, 0]
