"""The host rules of a session's reach targets without a GPU: the stand-alone program tests/c/reach_rules.cpp, built from
sigfish_amd/csrc/reach_rules.hpp alone with -Wall -Werror and once more under ASan + UBSan, against the numpy model of
tests/reach_model.py on the case table of tests/reach_cases.py -- the mask, the anchor of every column, the entries the prepared
runs give when bisected, the live mask under a depth cap -- for DNA (two strands) and RNA (one).  What the case table reaches is
asserted here: the columns admitted through a lead-in alone (hand counts), each strand's share, the entries below the track.  The
list refusals; the three new symbols of the C ABI; the host arithmetic of session_reach_bytes; the BED reader."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib
from tests import reach_cases as RC
from tests import reach_model as M
from tests.util import ROOT


def _build(tmp, sanitize):
    exe = str(tmp / ("reach_rules_san" if sanitize else "reach_rules"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "reach_rules.cpp")]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """[plain build, sanitizer build or None]: every request goes through all of them, and their answers must be the same lines"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("reach_rules")
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


def _request(strands, cap, targets, intervals, lens=RC.LENS, offs=RC.OFFS):
    tl = f"{len(targets)} " + " ".join(f"{c} {b} {e} {lead} {s or '.'}" for c, b, e, lead, s in targets)
    il = f"{len(intervals)} " + " ".join(f"{c} {b} {e}" for c, b, e in intervals)
    return f"reach {strands} {len(lens)} " + " ".join(f"{n} {o}" for n, o in zip(lens, offs)) + f" {cap} {tl} {il}\n"


def test_selftest_plain_and_under_sanitizers(programs):
    line = _ask(programs, "selftest\n")[-1].split()
    assert line[:2] == ["selftest", "ok"] and int(line[2]) > 300


# what every case's depth is: intervals over a body's first bases, a whole body, a lead-in but not the body -- and a cap of 2, so
# that cap - 1 stays open
COVER = [(3, 50, 55), (3, 50, 55), (4, 1100, 1150), (4, 1100, 1150), (4, 1036, 1100), (4, 1036, 1100), (2, 120, 125), (2, 120, 125), (2, 100, 101), (1, 20, 21), (1, 20, 21),
         (3, 100, 101), (3, 100, 101), (4, 1130, 1131), (4, 1130, 1131), (4, 1300, 1301), (4, 1300, 1301)]


@pytest.mark.parametrize("strands", [1, 2], ids=["rna_one_strand", "dna_two_strands"])
@pytest.mark.parametrize("name", list(RC.CASES))
def test_header_equals_the_numpy_model(programs, name, strands):
    targets = RC.CASES[name]
    lines = _ask(programs, _request(strands, 2, targets, COVER))
    mask, anchor, lead_only, entry = RC.model_tables(name, strands)
    tag, on, *words = lines[0].split()
    assert tag == "mask" and int(on) == int(mask.sum())
    assert [int(w, 16) for w in words] == M.words_of(mask)
    assert [int(v) for v in lines[1].split()[1:]] == anchor.tolist()
    assert [int(v) for v in lines[2].split()[1:]] == entry.tolist()
    md = M.Reach(RC.LENS, RC.OFFS, strands)
    md.add(COVER)
    live = md.live_mask(targets, 2)
    tag, n_live, *words = lines[3].split()
    assert tag == "live" and int(n_live) == int(live.sum()) and [int(w, 16) for w in words] == M.words_of(live)
    assert not (live & ~mask).any()
    # ---- what the case reaches ----
    want = RC.LEAD_ONLY[name]
    if want is not None:
        assert int(lead_only.sum()) == want[2 - strands], (name, int(lead_only.sum()))  # (dna, rna)
    else:
        assert lead_only.any() and (mask & ~lead_only).any()
    per = {s: sum(int(mask[at:at + md.rl[c]].sum()) for c, st, at in md.jobs if st == s) for s in "+-"}
    wants_plus = any(t[4] in (None, "+") for t in targets)
    wants_minus = any(t[4] in (None, "-") for t in targets)
    if name == "bodies below the offset":  # (its bodies and '+' lead-ins lie below what a '+' row reports)
        wants_plus = False
    assert (per["+"] > 0) == wants_plus and (per["-"] > 0) == (wants_minus and strands == 2), (name, per)
    if name == "minus only" and strands == 1:  # the empty result: a '-' target without '-' jobs
        assert not mask.any() and (entry == M.NONE).all() and lines[0].split()[1] == "0"
    if name == "bodies below the offset" and strands == 2:
        assert int((entry == M.BELOW_TRACK).sum()) == 69 and live[entry == M.BELOW_TRACK].all()  # no depth is counted there: never closed
    if name == "overlapping lead-ins":  # '+' columns of 1040 .. 1099 lie in both lead-ins: the anchor is the nearer body's begin, 1100
        at = [a for c, s, a in md.jobs if c == 4 and s == "+"][0]
        assert set(anchor[at + 40:at + 100]) == {1100} and set(anchor[at + 110:at + 130]) == {1130}
        assert not live[at + 20:at + 140].any()  # 1100 .. 1149 were covered twice: both bodies and everything that leads to them are closed
    if name == "both strands":  # (4, 1100, 1150) was covered twice: the body and BOTH its lead-ins close; covering a lead-in alone closes only itself
        ap = [a for c, s, a in md.jobs if c == 4 and s == "+"][0]
        assert not live[ap + 36:ap + 150].any()
        if strands == 2:
            am = [a for c, s, a in md.jobs if c == 4 and s == "-"][0]
            assert not live[am + 300 - 213:am + 300 - 99].any()
        a3 = [a for c, s, a in md.jobs if c == 3 and s == "+"][0]
        assert not live[a3 + 13:a3 + 48].any() and live[a3 + 48:a3 + 73].all()  # '+' lead-in 20..49 and bases 50..54 closed, 55..79 open


def test_lead_0_strand_0_is_the_plain_mask(programs):
    plain = [(1, 12, 20), (1, 40, 46), (2, 0, 101), (3, 100, 150), (3, 140, 200), (4, 1300, 1301), (0, 5, 37)]
    lines = _ask(programs, _request(2, 1, [(c, b, e, 0, None) for c, b, e in plain], []))
    md = M.Reach(RC.LENS, RC.OFFS, 2)
    want = np.zeros(md.total, bool)
    xs = np.full(md.total, -1)
    for g, c, s, x in md.columns():
        want[g] = any(t[0] == c and t[1] <= x < t[2] for t in plain)
        xs[g] = x if want[g] else -1
    assert [int(w, 16) for w in lines[0].split()[2:]] == M.words_of(want)
    assert [int(v) for v in lines[1].split()[1:]] == xs.tolist()


REFUSALS = [((-1, 0, 1, 0, None), "contig -1 out of range"), ((5, 0, 1, 0, None), "contig 5 out of range"), ((2, -1, 4, 0, None), "is negative"), ((2, 4, 4, 0, None), "is empty"),
            ((2, 100, 197, 0, None), "lies beyond contig 2"), ((2, 100, 110, -1, None), "lead -1 outside"), ((2, 100, 110, (1 << 30) + 1, None), "outside 0 .. 1073741824"),
            ((2, 100, 110, 3, "x"), "strand 120"), ((2, 100, 110, 3, "*"), "strand 42")]


@pytest.mark.parametrize("target,word", REFUSALS)
def test_list_refusals(programs, target, word):
    line = _ask(programs, _request(2, 1, [(2, 100, 196, 1 << 30, "-"), target], []))[0]
    assert line.startswith("refused target 1:") and word in line, line


# ---- the C ABI ----
NEW = ["sfa_session_targets_reach", "sfa_session_reach_tables", "sfa_session_reach_bytes"]


def test_the_library_exports_the_three_functions():
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    for sym in NEW:
        assert sym in _lib.SYMBOLS and getattr(L, sym) is not None, sym
        assert f" {sym}(" in header, sym
    assert S.REACH_TARGET_DTYPE.itemsize == 20 and S.REACH_TARGET_DTYPE.names == ("contig", "begin", "end", "lead", "strand", "pad")


def test_reach_bytes_is_host_arithmetic():
    rng = np.random.default_rng(5)
    lens = [31, 33, 70]
    fw = [rng.normal(size=n).astype(np.float32) for n in lens]
    dna = S.RefModel(["a", "b", "c"], [n + 5 for n in lens], lens, [0, 7, 100], fw, [x.copy() for x in fw])
    rna = S.RefModel(["a", "b", "c"], [n + 5 for n in lens], lens, [0, 7, 100], fw, None)
    assert S.session_reach_bytes(dna, 0) == 4 * 2 * sum(lens)
    assert S.session_reach_bytes(rna, S.RNA | S.INV) == 4 * sum(lens)


def test_bed_reader(tmp_path):
    bed = tmp_path / "t.bed"
    bed.write_text("# comment\ntrack name=x\nb\t10\t20\tn1\t0\t+\na 1 5 n2 0 -\n\nb\t30\t40\tn3\t0\t.\n")
    t = S.read_reach_targets(str(bed), ["a", "b"], 7, stranded=True)
    assert t.dtype == S.REACH_TARGET_DTYPE and t["contig"].tolist() == [1, 0, 1] and t["begin"].tolist() == [10, 1, 30] and t["end"].tolist() == [20, 5, 40]
    assert t["lead"].tolist() == [7, 7, 7] and t["strand"].tolist() == [ord("+"), ord("-"), 0] and not t["pad"].any()
    u = S.read_reach_targets(str(bed), ["a", "b"], 0)
    assert u["strand"].tolist() == [0, 0, 0] and u["lead"].tolist() == [0, 0, 0]
    assert S.read_targets(str(bed), ["a", "b"]).tolist() == [(1, 10, 20), (0, 1, 5), (1, 30, 40)]  # (read_targets reads the same file as before)
    for lead in (-1, (1 << 30) + 1, 1.5, True):
        with pytest.raises(S.SfaError, match="lead should be an integer"):
            S.read_reach_targets(str(bed), ["a", "b"], lead)
    (tmp_path / "short.bed").write_text("a\t1\t5\n")
    with pytest.raises(S.SfaError, match="no sixth column"):
        S.read_reach_targets(str(tmp_path / "short.bed"), ["a"], 3, stranded=True)
    assert len(S.read_reach_targets(str(tmp_path / "short.bed"), ["a"], 3)) == 1
    (tmp_path / "bad.bed").write_text("a\t1\t5\tn\t0\tx\n")
    with pytest.raises(S.SfaError, match="none of"):
        S.read_reach_targets(str(tmp_path / "bad.bed"), ["a"], 3, stranded=True)
    with pytest.raises(S.SfaError, match="not in the reference"):
        S.read_reach_targets(str(bed), ["a"], 3)
