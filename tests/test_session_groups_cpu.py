"""The host rules of a session's target groups without a GPU: the stand-alone program tests/c/group_rules.cpp, built from
sigfish_amd/csrc/group_rules.hpp alone with -Wall -Werror and once more under ASan + UBSan (its selftest checks the label table
against a loop over place_col of row_rules.hpp, every refusal, the key order, heads and the decision table); the numpy restatement
the GPU test relies on (tests/group_oracle.py) against the header's labels and decisions; the decision through the library's
sfa_group_decide; the BED reader with names; the tag formatter of both languages on hand-written records; the refusals of
--by-name without --targets, which come before any file or device is opened."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime
from tests import group_oracle as G
from tests.realtime_util import BIN, write_model
from tests.util import GOLD, ROOT

INF = float("inf")


def _build(tmp, source, name, sanitize):
    exe = str(tmp / (name + ("_san" if sanitize else "")))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", source)]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


def _programs(tmp, source, name):
    """[plain build, sanitizer build or None]"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe, build = _build(tmp, source, name, False)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    san, build = _build(tmp, source, name, True)
    if build.returncode != 0 and any(m in build.stderr for m in (b"libasan", b"libubsan", b"-lasan", b"-lubsan", b"unrecognized command-line option", b"unsupported option")):
        san = None
    else:
        assert build.returncode == 0, build.stderr.decode()[-2000:]
    return [exe, san]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return _programs(tmp_path_factory.mktemp("group_rules"), "group_rules.cpp", "group_rules")


@pytest.fixture(scope="module")
def tag_programs(tmp_path_factory):
    return _programs(tmp_path_factory.mktemp("group_tags"), "group_tags.cpp", "group_tags")


def _ask(programs, text):
    """every request goes through all builds, and their answers must be the same lines"""
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


def test_selftest_plain_and_under_sanitizers(programs):
    line = _ask(programs, "selftest\n")[-1].split()
    assert line[:2] == ["selftest", "ok"] and int(line[2]) > 1500


# ---- the numpy restatement of the labels against the header's ----
LENS = [1, 31, 32, 33, 64, 65, 300]
OFFS = [0, 7, 0, 100, 3, 0, 1000]
LISTS = {
    "empty": ([], 3),
    "whole contigs": ([(r, OFFS[r], OFFS[r] + LENS[r] + 1, 6 - r) for r in range(7)], 7),
    "overlaps of two and three": ([(6, 1010, 1100, 2), (6, 1030, 1080, 1), (6, 1050, 1060, 0), (6, 1055, 1200, 3), (4, 3, 40, 1), (4, 20, 68, 0)], 4),
    "touching, unsorted, an empty group": ([(6, 1200, 1260, 5), (6, 1010, 1040, 0), (6, 1040, 1064, 1), (6, 1064, 1065, 0), (3, 105, 120, 3), (0, 0, 2, 1022)], 1023),
    "below the offset": ([(3, 0, 100, 0), (6, 5, 1000, 1)], 2),
    "every column its own": ([(5, c, c + 1, 64 - c) for c in range(65)], 65),
}


def _labels_text(strands, t, n_groups):
    return f"labels {strands} {len(LENS)} " + " ".join(f"{n} {o}" for n, o in zip(LENS, OFFS)) + f" {n_groups} {len(t)} " + " ".join(" ".join(str(x) for x in k) for k in t) + "\n"


@pytest.mark.parametrize("strands", [1, 2], ids=["rna_one_strand", "dna_two_strands"])
@pytest.mark.parametrize("name", list(LISTS))
def test_python_labels_equal_the_headers(programs, name, strands):
    t, n_groups = LISTS[name]
    tag, in_group, *labels = _ask(programs, _labels_text(strands, t, n_groups))[0].split()
    want = G.labels_of(t, n_groups, LENS, OFFS, strands)
    assert tag == "labels" and [int(x) for x in labels] == [int(x) for x in want] and int(in_group) == int((want != n_groups).sum())
    if name in ("empty", "below the offset"):
        assert int(in_group) == 0
    if name == "whole contigs":
        assert int(in_group) == len(want)
    if name == "overlaps of two and three" and strands == 1:  # the lowest id wins: contig 6 begins at column 226 of the row
        at = sum(LENS[:6])
        assert [int(want[at + c]) for c in (9, 10, 29, 30, 49, 50, 59, 60, 79, 80, 99, 100, 199, 200)] == [4, 2, 2, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 4]


REFUSALS = [((-1, 0, 1, 0), 2, "contig"), ((7, 0, 1, 0), 2, "contig"), ((2, -1, 4, 0), 2, "negative"), ((2, 4, 4, 0), 2, "empty"), ((2, 0, 34, 0), 2, "beyond"),
            ((2, 0, 4, 2), 2, "group"), ((2, 0, 4, -1), 2, "group"), ((2, 0, 4, 0), 0, "n_groups"), ((2, 0, 4, 0), 1024, "n_groups")]


@pytest.mark.parametrize("target,n_groups,word", REFUSALS)
def test_refusals(programs, target, n_groups, word):
    line = _ask(programs, _labels_text(2, [(6, 1000, 1001, 0), target], n_groups))[0]
    assert line.startswith("refused ") and word in line and ("target 1:" in line or word == "n_groups")


# ---- the decision: the header's function (the program), the library's export and the oracle give the same answers ----
#        best second best_score second_score n valid min margin want
TABLE = [(3, 1, 10.0, 60.0, 100, 1, 100, 0.5, 3),      # margin exactly met, n at min_events
         (3, 1, 10.0, 59.5, 100, 1, 100, 0.5, None),   # margin just missed
         (3, 1, 10.0, 60.0, 99, 1, 100, 0.5, None),    # n_events < min_events
         (7, -1, 10.0, INF, 100, 1, 100, 1e30, 7),     # an empty runner-up counts as +inf
         (7, -1, 10.0, 3.0, 100, 1, 100, 0.5, 7),      # ... whatever its score field holds
         (2, 5, 10.0, INF, 100, 1, 100, 1e30, 2),      # a runner-up whose every column costs +inf
         (2, 5, INF, INF, 100, 1, 100, 0.0, None),
         (-1, -1, INF, INF, 100, 1, 100, 0.0, None),
         (3, 1, 10.0, 60.0, 100, 0, 100, 0.5, None),   # valid = 0
         (3, 1, 10.0, 60.0, 100, 1, 100, -1.0, None),  # a negative margin
         (3, 1, 10.0, 60.0, 100, 1, 100, INF, None),   # a margin that is not finite
         (1023, 0, 10.0, 10.0, 100, 1, 100, 0.0, 1023)]


def test_decision_table(programs):
    text = "".join("decide " + " ".join(str(x) for x in row[:8]) + "\n" for row in TABLE)
    for row, line in zip(TABLE, _ask(programs, text)):
        best, second, bs, ss, n, valid, min_events, margin, want = row
        assert line == f"decide {-1 if want is None else want}", row
        rec = np.zeros(1, S.GROUP_HEAD_DTYPE)
        rec[0] = (best, second, bs, ss, n, valid)
        assert S.group_decide(rec, min_events, margin) == want, row
        assert G.decide(rec[0], min_events, margin) == want, row
    with pytest.raises(S.SfaError, match="one head"):
        S.group_decide(np.zeros(2, S.GROUP_HEAD_DTYPE), 1, 0.1)


def test_oracle_entries_and_head():
    """the oracle on a hand-written row: ties go to the lowest column, entries without columns are never named"""
    row = np.array([5, 2, 9, 2, 7, np.inf, np.inf, 1], np.float32)
    label = np.array([0, 0, 1, 1, 4, 2, 2, 4])
    entries, head = G.entries_of_row(row, label, 4, [8], [10], 1)
    assert [e[4] for e in entries] == [1, 3, 5, -1, 7] and [float(e[0]) for e in entries] == [2, 2, INF, INF, 1]
    assert entries[2][1:4] == (0, 15, ord("+")) and entries[3][:4] == (np.float32(np.inf), -1, -1, 0)
    assert (head["best"], head["second"], float(head["best_score"]), float(head["second_score"])) == (4, 0, 1.0, 2.0)
    _, head = G.entries_of_row(row[:4], np.array([1, 1, 0, 0]), 2, [4], [0], 1)
    assert (head["best"], head["second"]) == (1, 0) and head["best_score"] == head["second_score"] == 2  # equal scores: the lower column first
    _, head = G.entries_of_row(row[:4], np.array([3, 3, 3, 3]), 3, [4], [0], 1)
    assert (head["best"], head["second"]) == (3, -1) and np.isinf(head["second_score"])


# ---- the BED reader with names ----
def test_read_target_groups(tmp_path):
    names = ["chrA", "chrB", "chrC"]
    bed = tmp_path / "t.bed"
    bed.write_text("# a comment\ntrack name=x\nbrowser position chrA:1-2\n\nchrB\t5\t40\tamp 2\t0\t+\nchrA 0 7 amp1\nchrB\t50\t60\tamp 2\nchrC\t1\t2\tamp0\n")
    got, groups = S.read_target_groups(str(bed), names)
    assert got.dtype == S.GROUP_TARGET_DTYPE and [tuple(int(v) for v in x) for x in got] == [(1, 5, 40, 0), (0, 0, 7, 1), (1, 50, 60, 0), (2, 1, 2, 2)]
    assert groups == ["amp 2", "amp1", "amp0"]  # numbered by first appearance
    for text, word in (("chrZ\t1\t2\tn\n", "not in the reference"), ("chrA\t1\n", "three columns"), ("chrA\tx\t2\tn\n", "integers"), ("chrA\t1\t2\tn\nchrA\t1\t2\n", r"t\.bed:2: .*fourth column"),
                       ("chrA 1 2\n", r"t\.bed:1: .*fourth column")):
        bed.write_text(text)
        with pytest.raises(S.SfaError, match=word):
            S.read_target_groups(str(bed), names)
    bed.write_text("".join(f"chrA\t{k}\t{k + 1}\tg{k}\n" for k in range(1023)))
    got, groups = S.read_target_groups(str(bed), names)
    assert len(groups) == 1023 == S.GROUP_MAX and int(got["group"][-1]) == 1022
    bed.write_text("".join(f"chrA\t{k}\t{k + 1}\tg{k}\n" for k in range(1024)))
    with pytest.raises(S.SfaError, match=r"t\.bed:1024: more than 1023 group names"):
        S.read_target_groups(str(bed), names)
    bed.write_text("")
    got, groups = S.read_target_groups(str(bed), names)
    assert len(got) == 0 and groups == []
    # read_targets reads the same file as before
    bed.write_text("chrB\t5\t40\tname\nchrA 0 7\n")
    assert [tuple(int(v) for v in x) for x in S.read_targets(str(bed), names)] == [(1, 5, 40), (0, 0, 7)]


# ---- the two tags, hand-written records, both languages ----
NAMES = ["amp1", "orf1ab", "N"]
#         best second best_score second_score n_events   the tags
RECORDS = [(1, 0, 10.0, 60.0, 100, "\\ttg:Z:orf1ab\\tgm:f:0.5000"),
           (3, 2, 12.5, 13.0, 40, "\\ttg:Z:*\\tgm:f:0.0125"),      # the background is best
           (0, -1, 12.5, INF, 40, "\\ttg:Z:amp1\\tgm:f:inf"),       # no runner-up
           (0, -1, 12.5, 1.0, 40, "\\ttg:Z:amp1\\tgm:f:inf"),       # ... whatever its score field holds
           (2, 0, 7.0, INF, 10, "\\ttg:Z:N\\tgm:f:inf"),           # a runner-up at +inf
           (2, 0, INF, INF, 10, "\\ttg:Z:N\\tgm:f:nan"),           # +inf against +inf
           (2, 0, 7.0, 7.0, 0, "\\ttg:Z:N\\tgm:f:nan"),            # no events
           (-1, -1, INF, INF, 10, "\\ttg:Z:*\\tgm:f:nan"),         # no entry
           (1, 2, 1.0, 1.00004, 1, "\\ttg:Z:orf1ab\\tgm:f:0.0000"),
           (1, 2, 100.25, 100.75, 3, "\\ttg:Z:orf1ab\\tgm:f:0.1667")]


def test_group_tags_in_both_languages(tag_programs):
    text = f"{len(NAMES)} " + " ".join(NAMES) + "\n" + "".join(" ".join(str(x) for x in r[:5]) + "\n" for r in RECORDS)
    lines = _ask(tag_programs, text)
    assert len(lines) == len(RECORDS)
    for rec, line in zip(RECORDS, lines):
        head = np.zeros(1, S.GROUP_HEAD_DTYPE)
        head[0] = (*rec[:5], 1)
        assert line == rec[5] == realtime.group_tags(head[0], NAMES).replace("\t", "\\t"), rec
    assert realtime.format_group_summary({("group", 1): 4, ("group", 3): 2, "A": [6, 100]}, NAMES) == \
        "[realtime] group amp1: accepted 0 reads\n[realtime] group orf1ab: accepted 4 reads\n[realtime] group N: accepted 0 reads\n[realtime] group *: accepted 2 reads\n"


# ---- --by-name belongs to --targets ----
def test_replay_refuses_by_name_without_targets_before_any_session():
    class NoAligner:
        def session(self, *a, **kw):
            raise AssertionError("a session was opened")

    with pytest.raises(S.SfaError, match="by_name belongs to targets"):
        list(realtime.replay(NoAligner(), [], 2, 100, 3, 25, 70, 30, 5, by_name=True))
    gt = (np.zeros(1, S.GROUP_TARGET_DTYPE), ["a"])
    for kw, word in ((dict(targets=gt, by_name=True, margin=0.1), "ENRICH"), (dict(targets=gt, by_name=True, mode=S.ENRICH), "margin")):
        with pytest.raises(S.SfaError, match=word):
            list(realtime.replay(NoAligner(), [], 2, 100, 3, 25, 70, 30, 5, **kw))


def test_binary_refuses_by_name_without_targets_before_any_file_or_device(tmp_path):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    model = write_model(tmp_path / "syn.model", 6)
    r = subprocess.run([BIN, "realtime", "--kmer-model", model, "--by-name", os.path.join(GOLD, "data", "nCoV-2019.reference.fasta"), str(tmp_path / "no_such.blow5")],
                       capture_output=True, timeout=60)
    err = r.stderr.decode()
    assert r.returncode > 0 and r.stdout == b"", (r.returncode, err)
    assert err.count("[sigfish-amd] ERROR:") == 1 and "--by-name belongs to --targets" in err, err
    assert "no_such" not in err and "accelerator" not in err, err


def test_symbols_are_bound():
    L = S._lib.load() if hasattr(S, "_lib") else None
    from sigfish_amd import _lib
    L = _lib.load()
    for name in ("sfa_session_target_groups", "sfa_session_group_count", "sfa_session_group_bests", "sfa_group_decide"):
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    assert S.GROUP_BEST_DTYPE.itemsize == 16 and S.GROUP_HEAD_DTYPE.itemsize == 24 and S.GROUP_TARGET_DTYPE.itemsize == 16
