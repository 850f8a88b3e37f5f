"""`realtime --group-cap` and replay(group_cap=) without a GPU: every refusal comes before any file, session or device is opened
(the files named do not exist; a refusal that came later would name them), and the formatters of the two languages agree: the
stand-alone program tests/c/group_cover_tags.cpp prints replay::group_is_full and replay::group_cover_line for hand-written
records -- a group without columns among them, whose mean is `-`: the quotient is never formed -- plain and under ASan + UBSan,
and its lines are realtime.group_is_full's and realtime.group_cover_line's."""
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime
from tests.realtime_util import BIN, write_model
from tests.test_session_groups_cpu import _ask, _programs
from tests.util import GOLD

BED = "nCoV.bed"
G_OK = ["--targets", BED, "--by-name", "--enrich", "--margin", "0.1"]
REFUSED = [(G_OK + ["--group-cap", "0"], "--group-cap should be an integer 1.."), (G_OK + ["--group-cap", "-2"], "--group-cap should be an integer 1.."),
           (G_OK + ["--group-cap", "x"], "--group-cap should be an integer 1.."), (G_OK + ["--group-cap", "1073741825"], "--group-cap should be an integer 1.."),
           (["--group-cap", "3"], "pass --targets FILE.bed --by-name --enrich"), (["--targets", BED, "--enrich", "--margin", "0.1", "--group-cap", "3"], "pass --targets FILE.bed --by-name --enrich"),
           (["--targets", BED, "--by-name", "--deplete", "--margin", "0.1", "--group-cap", "3"], "--group-cap with --deplete is not built"),
           (G_OK + ["--group-cap", "3", "--depth-cap", "3"], "--group-cap and --depth-cap are two caps"),
           (G_OK + ["--quota", "2", "--group-cap", "3", "--depth-cap", "3"], "--group-cap and --depth-cap are two caps"),
           (G_OK + ["--group-cap", "3", "--resweep"], "--group-cap is not available with --resweep")]


@pytest.mark.parametrize("extra,msg", REFUSED, ids=["_".join(e).replace("--", "") for e, _ in REFUSED])
def test_binary_refuses_group_cap_options_before_any_file_or_device(extra, msg, tmp_path):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    model = write_model(tmp_path / "syn.model", 6)
    r = subprocess.run([BIN, "realtime", "--kmer-model", model, *extra, os.path.join(GOLD, "data", "nCoV-2019.reference.fasta"), str(tmp_path / "no_such.blow5")],
                       capture_output=True, timeout=60)
    err = r.stderr.decode()
    assert r.returncode > 0 and r.stdout == b"", (r.returncode, err)
    assert err.count("[sigfish-amd] ERROR:") == 1 and msg in err, err
    assert "no_such" not in err and BED not in err.split("ERROR:")[1].replace("FILE.bed", "") and "accelerator" not in err, err


def test_help_names_the_option():
    r = subprocess.run([BIN, "realtime", "--help"], capture_output=True, timeout=60)
    assert "--group-cap INT" in (r.stdout + r.stderr).decode()


def test_replay_refuses_bad_group_caps_before_any_session():
    class NoAligner:
        def session(self, *a, **kw):
            raise AssertionError("a session was opened")

    class NoStarts:
        starts = False

        def __getattr__(self, name):
            raise AssertionError("the session was used")

    groups = (np.zeros(1, S.GROUP_TARGET_DTYPE), ["g"])
    ok = dict(targets=groups, by_name=True, mode=S.ENRICH, margin=0.1)
    for kw, word in ((dict(ok, group_cap=0), "integer 1"), (dict(ok, group_cap=-3), "integer 1"), (dict(ok, group_cap=1.5), "integer 1"), (dict(ok, group_cap=True), "integer 1"),
                     (dict(ok, group_cap=(1 << 30) + 1), "integer 1"), (dict(group_cap=2), "by_name=True"), (dict(targets=[(0, 0, 10)], mode=S.ENRICH, margin=0.1, group_cap=2), "by_name=True"),
                     (dict(ok, mode=S.DEPLETE, group_cap=2), "not built"), (dict(ok, group_cap=2, depth_cap=2), "two caps"), (dict(ok, quota=3, group_cap=2, depth_cap=2), "two caps"),
                     (dict(ok, group_cap=2, resweep=True), "resweep"), (dict(ok, group_cap=2, session=NoStarts()), "start columns")):
        with pytest.raises(S.SfaError, match=word):
            list(realtime.replay(NoAligner(), [], 2, 100, 3, 25, 70, 30, 5, **kw))


@pytest.fixture(scope="module")
def tag_programs(tmp_path_factory):
    return _programs(tmp_path_factory.mktemp("group_cover_tags"), "group_cover_tags.cpp", "group_cover_tags")


def test_group_cover_formatters_in_both_languages(tag_programs):
    # (name, columns, capped, depth_sum), the line both languages must print, full
    records = [("amp17", 8, 3, 20, "[realtime] group depth amp17\\tcolumns=8 capped=3 mean_depth=2.500", 0),
               ("none", 0, 0, 0, "[realtime] group depth none\\tcolumns=0 capped=0 mean_depth=-", 0),  # no columns: no quotient, never full
               ("full", 5, 5, 5, "[realtime] group depth full\\tcolumns=5 capped=5 mean_depth=1.000", 1),
               ("one", 1, 1, 4000000000, "[realtime] group depth one\\tcolumns=1 capped=1 mean_depth=4000000000.000", 1),
               ("third", 3, 2, 1, "[realtime] group depth third\\tcolumns=3 capped=2 mean_depth=0.333", 0),
               ("half", 16, 0, 40, "[realtime] group depth half\\tcolumns=16 capped=0 mean_depth=2.500", 0),
               ("deep", 29903, 29903, 3 * 29903 + 1, "[realtime] group depth deep\\tcolumns=29903 capped=29903 mean_depth=3.000", 1)]
    lines = _ask(tag_programs, "".join(f"{n} {c} {k} {s}\n" for n, c, k, s, _, _ in records))
    assert len(lines) == len(records)
    for (n, c, k, s, want, full), line in zip(records, lines):
        py = realtime.group_cover_line(n, c, k, s)
        assert py.endswith("\n") and line == f"{full} {want}" == f"{int(realtime.group_is_full(c, k))} " + py[:-1].replace("\t", "\\t"), (n, line, py)


def test_formatters_have_the_documented_shape():
    assert realtime.group_is_full(3, 3) and not realtime.group_is_full(3, 2) and not realtime.group_is_full(0, 0)
    assert realtime.group_cover_line("amp17", 8, 3, 20) == "[realtime] group depth amp17\tcolumns=8 capped=3 mean_depth=2.500\n"
    assert realtime.group_cover_line("none", 0, 0, 0) == "[realtime] group depth none\tcolumns=0 capped=0 mean_depth=-\n"  # the quotient is never formed
    rec = np.zeros(3, S.GROUP_COVER_DTYPE)
    rec["columns"], rec["capped"], rec["depth_sum"] = [4, 0, 9], [1, 0, 0], [6, 0, 0]
    text = realtime.format_group_cover_summary({"group_cover": dict(cap=2, intervals=5, bases=77, records=rec)}, ["a", "b"])
    assert text == "[realtime] group cap 2\t5 intervals, 77 bases added\n[realtime] group depth a\tcolumns=4 capped=1 mean_depth=1.500\n[realtime] group depth b\tcolumns=0 capped=0 mean_depth=-\n"
