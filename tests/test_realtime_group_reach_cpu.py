"""The refusals of `sigfish-amd realtime --group-lead / --group-stranded` and replay(group_lead=, group_stranded=) that need no
device: every one comes before any file, session or device is opened -- without --by-name, with --lead, with --depth-cap, with
--deplete, a lead outside 0 .. 2^30, --group-stranded without --group-lead.  --by-name with --lead keeps its refusal
(tests/test_realtime_reach_cpu.py pins it)."""
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime
from tests.realtime_util import BIN, write_model
from tests.util import GOLD


def test_replay_refuses_bad_group_leads_before_any_session():
    class NoAligner:
        def session(self, *a, **kw):
            raise AssertionError("a session was opened")

    groups = (np.zeros(1, S.GROUP_TARGET_DTYPE), ["g"])
    plain = dict(targets=[(0, 0, 10)], mode=S.ENRICH, margin=0.1)
    named = dict(targets=groups, by_name=True, mode=S.ENRICH, margin=0.1)
    for kw, word in ((dict(group_lead=5), "by_name=True"), (dict(group_stranded=True), "by_name=True"), (dict(plain, group_lead=5), "by_name=True"),
                     (dict(named, group_lead=5, lead=5), "two leads"), (dict(named, group_lead=5, stranded=True), "two leads"),
                     (dict(named, group_lead=5, depth_cap=2), "depth_cap is not built"),
                     (dict(named, group_lead=5, mode=S.DEPLETE), "mode=DEPLETE is not built"),
                     (dict(named, group_stranded=True), "belongs to group_lead="),
                     (dict(named, group_lead=-1), "integer 0"), (dict(named, group_lead=(1 << 30) + 1), "integer 0"), (dict(named, group_lead=1.5), "integer 0"),
                     (dict(named, group_lead=True), "integer 0"),
                     (dict(named, group_lead=5, group_stranded=True), "read_reach_target_groups"),
                     (dict(named, group_lead=5, resweep=True), "resweep")):
        with pytest.raises(S.SfaError, match=word):
            list(realtime.replay(NoAligner(), [], 2, 100, 3, 25, 70, 30, 5, **kw))
    # the label path's own refusal stays what it was
    with pytest.raises(S.SfaError, match="not built"):
        list(realtime.replay(NoAligner(), [], 2, 100, 3, 25, 70, 30, 5, **dict(named, lead=5)))


def test_summary_line_is_the_binarys():
    assert realtime.format_reach_group_summary(dict(reach_groups=dict(lead=400, stranded=True, columns=1234))) == "[realtime] reach groups: lead 400, stranded\tlabelled columns: 1234\n"
    assert realtime.format_reach_group_summary(dict(reach_groups=dict(lead=0, stranded=False, columns=0))) == "[realtime] reach groups: lead 0\tlabelled columns: 0\n"


BED = "nCoV.bed"
T_OK = ["--targets", BED, "--enrich", "--margin", "0.1"]
NAMED = T_OK + ["--by-name"]
REFUSED = [(["--group-lead", "5"], "pass --targets FILE.bed --by-name"), (["--group-stranded"], "pass --targets FILE.bed --by-name"), (T_OK + ["--group-lead", "5"], "pass --targets FILE.bed --by-name"),
           (NAMED + ["--group-lead", "5", "--lead", "5"], "two leads"), (NAMED + ["--group-lead", "5", "--stranded"], "two leads"),
           (NAMED + ["--group-lead", "5", "--depth-cap", "2"], "--group-lead with --depth-cap is not built"),
           (["--targets", BED, "--deplete", "--margin", "0.1", "--by-name", "--group-lead", "5"], "--group-lead with --deplete is not built"),
           (NAMED + ["--group-stranded"], "--group-stranded belongs to --group-lead"),
           (NAMED + ["--group-lead", "-1"], "--group-lead should be an integer 0..1073741824"), (NAMED + ["--group-lead", "1073741825"], "--group-lead should be an integer 0..1073741824"),
           (NAMED + ["--group-lead", "x"], "--group-lead should be an integer 0..1073741824"), (NAMED + ["--group-lead", "5.5"], "--group-lead should be an integer 0..1073741824"),
           (NAMED + ["--lead", "5"], "they are not built")]


@pytest.mark.parametrize("extra,msg", REFUSED, ids=["_".join(e).replace("--", "") for e, _ in REFUSED])
def test_binary_refuses_group_lead_options_before_any_file_or_device(extra, msg, tmp_path):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    model = write_model(tmp_path / "syn.model", 6)
    # (the BED file and the reads do not exist: a refusal that came after opening either would name them)
    r = subprocess.run([BIN, "realtime", "--kmer-model", model, *extra, os.path.join(GOLD, "data", "nCoV-2019.reference.fasta"), str(tmp_path / "no_such.blow5")],
                       capture_output=True, timeout=60)
    err = r.stderr.decode()
    assert r.returncode > 0 and r.stdout == b"", (r.returncode, err)
    assert err.count("[sigfish-amd] ERROR:") == 1 and msg in err, err
    assert "no_such" not in err and BED not in err.split("ERROR:")[1].replace("FILE.bed", "") and "accelerator" not in err, err


def test_help_names_the_options():
    r = subprocess.run([BIN, "realtime", "-h"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"--group-lead INT" in r.stdout and b"--group-stranded" in r.stdout
