"""The refusals of `sigfish-amd realtime --lead / --stranded` and replay(lead=, stranded=) that need no device: every one comes
before any file, session or device is opened -- without targets, with labels (--by-name / --quota / --group-cap: not built), a
lead outside 0 .. 2^30, --stranded without --lead."""
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime
from tests.realtime_util import BIN, write_model
from tests.util import GOLD


def test_replay_refuses_bad_leads_before_any_session():
    class NoAligner:
        def session(self, *a, **kw):
            raise AssertionError("a session was opened")

    t = [(0, 0, 10)]
    groups = (np.zeros(1, S.GROUP_TARGET_DTYPE), ["g"])
    ok = dict(targets=t, mode=S.ENRICH, margin=0.1)
    named = dict(targets=groups, by_name=True, mode=S.ENRICH, margin=0.1)
    for kw, word in ((dict(lead=5), "pass targets="), (dict(stranded=True), "pass targets="), (dict(lead=5, stranded=True), "pass targets="),
                     (dict(named, lead=5), "not built"), (dict(named, quota=2, lead=5), "not built"), (dict(named, group_cap=2, lead=5), "not built"),
                     (dict(named, stranded=True), "not built"),
                     (dict(ok, stranded=True), "belongs to lead="),
                     (dict(ok, lead=-1), "integer 0"), (dict(ok, lead=(1 << 30) + 1), "integer 0"), (dict(ok, lead=1.5), "integer 0"), (dict(ok, lead=True), "integer 0"),
                     (dict(ok, lead=5, stranded=True), "REACH_TARGET_DTYPE"),
                     (dict(targets=np.zeros(1, S.REACH_TARGET_DTYPE), mode=S.ENRICH, margin=0.1, lead=5, stranded=True, resweep=True), "resweep")):
        with pytest.raises(S.SfaError, match=word):
            list(realtime.replay(NoAligner(), [], 2, 100, 3, 25, 70, 30, 5, **kw))


BED = "nCoV.bed"
T_OK = ["--targets", BED, "--enrich", "--margin", "0.1"]
REFUSED = [(["--lead", "5"], "pass --targets FILE.bed"), (["--stranded"], "pass --targets FILE.bed"), (["--lead", "5", "--stranded"], "pass --targets FILE.bed"),
           (T_OK + ["--by-name", "--lead", "5"], "they are not built"), (T_OK + ["--by-name", "--quota", "2", "--lead", "5"], "they are not built"),
           (T_OK + ["--by-name", "--group-cap", "2", "--lead", "5", "--stranded"], "they are not built"), (T_OK + ["--by-name", "--stranded"], "they are not built"),
           (T_OK + ["--stranded"], "--stranded belongs to --lead"),
           (T_OK + ["--lead", "-1"], "--lead should be an integer 0..1073741824"), (T_OK + ["--lead", "1073741825"], "--lead should be an integer 0..1073741824"),
           (T_OK + ["--lead", "x"], "--lead should be an integer 0..1073741824"), (T_OK + ["--lead", "5.5"], "--lead should be an integer 0..1073741824")]


@pytest.mark.parametrize("extra,msg", REFUSED, ids=["_".join(e).replace("--", "") for e, _ in REFUSED])
def test_binary_refuses_lead_options_before_any_file_or_device(extra, msg, tmp_path):
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
    assert r.returncode == 0 and b"--lead INT" in r.stdout and b"--stranded" in r.stdout
