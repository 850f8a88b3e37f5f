"""The schedule with truth without a GPU: replay.hpp under ASan + UBSan (tests/c/replay_truth.cpp, a scripted stub in place of the
session) against realtime.Schedule on the same script -- a `verdict` line directly behind every `decide` line, before a `close`
line, carrying the decide line's channel, read and sent; the trace without its verdict lines is the trace of the run without truth;
the truth tags and the `truth:` summary of both languages; the refusals of --truth / truth= without targets, which come before any
file, session or device is opened; -h names the option."""
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime
from tests.realtime_util import BIN, write_model
from tests.test_session_groups_cpu import _ask, _programs
from tests.util import GOLD


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return _programs(tmp_path_factory.mktemp("replay_truth"), "replay_truth.cpp", "replay_truth")


#          length, decided once this many samples are out, action, decided class, true class
READS = [(1000, 300, "A", "T", "T"),        # accepted and right: held for 7 ticks
         (1050, 300, "A", "T", "O"),        # accepted and wrong, in the same tick
         (900, 100, "U", "O", "T"),         # unblocked and wrong: the channel takes the next read at once
         (450, 10 ** 9, "A", "T", "T"),     # never decides early: ends ('R', proceeds), no decided class -> tv N
         (400, 10 ** 9, "A", "O", "N"),     # a read without truth
         (730, 730, "A", "T", "T"), (615, 200, "U", "O", "O"), (980, 400, "U", "O", "N"), (100, 50, "A", "T", "O"), (333, 100, "A", "N", "T")]


def _python_run(channels, chunk, truth, quota, reads):
    class Source:
        nxt = 0

        def take(self, channel):
            if self.nxt >= len(reads):
                return None
            self.nxt += 1
            return reads[self.nxt - 1][0]

    trace, src = [], Source()
    sch = realtime.Schedule(channels, chunk, trace, targets=True)
    if quota:
        sch.set_quota(S.QuotaBook(1, quota), ["g"])
    account = realtime.new_truth_account()
    sch.start(src)
    while sch.busy():
        es = sch.begin_tick()
        reason = ["E" if first + n >= reads[r][1] else ("R" if end else None) for _, r, first, n, end in es]
        line = [why == "E" for why in reason]
        action = [realtime.action_of(why, reads[r][2]) if why else None for (_, r, _, _, _), why in zip(es, reason)]
        marks = [(reads[r][4], S.truth_verdict(reads[r][3] if why == "E" else "N", reads[r][4])) if why else None for (_, r, _, _, _), why in zip(es, reason)]
        sent = [first + n for _, _, first, n, _ in es]
        now = list(es)
        held = sch.end_tick(reason, line, src, action, [0] * len(es) if quota else None, marks if truth else None)
        for i, why in enumerate(reason):
            if why:
                realtime.note_truth(account, marks[i][0], False, action[i], marks[i][1], sent[i], held[i], reads[now[i][1]][0])
                if truth:
                    trace.append(f"tags read={now[i][1]} " + realtime.truth_tags(dict(tt=marks[i][0], tv=marks[i][1])))
    trace.append(f"end tick={sch.tick}")
    return trace + (realtime.format_truth_summary(account).splitlines() if truth else [])


def _cpp_run(programs, channels, chunk, truth, quota, reads):
    text = f"{channels} {chunk} {int(truth)} {quota} {len(reads)}\n" + "".join(f"{n} {at} {a} {tc} {tt}\n" for n, at, a, tc, tt in reads)
    return _ask(programs, text)


@pytest.mark.parametrize("quota", [0, 2], ids=["no_quota", "quota_2"])
def test_verdict_lines_in_both_languages(programs, quota):
    got = _python_run(3, 100, True, quota, READS)
    assert got == _cpp_run(programs, 3, 100, True, quota, READS)
    plain = _python_run(3, 100, False, quota, READS)
    assert plain == _cpp_run(programs, 3, 100, False, quota, READS)
    # truth changes no decision: without the lines it adds, the trace is the run's without truth
    assert [ln for ln in got if " verdict " not in ln and not ln.startswith(("tags ", "[realtime] truth:"))] == plain
    assert not any(" verdict " in ln for ln in plain)
    # one verdict line directly behind every decide line, with its tick, channel, read and sent
    decides = [k for k, ln in enumerate(got) if " decide " in ln]
    assert len(decides) == len(READS) == sum(" verdict " in ln for ln in got)
    for k in decides:
        d, v = got[k].split(), got[k + 1].split()
        assert v[2] == "verdict" and (d[0], d[1], d[3], d[4], d[-1]) == (v[0], v[1], v[3], v[4], v[-1]), (got[k], got[k + 1])
        read = int(d[4].split("=")[1])
        early = d[5] == "reason=E"
        want_tv = S.truth_verdict(READS[read][3] if early else "N", READS[read][4])
        assert v[5] == f"tt={READS[read][4]}" and v[6] == f"tv={want_tv}", (got[k + 1], READS[read])
    assert "tick 2 decide ch=0 read=0 reason=E line=1 sent=300" in got and got[got.index("tick 2 decide ch=0 read=0 reason=E line=1 sent=300") + 1] == "tick 2 verdict ch=0 read=0 tt=T tv=C sent=300"
    assert "tick 2 verdict ch=1 read=1 tt=O tv=W sent=300" in got and "tick 0 verdict ch=2 read=2 tt=T tv=W sent=100" in got
    assert any(ln.endswith("read=3 tt=T tv=N sent=450") for ln in got)  # ended without a class decision
    if quota:  # the close line of the read that filled the quota comes behind its verdict line
        close = [k for k, ln in enumerate(got) if " close " in ln]
        assert len(close) == 1 and " verdict " in got[close[0] - 1] and " decide " in got[close[0] - 2]
    # the tags and the summary
    assert "tags read=0 \ttt:A:T\ttv:A:C" in got and "tags read=4 \ttt:A:N\ttv:A:N" in got
    summary = [ln for ln in got if ln.startswith("[realtime] truth:")]
    assert len(summary) == 4 and summary[0].startswith("[realtime] truth: T reads=5 ") and summary[2].startswith("[realtime] truth: N reads=2 ")
    recount = {c: sum(int(ln.split("sent=")[1]) for ln in got if " verdict " in ln and f" tt={c} " in ln) for c in "TON"}
    for c, ln in zip("TON", summary):
        assert f" sent={recount[c]} " in ln, (ln, recount)


def test_tags_and_summary_formatting():
    names = ["amp1", "orf1ab"]
    assert realtime.truth_tags(dict(tt="T", tv="W")) == "\ttt:A:T\ttv:A:W"
    for g, gv, want in ((0, "C", "amp1"), (1, "W", "orf1ab"), (2, "C", "*"), (None, "N", ".")):
        assert realtime.truth_tags(dict(tt="O", tv="N", true_group=g, gv=gv), names) == f"\ttt:A:O\ttv:A:N\ttn:Z:{want}\tgv:A:{gv}"
    acc = realtime.new_truth_account(True)
    assert realtime.format_truth_summary(acc).endswith("0 / 0 = -, of the file's samples 0 / 0 = -, enrichment by signal -\n")  # nothing is divided
    realtime.note_truth(acc, "T", True, "A", "C", 1000, 4000, 5000)
    realtime.note_truth(acc, "O", False, "U", "C", 500, 0, 5000)
    realtime.note_truth(acc, "N", False, "P", "N", 700, 0, 700)
    acc["groups"]["W"] += 1
    text = realtime.format_truth_summary(acc)
    assert text.splitlines()[0] == "[realtime] truth: T reads=1 sent=1000 held=4000 file=5000 A=1 U=0 P=0 C=1 W=0 N=0 edge=1"
    assert "[realtime] truth: groups C=0 W=1 N=0\n" in text
    assert text.endswith("(sent + held) 5000 / 5500 = 0.9091, of the file's samples 5000 / 10000 = 0.5000, enrichment by signal 1.8182\n")
    assert realtime.truth_enrichment(acc) == ((5000, 5500), (5000, 10000), 5000 * 10000 / (5500 * 5000))


# ---- the refusals, before any session, file or device ----
def test_replay_refuses_truth_without_targets_before_any_session():
    class NoAligner:
        def session(self, *a, **kw):
            raise AssertionError("a session was opened")

    with pytest.raises(S.SfaError, match="targets="):
        list(realtime.replay(NoAligner(), [], 2, 100, 3, 25, 70, 30, 5, truth={}))
    with pytest.raises(S.SfaError, match="targets="):
        list(realtime.replay(NoAligner(), [], 2, 100, 3, 25, 70, 30, 5, truth={"r": (0, 1, 2)}, summary={}))


@pytest.mark.parametrize("extra", [[], ["--min-events", "30"], ["--by-name"], ["--enrich", "--margin", "0.1"]], ids=["alone", "min_events", "by_name", "mode_and_margin"])
def test_binary_refuses_truth_without_targets_before_any_file_or_device(tmp_path, extra):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    model = write_model(tmp_path / "syn.model", 6)
    run = subprocess.run([BIN, "realtime", "--kmer-model", model, "--truth", str(tmp_path / "no_such.paf")] + extra
                         + [os.path.join(GOLD, "data", "nCoV-2019.reference.fasta"), str(tmp_path / "no_such.blow5")], capture_output=True, timeout=60)
    err = run.stderr.decode()
    assert run.returncode > 0 and run.stdout == b"", (run.returncode, err)
    assert err.count("[sigfish-amd] ERROR:") == 1 and "--targets" in err, err
    assert "no_such" not in err and "accelerator" not in err and "cannot open" not in err, err


def test_a_bad_truth_file_is_refused_before_the_blow5_file_and_the_device(tmp_path):
    """with --targets given, the truth file is read first: its refusal names file and line, not the BLOW5 file that does not exist"""
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    model = write_model(tmp_path / "syn.model", 6)
    paf = tmp_path / "truth.paf"
    paf.write_text("r0\t10\t0\t10\t+\tMN908947.3\t29903\t5\t9\nr1\t10\t0\t10\t+\tnowhere\t29903\t5\t9\n")
    run = subprocess.run([BIN, "realtime", "--kmer-model", model, "--truth", str(paf), "--targets", str(tmp_path / "no_such.bed"), "--enrich", "--margin", "0.1",
                          os.path.join(GOLD, "data", "nCoV-2019.reference.fasta"), str(tmp_path / "no_such.blow5")], capture_output=True, timeout=60)
    err = run.stderr.decode()
    assert run.returncode > 0 and run.stdout == b"" and err.count("[sigfish-amd] ERROR:") == 1, err
    assert "truth.paf:2: contig 'nowhere' is not in the reference" in err and "no_such" not in err and "accelerator" not in err, err


def test_help_names_the_option():
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    run = subprocess.run([BIN, "realtime", "-h"], capture_output=True, timeout=60)
    out = run.stdout.decode()
    assert run.returncode == 0 and "--truth FILE.paf" in out and "tt:A:" in out and "tv:A:" in out and "verdict" in out
