"""The host rules of a session's target classes without a GPU: the stand-alone program tests/c/target_rules.cpp, built from
sigfish_amd/csrc/target_rules.hpp alone with -Wall -Werror and once more under ASan + UBSan (its selftest checks the mask against a
loop over place_col of row_rules.hpp, every refusal and the decision table); the Python restatement of the mask the GPU test
relies on (tests/targets_oracle.py) against the header's; the decision table through the library's sfa_target_decide; the BED
reader; the schedule with targets (hold ticks, channels freed by an unblock) as replay.hpp and its Python twin run it, against a
scripted stub; the option refusals of replay() and of the binary, which come before any file or device is opened."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from tests import targets_oracle as T
from tests.util import ROOT

INF = float("inf")


def _build(tmp, sanitize):
    exe = str(tmp / ("target_rules_san" if sanitize else "target_rules"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "target_rules.cpp")]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """[plain build, sanitizer build or None]: every request goes through all of them, and their answers must be the same lines"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("target_rules")
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


def test_selftest_plain_and_under_sanitizers(programs):
    line = _ask(programs, "selftest\n")[-1].split()
    assert line[:2] == ["selftest", "ok"] and int(line[2]) > 500


def test_the_program_runs_under_sanitizers(programs):
    if programs[1] is None:
        pytest.skip("toolchain without sanitizer runtimes")
    assert _ask(programs[1:], "mask 2 1 5 0 1 0 0 6\n") == ["mask 10 0 -1 000003ff"]


# ---- the Python restatement of the mask against the header's ----
LENS = [1, 31, 32, 33, 64, 65, 300]
OFFS = [0, 7, 0, 100, 3, 0, 1000]
LISTS = {
    "empty": [],
    "whole contigs": [(r, OFFS[r], OFFS[r] + LENS[r] + 1) for r in range(7)],
    "word edges": [(1, OFFS[1] + 1, OFFS[1] + 31), (2, 0, 32), (3, OFFS[3] + 32, OFFS[3] + 34), (4, OFFS[4] + 31, OFFS[4] + 33), (6, OFFS[6] + 64, OFFS[6] + 96)],
    "overlapping, unsorted": [(6, OFFS[6] + 200, OFFS[6] + 260), (6, OFFS[6] + 10, OFFS[6] + 40), (6, OFFS[6] + 30, OFFS[6] + 64), (6, OFFS[6] + 64, OFFS[6] + 65),
                              (3, OFFS[3] + 5, OFFS[3] + 20), (0, 0, 2), (6, OFFS[6] + 10, OFFS[6] + 40)],
    "below the offset": [(3, 0, 100), (6, 5, 1000)],
}


@pytest.mark.parametrize("strands", [1, 2], ids=["rna_one_strand", "dna_two_strands"])
@pytest.mark.parametrize("name", list(LISTS))
def test_python_mask_equals_the_headers(programs, name, strands):
    t = LISTS[name]
    text = f"mask {strands} {len(LENS)} " + " ".join(f"{n} {o}" for n, o in zip(LENS, OFFS)) + f" {len(t)} " + " ".join(f"{c} {b} {e}" for c, b, e in t) + "\n"
    tag, on, first_on, first_off, *words = _ask(programs, text)[0].split()
    mask = T.mask_of(t, LENS, OFFS, strands)
    assert tag == "mask" and int(on) == int(mask.sum())
    assert [int(w, 16) for w in words] == T.words_of(mask)
    assert int(first_on) == (int(np.flatnonzero(mask)[0]) if mask.any() else -1)
    assert int(first_off) == (int(np.flatnonzero(~mask)[0]) if not mask.all() else -1)
    if name in ("empty", "below the offset"):
        assert int(on) == 0
    if name == "whole contigs":
        assert mask.all()


REFUSALS = [((-1, 0, 1), "contig"), ((7, 0, 1), "contig"), ((2, -1, 4), "negative"), ((2, 4, 4), "empty"), ((2, 5, 4), "empty"), ((2, 0, 34), "beyond"),
            ((3, 100, 135), "beyond")]


@pytest.mark.parametrize("target,word", REFUSALS)
def test_refusals(programs, target, word):
    text = f"mask 2 {len(LENS)} " + " ".join(f"{n} {o}" for n, o in zip(LENS, OFFS)) + " 2 6 1000 1001 " + " ".join(str(x) for x in target) + "\n"
    line = _ask(programs, text)[0]
    assert line.startswith("refused target 1:") and word in line


# ---- the decision table: the header's function (the program) and the library's export give the same answers ----
#        on    off  on_rid off_rid  n  valid mode min margin  want
TABLE = [(10.0, 60.0, 0, 1, 100, 1, 0, 100, 0.5, "A"),   # margin exactly met, n at min_events
         (10.0, 60.0, 0, 1, 100, 1, 1, 100, 0.5, "U"),
         (10.0, 60.0, 0, 1, 99, 1, 0, 100, 0.5, None),   # n just below min_events
         (10.0, 60.0, 0, 1, 99, 1, 1, 100, 0.5, None),
         (10.0, 59.5, 0, 1, 100, 1, 0, 100, 0.5, None),  # margin just missed
         (60.0, 10.0, 0, 1, 100, 1, 0, 100, 0.5, "U"),   # off target, exactly met
         (60.0, 10.0, 0, 1, 100, 1, 1, 100, 0.5, "A"),
         (59.5, 10.0, 0, 1, 100, 1, 1, 100, 0.5, None),
         (INF, 10.0, -1, 1, 100, 1, 0, 100, 0.5, "U"),   # nothing on target
         (INF, 10.0, -1, 1, 100, 1, 1, 100, 0.5, "A"),
         (10.0, INF, 0, -1, 100, 1, 0, 100, 0.5, "A"),   # nothing off target
         (10.0, INF, 0, -1, 100, 1, 1, 100, 0.5, "U"),
         (INF, INF, -1, -1, 100, 1, 0, 100, 0.5, None),  # both empty
         (INF, INF, -1, -1, 100, 1, 1, 100, 0.5, None),
         (10.0, 60.0, 0, 1, 100, 0, 0, 100, 0.5, None),  # valid = 0
         (10.0, 60.0, 0, 1, 100, 1, 2, 100, 0.5, None),  # an unknown mode
         (10.0, 10.0, 0, 1, 100, 1, 0, 100, 0.0, "A")]   # margin 0, equal scores: on target is asked first


def test_decision_table(programs):
    text = "".join("decide " + " ".join(str(x) for x in row[:9]) + "\n" for row in TABLE)
    lines = _ask(programs, text)
    for row, line in zip(TABLE, lines):
        on, off, on_rid, off_rid, n, valid, mode, min_events, margin, want = row
        assert line == f"decide {want or '-'}", row
        rec = np.zeros(1, S.CLASS_DTYPE)
        rec[0] = (on, off, on_rid, 5, off_rid, 7, ord("+"), ord("-"), (0, 0), n, valid)
        assert S.target_decide(rec, mode, min_events, margin) == want, row


def test_read_targets(tmp_path):
    names = ["chrA", "chrB", "chrC"]
    bed = tmp_path / "t.bed"
    bed.write_text("# a comment\ntrack name=x\nbrowser position chrA:1-2\n\nchrB\t5\t40\tname\t0\t+\nchrA 0 7\nchrB\t5\t40\n")
    got = S.read_targets(str(bed), names)
    assert got.dtype == S.TARGET_DTYPE and [tuple(int(v) for v in x) for x in got] == [(1, 5, 40), (0, 0, 7), (1, 5, 40)]
    for text, word in (("chrZ\t1\t2\n", "not in the reference"), ("chrA\t1\n", "three columns"), ("chrA\tx\t2\n", "integers")):
        bed.write_text(text)
        with pytest.raises(S.SfaError, match=word):
            S.read_targets(str(bed), names)
    bed.write_text("")
    assert len(S.read_targets(str(bed), names)) == 0


# ---- the schedule with targets: the C++ header (a stand-alone program with a scripted stub) and the Python twin ----
from sigfish_amd import realtime  # noqa: E402
from tests.realtime_util import BIN, write_model  # noqa: E402
from tests.util import GOLD  # noqa: E402


def _python_trace(channels, chunk, targets, reads):
    """reads: [(length, decide once this many samples are sent, action)] -> the trace lines and the end line of the C++ stub"""
    class Source:
        nxt = 0

        def take(self, channel):
            if self.nxt >= len(reads):
                return None
            self.nxt += 1
            return reads[self.nxt - 1][0]

    trace, src, total_held = [], Source(), 0
    sch = realtime.Schedule(channels, chunk, trace, targets=targets)
    sch.start(src)
    while sch.busy():
        es = sch.begin_tick()
        reason = ["E" if first + n >= reads[r][1] else ("R" if end else None) for _, r, first, n, end in es]
        line = [why == "E" for why in reason]
        action = [realtime.action_of(why, reads[r][2]) if why else None for (_, r, _, _, _), why in zip(es, reason)]
        held = sch.end_tick(reason, line, src, action if targets else None)
        total_held += sum(held)
    return trace + [f"end tick={sch.tick} held={total_held}"]


@pytest.fixture(scope="module")
def schedule_program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("replay_targets") / "replay_targets")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I",
                            os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "replay_targets.cpp")], capture_output=True, timeout=600)
    if build.returncode != 0 and any(m in build.stderr for m in (b"libasan", b"libubsan", b"-lasan", b"-lubsan")):
        build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe,
                                os.path.join(ROOT, "tests", "c", "replay_targets.cpp")], capture_output=True, timeout=600)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    return exe


def _cpp_trace(exe, channels, chunk, targets, reads):
    text = f"{channels} {chunk} {int(targets)} {len(reads)}\n" + "".join(f"{n} {at} {a}\n" for n, at, a in reads)
    run = subprocess.run([exe], input=text.encode(), capture_output=True, timeout=120)
    assert run.returncode == 0 and b"runtime error" not in run.stderr and b"AddressSanitizer" not in run.stderr, run.stderr.decode()[-2000:]
    return run.stdout.decode().splitlines()


#          length, decided once this many samples are out, action
READS = [(1000, 300, "A"),   # accepted after 3 chunks of 100: 700 left, a multiple of the chunk -> 7 hold ticks
         (1050, 200, "A"),   # 850 left, no multiple -> 9 hold ticks
         (900, 100, "U"),    # unblocked at tick 0: the channel takes the next read, which sends from tick 1
         (450, 10 ** 9, "A"),  # never decides early: ends ('R', proceeds) with its last, short chunk -> nothing left, no hold
         (400, 10 ** 9, "A"),  # a multiple of the chunk: the empty last chunk carries the end
         (730, 730, "A"),    # accepted with its last chunk: nothing left
         (615, 200, "P"), (980, 400, "U"), (100, 50, "A"), (333, 100, "A")]


def test_hold_ticks_and_freed_channels(schedule_program):
    got = _python_trace(3, 100, True, READS)
    assert got == _cpp_trace(schedule_program, 3, 100, True, READS)
    text = "\n".join(got)
    # read 0 on channel 0: decided at tick 2 (300 sent), held for ticks 3..9, left counting 7..1; the next read of the channel at 10
    assert "tick 2 decide ch=0 read=0 reason=E line=1 sent=300" in got
    assert [ln for ln in got if " hold ch=0 read=0 " in ln] == [f"tick {3 + k} hold ch=0 read=0 left={7 - k}" for k in range(7)]
    take0 = [ln for ln in got if " take ch=0 " in ln]
    assert take0[1].startswith("tick 9 take ch=0 ") and f"tick 10 send ch=0 read={take0[1].split('read=')[1].split()[0]} first=0" in text
    # read 1: 850 left over a chunk of 100 is 9 hold ticks
    assert len([ln for ln in got if " hold ch=1 read=1 " in ln]) == 9
    # read 2 is unblocked at tick 0: no hold line, and its channel's next read sends at tick 1
    assert not any(" hold ch=2 read=2 " in ln for ln in got)
    assert "tick 0 take ch=2 read=3 len=450" in got and "tick 1 send ch=2 read=3 first=0 n=100 end=0" in got
    # reads that end with nothing left are not held
    for r in (3, 4, 5):
        assert not any(f" hold ch=" in ln and f" read={r} " in ln for ln in got), r
    assert "n=0 end=1" in text


def test_without_targets_the_trace_is_what_it_was(schedule_program):
    got = _python_trace(3, 100, False, READS)
    assert got == _cpp_trace(schedule_program, 3, 100, False, READS)
    assert not any(" hold " in ln for ln in got) and got[-1].endswith("held=0")
    # ... and it is the trace of a schedule that has never heard of targets: every decision frees its channel in the same tick
    for ln in got:
        if " decide " in ln:
            tick, ch = int(ln.split()[1]), ln.split("ch=")[1].split()[0]
            nxt = [x for x in got if x.startswith(f"tick {tick} take ch={ch} ")]
            assert nxt or not any(x.startswith(f"tick {tick} take ") for x in got), ln


def test_replay_refuses_bad_target_arguments_before_any_session():
    class NoAligner:
        def session(self, *a, **kw):
            raise AssertionError("a session was opened")

    t = [(0, 0, 10)]
    for kw, word in ((dict(targets=t, margin=0.1), "ENRICH"), (dict(targets=t, mode=S.ENRICH), "margin"), (dict(targets=t, mode=S.ENRICH, margin=0.1, resweep=True), "resweep"),
                     (dict(margin=0.1), "belong to targets"), (dict(mode=S.DEPLETE), "belong to targets")):
        with pytest.raises(S.SfaError, match=word):
            list(realtime.replay(NoAligner(), [], 2, 100, 3, 25, 70, 30, 5, **kw))


BED = "nCoV.bed"
REFUSED = [(["--targets", BED, "--enrich"], "--targets needs --margin"), (["--targets", BED, "--margin", "0.1"], "exactly one of --enrich and --deplete"),
           (["--targets", BED, "--enrich", "--deplete", "--margin", "0.1"], "exactly one of --enrich and --deplete"), (["--enrich"], "belong to --targets"),
           (["--margin", "0.1"], "belong to --targets"), (["--targets", BED, "--enrich", "--margin", "x"], "--margin should be a number"),
           (["--targets", BED, "--enrich", "--margin", "-1"], "--margin should be a number"),
           (["--targets", BED, "--deplete", "--margin", "0.1", "--resweep"], "not available with --resweep")]


@pytest.mark.parametrize("extra,msg", REFUSED, ids=["_".join(e).replace("--", "") for e, _ in REFUSED])
def test_binary_refuses_target_options_before_any_file_or_device(extra, msg, tmp_path):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    model = write_model(tmp_path / "syn.model", 6)
    # (the BED file and the reads do not exist: a refusal that came after opening either would name them)
    r = subprocess.run([BIN, "realtime", "--kmer-model", model, *extra, os.path.join(GOLD, "data", "nCoV-2019.reference.fasta"), str(tmp_path / "no_such.blow5")],
                       capture_output=True, timeout=60)
    err = r.stderr.decode()
    assert r.returncode > 0 and r.stdout == b"", (r.returncode, err)
    assert err.count("[sigfish-amd] ERROR:") == 1 and msg in err, err
    assert "no_such" not in err and BED not in err.split("ERROR:")[1].replace("FILE.bed", "") and "accelerator" not in err, err
