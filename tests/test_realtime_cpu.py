"""`sigfish-amd realtime` without a GPU:
  * the schedule (sigfish_amd/csrc/cli/replay.hpp) driven by a stub session through a scripted table, as a stand-alone program
    under ASan + UBSan (tests/c/replay_schedule.cpp checks the schedule's properties itself), and the same table through the
    Python twin (sigfish_amd/realtime.py) with the same stub: the two traces must be equal line for line;
  * every option combination the command refuses exits non-zero with its message before anything touches a device (there is
    none here, so a device call would be the error reported instead)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime
from tests.realtime_util import BIN, write_model
from tests.util import GOLD, ROOT

CHUNK = 8
LENS = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK]


def script_for(i):
    """the table of tests/c/replay_schedule.cpp: (samples, chunk at which the stub fires or 0, early, mapped, poisoned)"""
    n = LENS[i % 6]
    timing = (i + i // 6) % 3
    k = 1 if timing == 0 else (n // CHUNK + 1 if timing == 1 else 0)
    return n, k, i % 2 == 0, i % 4 != 3, timing == 2 and i in (10, 15)


class StubSession:
    """answers by the table; the read's position in the file travels in its scaling's offset"""

    def __init__(self):
        self.chunks = {}

    def extend_raw(self, slots, raw, raw_off, scaling, end):
        rows, info = np.zeros(len(slots), S.RESULT_DTYPE), np.zeros(len(slots), S.SESSION_RAW_INFO_DTYPE)
        rows["rid"] = -1
        for i, sl in enumerate(slots):
            _, k, early, is_mapped, poison = script_for(int(scaling[i][1]))
            j = self.chunks[sl] = self.chunks.get(sl, 0) + 1
            status = S.RAW_ENDED if end[i] else 0
            if poison:
                status |= S.RAW_POISONED
                is_mapped = False
            elif k and j == k:
                if early:
                    status |= S.RAW_CALIBRATED
                    info["q_events"][i], rows["mapq"][i], is_mapped = 100, 60, True
                else:
                    status |= S.RAW_FULL
            info["status"][i] = status
            info["n_samples"][i] = raw_off[i + 1] - raw_off[i]
            if is_mapped:
                rows["valid"][i], rows["rid"][i] = 1, 0
        return rows, info

    def query_span(self, slots):
        return np.zeros(len(slots), np.uint64), np.zeros(len(slots), np.uint64)

    def reset(self, slots):
        for sl in slots:
            self.chunks[sl] = 0


def python_trace():
    out = []
    for channels in (1, 3, 8):
        for n_reads in (0, 1, 7, 20):
            reads = ((f"read{i}", dict(digitisation=1.0, offset=float(i), range=1.0), np.zeros(script_for(i)[0], np.int16)) for i in range(n_reads))
            trace = []
            order = [(t, c) for t, c, *_ in realtime.replay(None, reads, channels, CHUNK, 0, 25, 25, 30, 20, session=StubSession(), trace=trace)]
            assert order == sorted(order), "decisions come out in tick, then channel order"
            ticks = 1 + max((int(ln.split()[1]) for ln in trace if " send " in ln), default=-1)
            out += [f"case C={channels} reads={n_reads}", *trace, f"end ticks={ticks} reads={sum(' take ' in ln for ln in trace)}"]
    return out


def test_schedule_under_sanitizers_and_python_twin(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "replay_schedule")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "sigfish_amd", "csrc"),
                            "-o", exe, os.path.join(ROOT, "tests", "c", "replay_schedule.cpp")], capture_output=True, timeout=600)
    if build.returncode != 0 and b"sanitize" in build.stderr:
        pytest.skip("toolchain without sanitizer runtimes")
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    run = subprocess.run([exe], capture_output=True, timeout=300)
    lines = run.stdout.decode().splitlines()
    assert run.returncode == 0 and lines[-1] == "12 cases, 0 failures", (run.stdout[-2000:] + run.stderr[-3000:]).decode()
    assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]
    want = python_trace()
    # the table reaches what it is meant to: every reason with and without a line, an empty last chunk, a poisoned slot
    text = "\n".join(lines)
    for needle in ("reason=E line=1", "reason=F line=1", "reason=F line=0", "reason=R line=1", "reason=R line=0", f"first={CHUNK} n=0 end=1", "n=0 end=1"):
        assert needle in text, needle
    assert lines[:-1] == want


REFUSED = [(["--rna"], "--rna needs --invert"), (["--rna", "--invert", "--dtw-std"], "--dtw-std is not available"), (["--from-end"], "--from-end is not available"),
           (["-p", "-1"], "-p must be >= 0"), (["--sam"], "--sam is not available"), (["--secondary", "yes"], "--secondary yes is not available"),
           (["--ranks", "2"], "--ranks is not available"), (["--device", "0,1"], "exactly one GPU"), (["--norm-events", "24"], "--norm-events should be 25..q"),
           (["--norm-events", "251"], "--norm-events should be 25..q"), (["-q", "100", "--norm-events", "101"], "--norm-events should be 25..q")]


@pytest.mark.parametrize("extra,msg", REFUSED, ids=["_".join(e).replace("--", "") for e, _ in REFUSED])
def test_refused_options_exit_before_any_device_call(extra, msg, tmp_path):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    rna = "--rna" in extra
    model = write_model(tmp_path / "syn.model", 5 if rna else 6)
    files = [os.path.join(GOLD, "data", "rnasequin_sequences_2.4.fa" if rna else "nCoV-2019.reference.fasta"),
             os.path.join(GOLD, "data", "sequin_rna.blow5" if rna else "sp1_dna.blow5")]
    r = subprocess.run([BIN, "realtime", "--kmer-model", model, *extra, *files], capture_output=True, timeout=60)
    err = r.stderr.decode()
    assert r.returncode not in (0, None) and r.returncode > 0 and r.stdout == b"", (r.returncode, err)
    assert err.count("[sigfish-amd] ERROR:") == 1 and msg in err, err
    assert "accelerator" not in err and "hip" not in err.lower(), err


def test_help_lists_realtime():
    r = subprocess.run([BIN, "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"realtime" in r.stdout
    r = subprocess.run([BIN, "realtime", "--help"], capture_output=True, timeout=60)
    out = r.stdout.decode()
    assert r.returncode == 0 and "--channels" in out and "never calibrated and prints nothing" in out
