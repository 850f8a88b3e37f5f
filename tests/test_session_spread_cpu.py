"""Spread sessions without a GPU: the host rules as the library ships them (sigfish_amd/csrc/session_spread.hpp) through the
stand-alone program tests/c/session_spread.cpp, built from that header alone with -Wall -Werror and once more under ASan + UBSan
-- its own checks for G = 1, 2, 3 and 8, and its answers against a restatement of the rule here --, and what the header and
sfa_session_bytes say about the flag."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import ROOT


def _build(tmp, sanitize):
    exe = str(tmp / ("session_spread_san" if sanitize else "session_spread"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "session_spread.cpp")]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """[plain build, sanitizer build or None]"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("session_spread")
    exe, build = _build(tmp, False)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    san, build = _build(tmp, True)
    if build.returncode != 0 and any(m in build.stderr for m in (b"libasan", b"libubsan", b"-lasan", b"-lubsan", b"unrecognized command-line option", b"unsupported option")):
        san = None
    else:
        assert build.returncode == 0, build.stderr.decode()[-2000:]
    return [exe, san]


def _run(programs, args, text=""):
    outs = []
    for exe in programs:
        if exe is None:
            continue
        run = subprocess.run([exe] + args, input=text.encode(), capture_output=True, timeout=300)
        assert run.returncode == 0, (run.returncode, (run.stdout + run.stderr).decode()[-3000:])
        assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]
        outs.append(run.stdout.decode().splitlines())
    assert all(o == outs[0] for o in outs)
    return outs[0]


def test_the_programs_own_checks(programs):
    """placement and inverse, partition and scatter, offset tables, refusals, for G = 1, 2, 3, 8 (the C program's self check)"""
    out = _run(programs, [])
    assert len(out) == 1 and out[0].startswith("ok ") and int(out[0].split()[1]) > 10000, out


def test_the_program_runs_under_sanitizers(programs):
    if programs[1] is None:
        pytest.skip("toolchain without sanitizer runtimes")
    assert _run(programs[1:], [])[0].startswith("ok ")


def _restated(G, n_slots, once, slots, off):
    """the rule, stated again: refusal (why, index, slot) or per shard (local, index, off)"""
    seen = set()
    for i, s in enumerate(slots):
        if s < 0 or s >= n_slots:
            return (1, i, s)
        if once and s in seen:
            return (2, i, s)
        seen.add(s)
    out = []
    for r in range(G):
        idx = [i for i, s in enumerate(slots) if s % G == r]
        lens = [off[i + 1] - off[i] for i in idx]
        out.append(([slots[i] // G for i in idx], idx, [0] + list(np.cumsum(lens))))
    return out


def test_partition_equals_the_restatement(programs):
    rng = np.random.default_rng(8)
    calls = []
    for G in (1, 2, 3, 8):
        for n_slots in sorted({1, max(G - 1, 1), G, G + 1, 37}):
            every = list(range(n_slots))
            last_shard = [s for s in every if s % G == min(G, n_slots) - 1]
            for once, slots in ((1, every), (1, every[::-1]), (1, [n_slots - 1]), (1, last_shard), (1, []), (1, list(rng.permutation(n_slots)[:max(1, n_slots // 2)])),
                                (0, [0, 0, n_slots - 1]), (1, [0, 0]), (1, [n_slots]), (0, [-1]), (1, every + [0])):
                lens = rng.integers(0, 61, len(slots))  # chunks of 0 to 60 events
                if len(lens) > 1:
                    lens[rng.integers(0, len(lens) - 1)] = 0  # an empty chunk; the one at the end is not
                    lens[-1] = 17
                calls.append((G, n_slots, once, [int(s) for s in slots], [5] + [int(x) for x in 5 + np.cumsum(lens)]))  # (the caller's offsets need not begin at 0)
    text = "".join(f"part {G} {n} {once} {len(sl)} {' '.join(map(str, sl))} {' '.join(map(str, off))}\n" for G, n, once, sl, off in calls)
    lines = iter(_run(programs, ["-"], text))
    n_refused = 0
    for G, n_slots, once, slots, off in calls:
        want = _restated(G, n_slots, once, slots, off)
        first = next(lines).split()
        if isinstance(want, tuple):
            assert first == ["refused"] + [str(x) for x in want], (G, n_slots, slots)
            n_refused += 1
            continue
        for r, (local, idx, o) in enumerate(want):
            got = first if r == 0 else next(lines).split()
            fields = " ".join(got).split("|")
            assert fields[0].split() == ["shard", str(r), str(len(idx))], (G, n_slots, slots, r)
            assert [[int(x) for x in f.split()] for f in fields[1:]] == [local, idx, [int(x) for x in o]], (G, n_slots, slots, r)
    assert next(lines, None) is None and n_refused >= 4 * 4


def test_the_header_defines_the_flag():
    text = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    flags = {name: int(value, 16) for name, value in re.findall(r"#define (SFA_SESSION_[A-Z_]+) (0x[0-9a-fA-F]+)", text)}
    assert flags["SFA_SESSION_SPREAD"] == 0x10
    assert 0x2 not in flags.values() and "0x2 is not assigned" in text  # still refused as an unknown bit
    assert flags == {"SFA_SESSION_NO_START": 0x1, "SFA_SESSION_RESWEEP": 0x4, "SFA_SESSION_SPREAD": 0x10}
    import sigfish_amd as S
    assert S.SESSION_SPREAD == 0x10


def test_session_bytes_takes_the_flag():
    from sigfish_amd import _lib
    L = _lib.load()
    for cols, n in ((59_000, 512), (1, 1), (2_000_000, 7)):
        for fl in (0, 0x1, 0x4, 0x5):
            want = int(L.sfa_session_bytes(cols, n, fl))
            assert want > 0 and int(L.sfa_session_bytes(cols, n, fl | 0x10)) == want  # the session holds the same rows
    for fl in (0x18, 0x12, 0x2, 0x8, 0x80000010):
        assert int(L.sfa_session_bytes(59_000, 512, fl)) == -1  # SFA_EINVAL: unknown bits beside it
    # the share of device r of G: the slots (n - r + G - 1) // G add up to all of them
    for G in (1, 2, 3, 8):
        for n in (1, G, G + 1, 37, 512):
            assert sum((n - r + G - 1) // G for r in range(G)) == n
