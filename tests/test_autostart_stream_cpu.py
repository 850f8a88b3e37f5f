"""The automatic query start of raw sessions without a GPU: the host twin of the target (sfa_auto_start_target) against
sfa_detect_query_start, the restated session rule (tests/autostart_oracle.py) under different schedules, the host arithmetic of
sfa_session_auto_bytes, the refusals that need no device, and the target function under ASan + UBSan."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib, synth
from tests.autostart_oracle import AutoTwin, cut, points_between
from tests.util import GOLD, ROOT

KINDS = [k for k in synth.RNA_POLYA_KINDS if k != "nonfinite"]


def _first_event_behind(ev, target):
    if target < 0:
        return -1
    i = int(np.searchsorted(ev["start"], np.uint64(target), "left"))
    return i if i < len(ev) else -1


def _check_reads(reads, pore):
    found = missing = 0
    for rid, dig, off, rng_, rate, raw in reads:
        meta = dict(digitisation=dig, offset=off, range=rng_)
        ev = S.detect_events(raw, meta, True)
        target = S.auto_start_target(raw, meta, pore)
        assert -1 <= target < len(raw), (rid, target)
        assert _first_event_behind(ev, target) == S.detect_query_start(raw, meta, ev, pore), (rid, target)
        found += target >= 0
        missing += target < 0
    return found, missing


def test_target_on_the_fixture_reads():
    reads = [(rid, m["digitisation"], m["offset"], m["range"], 0.0, raw) for rid, m, raw in S.Blow5File(os.path.join(GOLD, "data", "sequin_rna.blow5"))]
    found, _ = _check_reads(reads, 0)
    assert found >= 1  # (about the fixture: the golden case rna_q500_pauto finds starts)


@pytest.mark.parametrize("pore", [0, 2])
def test_target_on_synthetic_reads(pore):
    reads = synth.make_rna_polya_reads(400, seed=5, pore=pore, kinds=KINDS)
    found, missing = _check_reads(reads, pore)
    assert found >= 100 and missing >= 20, (found, missing)  # (about this test's own inputs: both outcomes)


def test_target_needs_more_than_2000_samples():
    (rid, dig, off, rng_, rate, raw), = synth.make_rna_polya_reads(1, seed=3, kinds=["normal"])
    meta = dict(digitisation=dig, offset=off, range=rng_)
    for n in (0, 1, 2000):
        assert S.auto_start_target(raw[:n], meta) == -1
    assert S.auto_start_target(raw, meta) >= 0


def test_points():
    assert points_between(0, 1600, False, 1600, 10 ** 6) == ([1600], None)
    assert points_between(1599, 1600, False, 1600, 10 ** 6) == ([1600], None)
    assert points_between(1600, 1601, False, 1600, 10 ** 6) == ([], None)
    assert points_between(100, 5000, False, 1600, 10 ** 6) == ([1600, 3200, 4800], None)
    assert points_between(100, 5000, True, 1600, 10 ** 6) == ([1600, 3200, 4800], 5000)
    assert points_between(100, 4800, True, 1600, 10 ** 6) == ([1600, 3200], 4800)  # a periodic point that is the final point
    assert points_between(8000, 9000, False, 1600, 8192) == ([], 8192)            # the cap is the final point ...
    assert points_between(8192, 9000, True, 1600, 8192) == ([], 8192)             # (only reached if the end comes first)
    assert points_between(7000, 9000, False, 1600, 8000) == ([], 8000)            # ... also where it is a multiple
    assert points_between(0, 5000, True, 0, 10 ** 6) == ([], 5000)
    assert points_between(0, 0, True, 1600, 10 ** 6) == ([], 0)


SCHEDULES = {"chunks": [1600], "ragged": [1, 1599, 1, 777, 3000], "whole": [10 ** 9]}


@pytest.mark.parametrize("max_samples", [10 ** 6, 8192])
def test_rule_does_not_depend_on_the_schedule(max_samples):
    """the twin under three schedules: equal state wherever two schedules have given a slot equally many samples, and the
    end state of all three"""
    reads = synth.make_rna_polya_reads(24, seed=11, kinds=[k for k in KINDS if k != "adaptor_hi"], body=(3000, 6000))
    frozen_mid = fallback = 0
    for rid, dig, off, rng_, rate, raw in reads:
        meta = dict(digitisation=dig, offset=off, range=rng_)
        runs = []
        for sizes in SCHEDULES.values():
            t, at, states = AutoTwin(meta, 0, 1600, max_samples, 4000, 100), 0, {}
            chunks = cut(len(raw), sizes)
            for i, c in enumerate(chunks):
                t.feed(raw[at:at + c], i == len(chunks) - 1)
                at += c
                states[at] = (t.state(), len(t.final()))
            runs.append(states)
            assert t.skip >= 0 and (t.status & 15) != S.AUTO_PENDING, (rid, t.state())  # an ended read has its skip
            assert t.target < t.frozen_at or t.target == -1, (rid, t.state())
        for a in runs[1:]:
            for n in set(runs[0]) & set(a):
                assert runs[0][n] == a[n], (rid, n)
        frozen_mid += t.target >= 0 and not t.status & S.AUTO_AT_FINAL
        fallback += t.failed()
    assert (frozen_mid >= 4 or max_samples == 8192) and fallback >= 2, (frozen_mid, fallback)  # (about this test's own inputs)


def test_whole_read_is_the_batch_answer():
    """every_samples = 0 and a cap above the read: the only point is the whole read, so skip and the fallback are select_query's"""
    reads = synth.make_rna_polya_reads(40, seed=5, kinds=[k for k in KINDS if k != "adaptor_hi"], body=(3000, 6000))
    for rid, dig, off, rng_, rate, raw in reads:
        meta = dict(digitisation=dig, offset=off, range=rng_)
        t = AutoTwin(meta, 0, 0, 10 ** 6, 10 ** 6, 100)
        t.feed(raw, True)
        ev = S.detect_events(raw, meta, True)
        st = S.detect_query_start(raw, meta, ev, 0) if len(ev) else -1
        assert (t.skip, t.failed()) == ((st, False) if st >= 0 else (50, True)), (rid, t.state(), st)


def test_bytes_and_names():
    L = _lib.load()
    assert L.sfa_session_auto_bytes(512, 65536) == 512 * (2 * 65536 + 16 + 4 * 65537) == S.session_auto_bytes(512, 65536)
    for bad in ((0, 100), (4, 0), (4, -1), (4, 2 ** 20 + 1), (-1, 100)):
        assert L.sfa_session_auto_bytes(*bad) < 0, bad
    with pytest.raises(S.SfaError):
        S.session_auto_bytes(4, 0)
    hdr = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    for name, value in (("PENDING", 0), ("RESOLVED", 1), ("NO_TARGET", 2), ("NO_EVENT", 3), ("BEYOND_MAX", 4), ("AT_FINAL", 16)):
        assert re.search(rf"#define\s+SFA_AUTO_{name}\s+{value}\b", hdr) and getattr(S, "AUTO_" + name) == value
    assert S.SESSION_AUTO_DTYPE.itemsize == 24


def test_null_handles_are_refused():
    L = _lib.load()
    assert L.sfa_session_raw_auto_start(None, 1600, 65536, 0) < 0 and b"null session" in L.sfa_last_error()
    assert L.sfa_session_auto_start(None, None, 0, None) < 0


def test_target_under_sanitizers(tmp_path):
    """tests/c/autostart_target_asan.cpp: prefixes of 0, 1, 2000, 2001 samples and around a closing poly-A, under ASan + UBSan on
    the host sources (CPU build only)"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "sigfish_amd", "csrc")
    exe = str(tmp_path / "autostart_target_asan")
    units = [os.path.join(csrc, u) for u in ("sfa_host.cpp", "host/blow5.cpp", "host/inflate.cpp", "host/events.cpp", "host/refio.cpp", "host/sam.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
                            "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "autostart_target_asan.cpp"), *units, "-lz", "-lpthread"],
                           capture_output=True, timeout=600)
    if build.returncode != 0 and b"sanitize" in build.stderr:
        pytest.skip("toolchain without sanitizer runtimes")
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    run = subprocess.run([exe], capture_output=True, timeout=300)
    assert run.returncode == 0 and b"\n0 failures" in run.stdout, (run.stdout + run.stderr).decode()[-3000:]
    assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]
