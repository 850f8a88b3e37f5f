"""The host rules in front of the DP as the library ships them (sigfish_amd/csrc/pre_rules.hpp), without a GPU: the stand-alone
program tests/c/pre_rules.cpp, built from that header alone with -Wall -Werror and once more under ASan + UBSan.  Its query
windows are compared with oracle.query_window, the project's independent pin of normalise_single (src/sigfish.c:433-480), its
status bits with the rule as this file states it, its tables with the reference's literals."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import ROOT

SHORT, DROPPED, AUTO_FAILED = 1, 2, 4  # sfa_query_info_t.status
FALLBACK = 50                          # src/sigfish.c:438-446
ORC_END = 0x020
COUNTS = list(range(81)) + [249, 250, 251, 299, 300, 301, 2048]
PREFIXES, QUERIES = (0, 1, 50, 60), (1, 25, 250)


def _build(tmp, sanitize):
    exe = str(tmp / ("pre_rules_san" if sanitize else "pre_rules"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "pre_rules.cpp")]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """[lines of the plain build, lines of the sanitizer build or None]"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("pre_rules")
    exe, build = _build(tmp, False)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    san, build = _build(tmp, True)
    # (the plain build went through, so the source compiles; only a toolchain that says its sanitizer runtime is missing counts as without)
    if build.returncode != 0 and any(m in build.stderr for m in (b"libasan", b"libubsan", b"-lasan", b"-lubsan", b"unrecognized command-line option", b"unsupported option")):
        san = None
    else:
        assert build.returncode == 0, build.stderr.decode()[-2000:]
    outs = []
    for prog in (exe, san):
        if prog is None:
            outs.append(None)
            continue
        run = subprocess.run([prog], capture_output=True, timeout=300)
        assert run.returncode == 0, (run.returncode, (run.stdout + run.stderr).decode()[-3000:])
        assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]
        outs.append(run.stdout.decode().splitlines())
    return outs


def test_both_builds_print_the_same_lines(outputs):
    if outputs[1] is None:
        pytest.skip("toolchain without sanitizer runtimes")
    assert outputs[0] == outputs[1] and len(outputs[0]) > 1000


def _windows(lines):
    """{(n_events, n_samples, prefix, query, from_end, auto, auto_event): (start, end, status, keep)}"""
    out = {}
    for ln in lines:
        if ln.startswith("win "):
            key, val = ln[4:].split(" -> ")
            out[tuple(int(x) for x in key.split())] = tuple(int(x) for x in val.split())
    return out


def test_query_window_equals_the_oracle_and_the_status_rule(outputs):
    from oracle import oracle as O

    got = _windows(outputs[0])
    seen = set()
    n_cells = 0
    for n in COUNTS:
        for query in QUERIES:
            cells = [(prefix, from_end, False, -1) for prefix in PREFIXES for from_end in (0, 1)]
            cells += [(-1, 0, True, a) for a in (-1, 0, 10, 55, n)]
            for prefix, from_end, auto, auto_event in cells:
                start, end, status, keep = got[(n, 4000, prefix, query, from_end, int(auto), auto_event)]
                cell = (n, prefix, query, from_end, auto, auto_event)
                # for the automatic start the oracle takes the resolved start, or 50 where the detection failed
                resolved = (auto_event if auto_event >= 0 else FALLBACK) if auto else prefix
                o_keep, o_start, o_end = O.query_window(n, resolved, query, ORC_END if from_end else 0)
                assert (start, end) == (o_start, o_end), cell
                # a read without events is not kept and reports nothing (sfa_align_raw's rule; the oracle, like the reference, is
                # never asked: with --from-end and no prefix it would keep an empty window)
                assert keep == (o_keep if n > 0 else 0), cell
                if n == 0:
                    assert (start, end, status, keep) == (0, 0, 0, 0), cell
                    continue
                if not from_end:
                    assert bool(status & DROPPED) == (not keep), cell                  # (it has events and samples)
                    assert bool(status & SHORT) == (bool(keep) and end - start < query), cell
                    assert bool(status & AUTO_FAILED) == (auto and auto_event < 0), cell
                else:
                    assert bool(status & SHORT) == (n - prefix - query < 0), cell
                    assert bool(status & DROPPED) == (n - prefix < 0), cell
                    assert not status & AUTO_FAILED, cell
                assert status & ~7 == 0, cell
                seen.add((from_end, status))
                n_cells += 1
                if not auto:  # without samples: not kept, 0..0, status 0, whatever the events
                    assert got[(n, 0, prefix, query, from_end, 0, -1)] == (0, 0, 0, 0), cell
    assert n_cells > 2500
    # the grid reaches every outcome of the rule
    assert seen == {(0, 0), (0, SHORT), (0, DROPPED), (0, AUTO_FAILED), (0, AUTO_FAILED | SHORT), (0, AUTO_FAILED | DROPPED),
                    (1, 0), (1, SHORT), (1, SHORT | DROPPED)}


def test_tables_equal_the_reference_literals(outputs):
    lines = outputs[0]
    # src/events.c:47-58:
    #   event_detection_defaults = {.window_length1 = 3, .window_length2 = 6, .threshold1 = 1.4f, .threshold2 = 9.0f, .peak_height = 0.2f};
    #   event_detection_rna      = {.window_length1 = 7, .window_length2 = 14, .threshold1 = 2.5f, .threshold2 = 9.0f, .peak_height = 1.0f};
    det = {int(ln.split()[1]): ln.split()[2:] for ln in lines if ln.startswith("det ")}
    for rna, (w1, w2, thr1, thr2, peak) in {0: (3, 6, "1.4", "9.0", "0.2"), 1: (7, 14, "2.5", "9.0", "1.0")}.items():
        assert [int(det[rna][0]), int(det[rna][1])] == [w1, w2]
        assert [np.float32(x) for x in det[rna][2:]] == [np.float32(thr1), np.float32(thr2), np.float32(peak)]
    # src/jnn.h: JNNV2_RNA_R9_ADAPTOR { .std_scale = 0.5, ..., .lo_thresh = 2000 }, JNNV2_RNA_RNA004_ADAPTOR { .std_scale = 0.7, ..., .lo_thresh = 500 };
    # RNA004 is pore 2 (sfa_set_pore), every other pore takes the R9 set
    ad = {int(ln.split()[1]): ln.split()[2:] for ln in lines if ln.startswith("adaptor ")}
    for pore, (lo, scale) in {0: (2000, "0.5"), 1: (2000, "0.5"), 2: (500, "0.7")}.items():
        assert int(ad[pore][0]) == lo and np.float32(ad[pore][1]) == np.float32(scale)
    assert [ln for ln in lines if ln.startswith("status ")] == [f"status {SHORT} {DROPPED} {AUTO_FAILED} fallback {FALLBACK}"]
    # room for len + 2 event records per read
    caps = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("cap ")]
    assert len(caps) == 4 and all(c == n + 2 for n, c in caps)
    # event_single(), src/sigfish.c:343: raw_unit = (float)range / (float)digitisation, offset as float
    scales = [ln for ln in lines if ln.startswith("scale ")]
    assert len(scales) == 3
    for ln in scales:
        args, bits = ln[6:].split(" -> ")
        dig, off, rng = (float(x) for x in args.split())
        want = [np.float32(off), np.float32(rng) / np.float32(dig)]
        assert [int(b, 16) for b in bits.split()] == [int(np.array(w, np.float32).view(np.uint32)) for w in want]
