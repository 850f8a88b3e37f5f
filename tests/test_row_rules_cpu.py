"""The row rule without a GPU: what the finalize kernels call (sigfish_amd/csrc/row_rules.hpp) through the stand-alone program
tests/c/row_rules.cpp, built from that header alone with -Wall -Werror and once more under ASan + UBSan.  This file writes the cases,
the program answers with what the shipped functions return, and the answers are held against the oracle: orc_mapq (oracle/oracle.py)
and update_aln (tests/secondary_oracle.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from sigfish_amd.api import RESULT_DTYPE
from tests.secondary_oracle import CAP, _update_aln
from tests.util import ROOT

INF = np.float32(np.inf)


def _build(tmp, sanitize):
    exe = str(tmp / ("row_rules_san" if sanitize else "row_rules"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "row_rules.cpp")]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """[plain build, sanitizer build or None], and where the requests go"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("row_rules")
    exe, build = _build(tmp, False)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    san, build = _build(tmp, True)
    if build.returncode != 0 and any(m in build.stderr for m in (b"libasan", b"libubsan", b"-lasan", b"-lubsan", b"unrecognized command-line option", b"unsupported option")):
        san = None
    else:
        assert build.returncode == 0, build.stderr.decode()[-2000:]
    return [exe, san], tmp


def _ask(programs, requests):
    """one answer line per request, the same from both builds"""
    (exes, tmp), outs = programs, []
    path = str(tmp / "requests.txt")
    with open(path, "w") as f:
        f.write("".join(r + "\n" for r in requests))
    for exe in exes:
        if exe is None:
            continue
        run = subprocess.run([exe, path], capture_output=True, timeout=300)
        assert run.returncode == 0, (run.returncode, (run.stdout + run.stderr).decode()[-3000:])
        assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]
        outs.append(run.stdout.decode().splitlines())
    assert all(o == outs[0] for o in outs)
    assert len(outs[0]) == len([r for r in requests if not r.startswith("tables")])
    return outs[0]


def _hex(x):
    return "%x" % int(np.float32(x).view(np.uint32))


def _f32(h):
    return np.uint32(int(h, 16)).view(np.float32)


def test_the_program_runs_under_sanitizers(programs):
    if programs[0][1] is None:
        pytest.skip("toolchain without sanitizer runtimes")
    assert _ask(([programs[0][1]], programs[1]), ["norow"])[0].startswith("row ")


def test_mapq_is_the_oracles_bit_for_bit(programs):
    from oracle import oracle as O
    edges = [(0, 0), (0, 1.5), (0, 1e-30), (3.25, 3.25), (1, INF), (40.5, INF), (INF, INF), (INF, 1), (-1, -1), (-2, 3), (2, -3), (-2, -3), (-0.0, 1),
             (1000, 1001), (1000, 1003), (1000, 1005), (1000, 1119), (1000, 1120), (1000, 1121), (1000, 999), (1000, 997), (8, 8.008),  # 500 d / score = k + .5
             (1, 1e8), (1, -1e8), (1, 4294968.0), (1, 4294967.5), (-1, 1e8), (1e-30, 1e10), (1e-38, 3e38), (-1e-38, 3e38), (1, 3e38), (1e-45, 1)]  # beyond 2^31
    rng = np.random.default_rng(575)
    pairs = [(np.float32(a), np.float32(b)) for a, b in edges]
    pairs += list(zip(rng.integers(0, 2**32, 2000, dtype=np.uint64).astype(np.uint32).view(np.float32), rng.integers(0, 2**32, 2000, dtype=np.uint64).astype(np.uint32).view(np.float32)))
    best = rng.uniform(0.5, 120, 2000).astype(np.float32)  # scores as alignments have them: the second a little above the best
    pairs += list(zip(best, (best * rng.uniform(1.0, 1.2, 2000)).astype(np.float32)))
    got = _ask(programs, [f"mapq {_hex(a)} {_hex(b)}" for a, b in pairs])
    want = [f"mapq {O.mapq(a, b)}" for a, b in pairs]
    assert got == want, [(p, g, w) for p, g, w in zip(pairs, got, want) if g != w][:5]
    assert len({w for w in want}) > 40  # (the cases do reach the values between 0 and 60)


VALUES = np.array([1.0, 1.25, 1.5, 2.0, 2.0, np.inf], np.float32)  # a handful of values, so that equals are frequent, and +inf among them


def _jobs(rng, n_jobs, empty=()):
    """windows of every job as (score, pos): 0 to 8 per job"""
    return [[] if j in empty else [(VALUES[rng.integers(len(VALUES))], 100 * j + w) for w in range(int(rng.integers(0, 9)))] for j in range(n_jobs)]


def _windows(jobs):
    return " ".join(f"{len(ws)} " + " ".join(f"{_hex(sc)} {pos}" for sc, pos in ws) for ws in jobs)


def test_merge_of_the_jobs_top2_is_update_aln(programs):
    """Every job's top-2 over its own windows, the jobs merged in processing order: best, second and what is kept of the best are the two
    top entries of update_aln over all windows in processing order.  Jobs without a window and a read without any among them.
    (Known and as before this header: a partial without a window is (+inf, +inf, nothing) and still wins a tie against +inf, so a read
    whose windows so far ALL scored +inf loses what it kept to a later job without a window, where update_aln keeps the last +inf
    window.  No case below is that one; on the device every job has a window and a read with a finite query has no +inf window.)"""
    rng = np.random.default_rng(577)
    reads = [_jobs(rng, int(rng.integers(1, 7))) for _ in range(300)]
    reads += [_jobs(rng, 4, empty=(1,)), _jobs(rng, 3, empty=(0,)), _jobs(rng, 5, empty=(4,)), _jobs(rng, 6, empty=(2, 3)), [[]], [[], [], []]]
    got = _ask(programs, [f"top2 {len(jobs)} {_windows(jobs)}" for jobs in reads])
    for jobs, line in zip(reads, got):
        whole = [(INF, -1, -1, -1, 0)] * CAP
        for job, ws in enumerate(jobs):
            for sc, pos in ws:
                _update_aln(whole, sc, job, pos, "+", 0)
        tag, best, second, pos, job = line.split()
        assert tag == "top2"
        assert (_f32(best), _f32(second), int(pos), int(job)) == (whole[4][0], whole[3][0], whole[4][3], whole[4][1]), (jobs, line)


@pytest.mark.parametrize("seed", range(6))
def test_merge_of_the_jobs_lists_is_update_aln(programs, seed):
    """Pass 1 keeps a list per (read, job) -- update_aln over that job's windows -- and the merge offers the jobs' lists to one list
    in job order, each in its own order (worst first, empty entries skipped).  That is update_aln over all windows in processing
    order, ties included: scores from a handful of values so that equals are frequent, and +inf among them.  The lists are the shipped
    top5_offer's, the merge the shipped register list's, with two payload words (batches) and with one (sessions); and the ranks as
    they are written out: an entry without a job or with a score that is not finite gives -1."""
    rng = np.random.default_rng(seed)
    n_jobs = int(rng.integers(1, 7))
    values = np.array([1.0, 1.25, 1.5, 2.0, 2.0, np.inf], np.float32)
    whole = [(np.float32(np.inf), -1, -1, -1, 0)] * CAP  # the reference's list over every window
    jobs = []
    for job in range(n_jobs):
        jobs.append([])
        for w in range(int(rng.integers(0, 9))):
            sc, pos = values[rng.integers(len(values))], 100 * job + w
            _update_aln(whole, sc, job, pos, "+", 0)
            jobs[-1].append((sc, pos))
    for line in _ask(programs, [f"top5 {P} {n_jobs} {_windows(jobs)}" for P in (2, 1)]):
        lst, ranks = (part.split() for part in line[len("top5 "):].split("|"))
        merged = [(_f32(lst[3 * m]), int(lst[3 * m + 1]), int(lst[3 * m + 2])) for m in range(CAP)]
        assert [(e[0], e[3], e[1]) for e in whole] == merged
        for k in range(CAP):
            sc, rid, _, pos, _ = whole[CAP - 1 - k]
            there = rid >= 0 and np.isfinite(sc)
            assert (_f32(ranks[3 * k]), int(ranks[3 * k + 1]), int(ranks[3 * k + 2])) == (sc, pos if there else -1, rid if there else -1), (k, line)


def test_rank_without_a_job_or_a_finite_score_is_minus_one(programs):
    """(the seeds above need not reach both: one finite window, one window of +inf, no window)"""
    line = _ask(programs, [f"top5 2 3 2 {_hex(1.5)} 7 {_hex(INF)} 9 0 1 {_hex(INF)} 205"])[0]
    ranks = line.split("|")[1].split()
    got = [(_f32(ranks[3 * k]), int(ranks[3 * k + 1]), int(ranks[3 * k + 2])) for k in range(CAP)]
    assert got == [(np.float32(1.5), 7, 0), (INF, -1, -1), (INF, -1, -1), (INF, -1, -1), (INF, -1, -1)]


def _row(line):
    tag, data = line.split()
    assert tag == "row" and len(data) == 2 * RESULT_DTYPE.itemsize
    return np.frombuffer(bytes.fromhex(data), RESULT_DTYPE)[0]


def _expect(**kw):
    r = np.zeros(1, RESULT_DTYPE)[0]
    r["rid"], r["pos_st"], r["pos_end"], r["score"], r["score2"] = -1, -1, -1, INF, INF
    for k, v in kw.items():
        r[k] = v
    return r


TABLES = "tables 4 0 0 1 1 + - + - 2 300 500 7 1000"  # jobs (contig, strand); contigs of 300 and 500 columns at offsets 7 and 1000


def test_rows(programs):
    from oracle import oracle as O
    got = _ask(programs, ["norow", TABLES, f"prow {_hex(20)} {_hex(21)} 3", f"prow {_hex(20)} {_hex(INF)} -1",
                          f"srow {_hex(30)} {_hex(INF)} 1 10 49", f"srow {_hex(30)} {_hex(31.5)} 2 0 499"])
    assert got[0] == "row " + np.array([(-1, -1, -1, np.inf, np.inf, 0, 0, 0, 0)], RESULT_DTYPE).tobytes().hex()  # byte for byte
    assert _row(got[1]) == _expect(valid=1, score=20, score2=21, rid=1, strand=ord("-"), mapq=O.mapq(20, 21))
    assert _row(got[2]) == _expect(valid=1, score=20)  # no window won: scores alone
    # rank 4: nothing behind it, score2 is +inf; '-' on contig 0: flipped, then the offset
    assert _row(got[3]) == _expect(valid=1, score=30, rid=0, strand=ord("-"), mapq=0, pos_st=300 - 49 + 7, pos_end=300 - 10 + 7)
    assert _row(got[4]) == _expect(valid=1, score=30, score2=31.5, rid=1, strand=ord("+"), mapq=0, pos_st=1000, pos_end=1499)


def test_place_and_drop_start(programs):
    cases = [(s, st, end) for s in "+-" for st, end in ((0, 299), (0, 0), (299, 299), (17, 120))]  # st = 0 and end = rl - 1 among them
    got = _ask(programs, [f"{what} {s} {st} {end} 300 7" for what in ("place", "drop") for s, st, end in cases])
    placed = [((st if s == "+" else 300 - end) + 7, (end if s == "+" else 300 - st) + 7) for s, st, end in cases]  # src/sigfish.c:971-975
    assert got[:len(cases)] == [f"place {a} {b}" for a, b in placed]
    # without start columns the coordinate that came from the start is unknown: pos_st on '+', pos_end on '-'
    assert got[len(cases):] == [f"place {-1 if s == '+' else a} {b if s == '+' else -1}" for (s, _, _), (a, b) in zip(cases, placed)]


def test_span_bucket(programs):
    cases = [((5, 4, 100), -1), ((-1, 10, 100), -1), ((0, 10, 0), -1),  # end < st, no start, no query: no alignment
             ((0, 0, 100), 0), ((10, 109, 100), 16), ((10, 108, 100), 15),  # a span of qlen columns is bucket 16
             ((0, 193, 100), 31), ((0, 192, 100), 30), ((0, 100000, 100), 31), ((0, 2**31 - 2, 1), 31)]  # the last bucket is open
    got = _ask(programs, [f"span {st} {end} {q}" for (st, end, q), _ in cases])
    assert got == [f"span {b}" for _, b in cases]
