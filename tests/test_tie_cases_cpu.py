"""Every case of tests/tie_cases.py is what it claims, shown with the oracle and the host-pure planner alone (no GPU): the named
last-row columns hold bitwise equal values, each is the minimum of its window, the reference reports the claimed candidate with
score == score2 where claimed, the top-5 list is the claimed one -- and the boundaries the ties are said to lie across are real:
window edges w * qlen, the segment ranges, and the chunk split of the batch sizes tests/test_tie_cases_gpu.py runs, the latter
from tests/c/tie_plan.cpp (sfa_plan.hpp as a stand-alone program).  A case whose tie does not hold fails; none is skipped."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import tie_cases as T
from tests.secondary_oracle import top5
from tests.util import ROOT

CSRC = os.path.join(ROOT, "sigfish_amd", "csrc")


def oracle_ref(O, case):
    names = [f"c{i}" for i in range(len(case.lens))]
    return O.RefSynth(names, [n + 5 for n in case.lens], case.lens, case.offs, case.forward, case.reverse)


_rows = {}


def last_rows(O, case):
    """per read {(contig, strand): last-row values}; --dtw-std: the last row of the std_dtw matrix (its last column is the candidate)"""
    if case.name not in _rows:
        oref = oracle_ref(O, case)
        out = []
        for i in range(len(case.q_off) - 1):
            ev = case.q[case.q_off[i]:case.q_off[i + 1]]
            if case.flag & T.DTW:
                query = ev[::-1].copy() if not case.flag & T.INV else ev
                out.append({(c, "+"): O.std_dtw(query, y)[-1].copy() for c, y in enumerate(case.forward)})
            else:
                out.append({(c, s): cost for c, s, cost, _ in O.last_rows(ev, oref, case.flag)})
        _rows[case.name] = out
    return _rows[case.name]


def window_of(case, col):
    return 0 if case.flag & T.DTW else col // case.qlen


def test_the_case_list_reaches_every_situation_and_class():
    fns = {T._TABLE[n][0].__name__ for n in T.NAMES}
    assert fns == {"in_window_adjacent", "in_window_far", "edge_adjacent", "windows_apart", "last_partial", "short_contig_twins", "contig_twins",
                   "strand_twin", "segment_twins", "many_windows", "many_contigs", "rank5_tie", "std_twins", "zero_score"}
    assert {T._TABLE[n][2] for n in T.NAMES} >= {24, 64, 250, 600, 1024, 1500, 2048, 2100, 4500}
    assert {T._TABLE[n][1] for n in T.NAMES} == {"dna", "rna", "rna_std", "rna_inv"}
    assert [n for n in T.NAMES if T.build(n).zero] == ["zero_score_rna_q250"]
    for n in T.NAMES:
        c = T.build(n)
        assert sum(c.lens) <= 9100 and len(c.q_off) - 1 <= 40 and (np.diff(c.q_off) == c.qlen).all(), n
        assert c.qlen <= 2048 or len(c.q_off) - 1 <= 2, n


@pytest.mark.parametrize("name", T.NAMES)
def test_named_columns_tie_and_are_their_windows_minima(oracle, name):
    case = T.build(name)
    for i, rows in enumerate(last_rows(oracle, case)):
        for cols in case.ties:
            vals = [rows[(c, s)][col] for c, s, col in cols]
            assert len({v.tobytes() for v in vals}) == 1, (name, i, cols, vals)
            assert np.isfinite(vals[0]) and (vals[0] == 0) == case.zero, (name, i, vals[0])
            for c, s, col in cols:
                row = rows[(c, s)]
                if case.flag & T.DTW:
                    assert col == len(row) - 1  # the one candidate of a contig
                    continue
                w0, w1 = T.windows(len(row), case.qlen)[window_of(case, col)]
                assert w0 <= col < w1 and row[col] == row[w0:w1].min(), (name, i, c, s, col, int(np.argmin(row[w0:w1])) + w0)
                first = w0 + int(np.argmin(row[w0:w1]))  # scan_windows: the first strict minimum
                assert first == col or (first < col and (c, s, first) in cols), (name, i, c, s, col, first)


@pytest.mark.parametrize("name", T.NAMES)
def test_the_reference_reports_the_claimed_winner(oracle, name):
    case = T.build(name)
    oref = oracle_ref(oracle, case)
    want = oracle.align_batch(case.q, case.q_off, oref, case.flag, threads=8)
    c, s, col = case.winner
    rl, off = case.lens[c], case.offs[c]
    for i, rows in enumerate(last_rows(oracle, case)):
        r = want[i]
        assert r["valid"] == 1 and r["rid"] == c and chr(r["strand"]) == s, (name, i, r)
        assert (r["pos_end"] == col + off) if s == "+" else (r["pos_st"] == rl - col + off), (name, i, r, col)  # src/sigfish.c:971-975
        assert r["score"].tobytes() == rows[(c, s)][col].tobytes(), (name, i, r)
        if case.top_tie:
            assert r["score"].tobytes() == r["score2"].tobytes(), (name, i, r)
            assert r["mapq"] == 0
        else:
            assert r["score2"] > r["score"], (name, i, r)
        if not case.zero:
            assert r["score"] > 0


@pytest.mark.parametrize("name", T.MANY)
def test_the_claimed_five_stay_in_the_claimed_order(oracle, name):
    case = T.build(name)
    oref = oracle_ref(oracle, case)
    for i, rows in enumerate(last_rows(oracle, case)):
        aln = top5(oracle, case.q[case.q_off[i]:case.q_off[i + 1]], oref, case.flag)
        got = [(rid, d, end) for _, rid, _, end, d in aln[::-1]]
        assert got == list(case.top5), (name, i, got)
        out = [x for x in case.ties[-1] if x not in case.top5]  # tied candidates that fell out ...
        assert out and all(rows[(c, s)][col].tobytes() == aln[0][0].tobytes() for c, s, col in out), (name, i)  # ... tie with the fifth place
        assert case.top5[4] in case.ties[-1] and all(o < case.top5[4] for o in out)  # and come earlier in processing order


def test_claimed_window_edges():
    """w * qlen, recomputed: which window every named column lies in"""
    for name in T.NAMES:
        case = T.build(name)
        fn = T._TABLE[name][0].__name__
        q = case.qlen
        wins = [[col // q for _, _, col in cols] for cols in case.ties]
        if fn in ("in_window_adjacent", "in_window_far"):
            a, b = case.ties[0]
            assert wins[0] == [2, 2] and wins[1:] in ([], [[1, 2]]) and b[2] - a[2] == (1 if fn == "in_window_adjacent" else q // 2) and case.winner == a, name
        elif fn == "edge_adjacent":
            a, b = case.ties[2]
            assert a[2] % q == q - 1 and b[2] == a[2] + 1 and b[2] % q == 0 and case.winner == b, name
            if q > 2100:
                assert b[2] // q == (case.lens[0] - 1) // q and case.lens[0] % q  # the later one in the last, partial window
        elif fn == "windows_apart":
            assert wins == [[1, 3]], name
        elif fn == "last_partial":
            assert wins == [[1, 3]] and case.lens[0] % q and (case.lens[0] - 1) // q == 3, name
        elif fn == "short_contig_twins":
            assert wins == [[0, 0]] and max(case.lens) < q, name
        elif fn == "many_windows":
            assert wins == [[1, 3, 5, 7, 9, 11, 13]], name
        elif fn == "segment_twins":
            assert all(a < b for w in wins for a, b in zip(w, w[1:])) or len(case.ties) == 3, name


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """(case name, copies, lane_widening, column_segments, secondary) -> the plan tests/c/tie_plan.cpp prints"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("tie_plan") / "tie_plan")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "c", "tie_plan.cpp")],
                           capture_output=True, timeout=600)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    keys, text = [], []
    for name in T.NAMES:
        case = T.build(name)
        for reps in T.REPS:
            for sec in (0, 4):
                keys.append((name, reps, 0, 0, sec))
                text.append(T.plan_request(case, reps, secondary=sec))
        if case.options:
            keys.append((name, 1, case.options["lane_widening"], case.options["column_segments"], 0))
            text.append(T.plan_request(case, 1, widening=keys[-1][2], segments=keys[-1][3]))
    run = subprocess.run([exe], input="".join(text).encode(), capture_output=True, timeout=600)
    assert run.returncode == 0, (run.returncode, (run.stdout + run.stderr).decode()[-2000:])
    lines = run.stdout.decode().splitlines()
    assert lines[-1] == f"done {len(keys)}" and len(lines) == len(keys) + 1
    out = {}
    for k, ln in zip(keys, lines):
        v = [int(x) for x in ln.split()[1:]]
        out[k] = dict(widening=v[0], n_quads=v[1], n_chunks=v[2], n_seg=v[3], warm=v[4], max_lanes=v[5], chunk_begin=v[6:])
    return out


def _chunk_of(plan, job):
    return int(np.searchsorted(plan["chunk_begin"], job, side="right")) - 1


def test_twin_contigs_lie_across_a_chunk_boundary(plans):
    """the job list of the large batch is really split (fewer chunks than jobs), the twins' jobs lie in different chunks at
    every batch size, and some chunk of the large batch holds two jobs"""
    assert len(T.SPLIT) == 4
    for name in T.SPLIT:
        case = T.build(name)
        n_jobs = len(T.job_lens(case))
        for reps in T.REPS:
            for sec in (0, 4):
                p = plans[(name, reps, 0, 0, sec)]
                assert p["n_seg"] == 1 and p["chunk_begin"][0] == 0 and p["chunk_begin"][-1] == n_jobs, (name, reps)
                for a, b in case.chunk_pairs:
                    assert a < b and _chunk_of(p, a) < _chunk_of(p, b), (name, reps, p["chunk_begin"])
                if reps in case.real_split:
                    assert 1 < p["n_chunks"] < n_jobs and max(np.diff(p["chunk_begin"])) >= 2, (name, reps, p)
                    a, b = case.chunk_pairs[0]
                    if b == a + 1:  # neighbours: the cut falls right between them
                        assert b in p["chunk_begin"], (name, reps, p["chunk_begin"])
        assert len({plans[(name, reps, 0, 0, 0)]["widening"] for reps in T.REPS}) > 1, name  # the batch size alone changes the shape


def test_segment_twins_lie_across_a_hand_over(plans):
    assert len(T.SEGMENTED) == 4
    for name in T.SEGMENTED:
        case = T.build(name)
        n_seg = case.options["column_segments"]
        p = plans[(name, 1, 4, n_seg, 0)]
        assert p["widening"] == 4 and p["max_lanes"] == 64 and p["n_seg"] == n_seg and p["n_chunks"] == n_seg * len(T.job_lens(case)), (name, p)
        assert case.segments
        for n, job, a, b in case.segments:
            rlen = T.job_lens(case)[job]
            ranges = [T.segment_range(rlen, case.qlen, n, p["warm"], s) for s in range(n)]
            assert not any(r[3] for r in ranges) and ranges[-1][4] and ranges[0][1] == 0 and ranges[-1][2] == rlen
            assert all(x[2] == y[1] for x, y in zip(ranges, ranges[1:]))  # real columns: one segment ends where the next begins
            seg = lambda col: next(s for s, r in enumerate(ranges) if r[1] <= col < r[2])
            assert seg(a) < seg(b), (name, a, b, ranges)
        assert {seg for _, _, a, b in case.segments for seg in (a, b)} == {col for cols in case.ties for _, _, col in cols}
        assert plans[(name, 1, 0, 0, 0)]["n_seg"] >= 3, name  # ... and the planner cuts segments for the single copy by itself


def test_the_batch_sizes_change_the_plan(plans):
    """one, five and 300 copies: over the case list the planner picks every lane widening, chunk counts from one per job down to a
    real split, and column segments where the batch is small (a case of one short job stays widened even at 300 copies)"""
    seen = {reps: [plans[(name, reps, 0, 0, 0)] for name in T.NAMES if T.build(name).qlen <= 2048] for reps in T.REPS}
    assert {p["widening"] for p in seen[1]} == {4} and {p["widening"] for p in seen[300]} == {1, 2, 4}
    assert any(p["n_seg"] > 1 for p in seen[1]) and any(p["n_seg"] > 1 for p in seen[5])
    changed = [name for name in T.NAMES if len({(plans[(name, reps, 0, 0, 0)]["widening"], plans[(name, reps, 0, 0, 0)]["n_seg"]) for reps in T.REPS}) > 1]
    assert len(changed) >= len(T.NAMES) // 3, changed
