"""The wave matrix of the session tests, without a GPU: the restated grouping rule (tests/session_waves.py) says which (class
shape, first chunk or carried row, occupancy, g0) combinations build_matrix reaches -- all of them -- and which the hand-written
schedule of test_session_gpu.py reaches -- few; and the oracle's last row with its per-column tracebacks (oracle.last_row, what
a carried row must hold) reproduces oracle.align_batch's rows through the window scan."""
import os

import numpy as np
import pytest

from oracle import oracle as OM
from tests import session_waves as W
from tests.test_session_gpu import SCHED

DNA_LENS = [1, 2, 3, 5, 62, 63, 64, 301, 1030]
RNA_LENS = [3, 63, 301, 1030]


def test_restatement_basics():
    assert [W.class_for(n) for n in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048)] == [5, 5, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0]
    # the launch split at 2048 events: a chunk of 4097 is three launches, 2048 + 2048 + 1, and only its first piece is a first chunk
    la = W.plan_call([(0, 4097)], {})
    assert [[(p.len, p.total, p.first) for g in gs for p in g.pieces] for gs in la] == [[(2048, 2048, 1)], [(2048, 4096, 0)], [(1, 4097, 0)]]
    assert W.counts(la, 18) == (54, 3)
    assert len(W.plan_call([(0, 2048)], {3: 5})) == 1 and len(W.plan_call([(0, 2049), (1, 0)], {})) == 2
    # waves: same kind, class and residue; sorted by length, 64 / lanes per wave; the first is the longest
    gs = W.plan_call([(0, 9), (1, 61), (2, 5), (3, 1), (4, 60), (5, 13), (6, 300)], {6: 10})[0]
    assert [[p.len for p in g.pieces] for g in gs] == [[60], [61, 13, 9, 5], [1], [300]]
    assert gs[1].g0 == [0, 12, 13, 14] and (gs[1].lq, gs[1].rq) == (15, 0) and gs[3].first == 0


@pytest.mark.parametrize("kind", ["first", "carried"])
def test_matrix_reaches_every_wave_shape(kind):
    m = W.build_matrix(kind)
    first = 1 if kind == "first" else 0
    assert 40 <= len(m.slots) <= 50 and len(set(m.slots)) == len(m.slots) and max(m.slots) >= 100
    assert m.slots != sorted(m.slots) and not {W.ZERO_SLOT, W.UNNAMED_SLOT} & set(m.slots)
    if kind == "carried":
        assert len(set(m.prefix)) == len(m.prefix) and min(m.prefix) == 3 and max(m.prefix) > 1030
    else:
        assert not any(m.prefix)
    launches = W.plan_call(list(zip(m.slots, m.lens)), dict(zip(m.slots, m.prefix)))
    assert len(launches) == 1 and W.classes_per_launch(launches) == [6]
    cov = W.coverage(launches)
    print(f"\ncoverage of build_matrix({kind!r}):")
    for shape in W.SHAPES:
        print(f"  {shape} {kind}: {cov[(shape, first)]}")
    assert set(cov) == {(sh, first) for sh in W.SHAPES}
    assert W.shortfalls(cov, kinds=(first,)) == []
    for shape in W.SHAPES:  # (spelt out once more: the table of the coverage the GPU test relies on)
        c, cap = cov[(shape, first)], 64 // shape[1]
        assert c["groups"] >= 2 and c["full"] >= 1 and c["max_g0_full"] >= cap - 1
        assert cap == 1 or c["partial"] >= 1
    # the g0 == lq == 15, rq == 0 wave: 61 & 1
    w = [g for g in launches[0] if [p.len for p in g.pieces] == [61, 1]]
    assert len(w) == 1 and (w[0].g0, w[0].lq, w[0].rq) == ([0, 15], 15, 0)
    # longest & shortest of a residue share a wave in every shape that has waves to share
    got = {g.shape: tuple(p.len for p in g.pieces) for g in launches[0] if tuple(p.len for p in g.pieces) in W.PAIRS.values()}
    assert got == W.PAIRS
    # rq == R - 1 (length % R == 0) and rq == 0 (length % R == 1) both occur in partly filled waves
    part = [g for g in launches[0] if g.occupancy < g.capacity]
    assert any(g.rq == g.R - 1 for g in part) and any(g.rq == 0 for g in part)
    # the window lengths (totals) of the slots of one wave all differ, and they straddle the contig lengths
    for g in launches[0]:
        tot = [p.total for p in g.pieces]
        assert len(set(tot)) == len(tot), tot
    tot = [p.total for g in launches[0] for p in g.pieces]
    for n in (5, 62, 64, 301, 1030):
        assert min(tot) < n < max(tot)
    # a last block with idle waves: tasks of the 18-job DNA reference are no multiple of 4
    n_tasks, n_launches = W.counts(launches, 2 * len(DNA_LENS))
    assert n_tasks % 4 != 0 and n_launches == 1
    # the continuation moves every slot into another class
    cont = W.continuation_lengths(m)
    assert all(W.class_for(a) != W.class_for(b) for a, b in zip(cont, m.lens))
    held = {s: p + n for s, p, n in zip(m.slots, m.prefix, m.lens)}
    cc = W.coverage(W.plan_call(list(zip(m.slots, cont)), held))
    assert {sh for sh, f in cc} == set(W.SHAPES) and all(f == 0 for sh, f in cc)


def test_split_schedule_spans_launches():
    la = W.plan_call(W.SPLIT, {})
    assert len(la) == 3 and W.counts(la, 18)[1] == 3
    assert sorted(p.len for g in la[0] for p in g.pieces) == [64, 300, 2048, 2048]
    assert sorted(p.len for g in la[1] for p in g.pieces) == [1, 2048] and all(g.first == 0 for g in la[1])
    assert [p.len for g in la[2] for p in g.pieces] == [1]


def _sched_launches(sched):
    used = {s: 0 for s in sched}
    out = []
    for c in range(max(len(v) for v in sched.values())):
        named = [s for s, v in sched.items() if c < len(v) and v[c] is not None]
        out += W.plan_call([(s, sched[s][c]) for s in named], used)
        for s in named:
            used[s] += sched[s][c]
    return out


def test_old_schedule_falls_short():
    """A recorded contrast: what test_session_gpu.SCHED reaches of the same table.  If this test fails because SCHED grew, move
    the entry that is now reached out of the list; the matrix above does not depend on it."""
    launches = _sched_launches(SCHED)
    cov = W.coverage(launches)
    miss = W.shortfalls(cov)
    print("\nshortfall of test_session_gpu.SCHED:")
    for m in miss:
        print("  ", m)
    for shape in ((8, 16), (32, 16), (32, 32)):  # first chunks of three shapes: those session_body instantiations never run
        assert (shape, 1, "never run") in miss
    # the shortest chunk starting in the owner's lane: never with first chunks; below a carried row only 25 & 1 of (4, 16), lq 6
    assert (None, 1, "no wave with g0 == lq") in miss
    assert [sh for (sh, f), c in cov.items() if c["g0_eq_lq"]] == [(4, 16)]
    # first chunks never share a wave; below a carried row only (4, 16) does, and never with four slots
    assert all(c["max_occupancy"] == 1 for (sh, f), c in cov.items() if f == 1)
    assert [sh for (sh, f), c in cov.items() if f == 0 and c["max_occupancy"] > 1] == [(4, 16)]
    assert all(c["full"] == 0 for (sh, f), c in cov.items() if sh[1] < 64)
    assert max(W.classes_per_launch(launches)) < 6
    assert len(miss) >= 15


# ---- the oracle's last row against what is already trusted ----
def _arr(rng, n, quant):
    return (rng.integers(-6, 7, n) / 4).astype(np.float32) if quant else rng.normal(size=n).astype(np.float32)


def _scan_row(O, q, ref, flag):
    """The window scan of src/sigfish.c:891-901 over oracle.last_rows, jobs merged in processing order (a later candidate wins
    ties, sigfish.c:577-583), then sigfish.c:969-983 -> one RESULT_DTYPE row."""
    n = len(q)
    cand = []  # (score, contig, strand, end column, start column) in the order the reference offers them
    for contig, strand, cost, start in O.last_rows(q, ref, flag):
        for w in range(0, len(cost), n):
            win = cost[w:w + n]
            at = w + int(np.argmin(win))  # first strict minimum
            cand.append((win.min(), contig, strand, at, int(start[at])))
    scores = np.array([c[0] for c in cand], np.float32)
    best = len(scores) - 1 - int(np.argmin(scores[::-1]))  # the last of the equal minima
    second = np.sort(scores)[1] if len(scores) > 1 else np.float32(np.inf)
    score, contig, strand, end, st = cand[best]
    rl, off = int(ref.ref_lengths[contig]), int(ref.st_offset[contig])
    row = np.zeros(1, O.RESULT_DTYPE)
    row["rid"], row["strand"], row["valid"] = contig, ord(strand), 1
    row["pos_st"] = (st if strand == "+" else rl - end) + off
    row["pos_end"] = (end if strand == "+" else rl - st) + off
    row["score"], row["score2"] = score, second
    row["mapq"] = O.mapq(score, second)
    return row


def test_last_row_reproduces_align_batch(oracle):
    O = oracle
    rng = np.random.default_rng(77)
    have_ref = os.path.exists(OM.REF_SO)
    for i in range(30):
        rna, quant = bool(i & 1), bool(i & 2)
        flag = (O.RNA | O.INV) if rna else 0
        pool = RNA_LENS if rna else DNA_LENS
        lens = [int(x) for x in rng.choice(pool, size=int(rng.integers(1, 5)), replace=False)]
        fw = [_arr(rng, n, quant) for n in lens]
        rv = None if rna else [_arr(rng, n, quant) for n in lens]
        ref = O.RefSynth([f"c{k}" for k in range(len(lens))], [n + 5 for n in lens], lens,
                         rng.integers(1, 4, len(lens)) if rna else [0] * len(lens), fw, rv)
        q = _arr(rng, int(rng.integers(1, 601)) if i else 1, quant)
        want = O.align_batch(q, np.array([0, len(q)], np.int64), ref, flag)
        got = _scan_row(O, q, ref, flag)
        assert got.tobytes() == want.tobytes(), (i, lens, len(q), got, want)
        if have_ref:  # the query rows under INV are the events as they are (sigfish.c:861-866)
            for contig, strand, cost, start in O.last_rows(q, ref, flag):
                y = fw[contig] if strand == "+" else rv[contig]
                assert cost.tobytes() == O.ref_subsequence(q, y)[-1].tobytes(), (i, contig, strand)
