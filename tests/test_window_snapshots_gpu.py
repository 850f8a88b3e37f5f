"""The LDS-checkpoint fill takes every read's snapshots where the read's OWN windows end (sdtw_kernels.hpp, LdsCkpt) and saves,
for a window that becomes the read's best, the one taken a window before it began: pass 2 starts one own window -- less the lane
skew -- in front of its window, the first two windows of a strand from scratch, and a path that began earlier backs off to the
sparse HBM store, which the fill now writes at cuts of the wave as well.  Every case compares every row field bit for bit with
the oracle, on the smallest shapes that reach those paths, with pass 2 as its own launch and inside the fill launch."""
import numpy as np
import pytest

import sigfish_amd as S

pytestmark = pytest.mark.gpu

LDS = {"lane_widening": 1, "lds_ckpt": 2}  # the 16-lane shapes on the LDS route whatever the batch size


def _ref(rng, lens, rna):
    fw = [rng.normal(size=n).astype(np.float32) for n in lens]
    rv = None if rna else [rng.normal(size=n).astype(np.float32) for n in lens]
    return S.RefModel([f"c{i}" for i in range(len(lens))], [n + 5 for n in lens], lens, [0] * len(lens), fw, rv)


def _oracle_ref(O, ref):
    return O.RefSynth(ref.names, ref.seq_lengths, ref.ref_lengths, ref.st_offset, ref.forward, ref.reverse)


def _planted(rng, levels, starts, qlens, stride=1, reverse=False, noise=0.05):
    """Queries that follow `levels` from starts[i], one event per `stride` columns: the best path is (nearly) that line."""
    rows = []
    for s, n in zip(starts, qlens):
        row = levels[s + stride * np.arange(n)] + rng.normal(0, noise, size=n).astype(np.float32)
        rows.append(row[::-1] if reverse else row)
    q_off = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int64)
    return np.concatenate(rows).astype(np.float32), q_off


def _assert_bitwise(got, want, what):
    for f in ("rid", "strand", "pos_st", "pos_end", "mapq", "valid"):
        assert np.array_equal(got[f], want[f]), (what, f, np.flatnonzero(got[f] != want[f])[:10])
    for f in ("score", "score2"):
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), (what, f)


def _run(ref, flag, q, q_off, want, extra=None):
    """Rows of the LDS route with pass 2 as its own launch and by ticket inside the fill launch; the last profile."""
    prof = None
    for fused in (0, 2):
        with S.Aligner(ref, flag) as al:
            for k, v in {**LDS, "fused_trace": fused, **(extra or {})}.items():
                al.set_option(k, v)
            got = al.align_db(q, q_off)
            prof = al.profile()
        assert prof["lds_ckpt"] == (2 if fused else 1), prof
        _assert_bitwise(got, want, f"fused_trace={fused}")
    return prof


def test_winners_in_the_first_three_windows_and_the_last_partial_one(oracle):
    """2 400 levels per strand at q = 250: windows 0 .. 8 and a last one of 150 columns.  Reads planted so that their winning cell
    falls into windows 0, 1, 2, 5 and 9; those of windows 0 and 1 have no snapshot and are reported as started from scratch.  The
    read planted at column 251 ends in the first column of window 2: its path begins before the snapshot of that window (row 0
    at column 2 * 250 - 250 + 15), so it leaves the saved record."""
    rng = np.random.default_rng(101)
    q, n = 250, 2400
    ref = _ref(rng, [n], False)
    starts = [0, 0, 1, 120, 250, 251, 300, 500, 1100, 1251, 2001, 2100, 2150, 2150]
    qs, q_off = _planted(rng, ref.forward[0], starts, [q] * len(starts))
    want = oracle.align_batch(qs, q_off, _oracle_ref(oracle, ref), 0, threads=8)
    assert (want["strand"] == ord("+")).all() and np.array_equal(want["pos_end"], np.array(starts) + q - 1)
    window = want["pos_end"] // q
    assert {0, 1, 2, 5, n // q} <= set(window.tolist())
    prof = _run(ref, 0, qs, q_off, want)
    assert prof["n_chunks"] == 2  # two chunks per quad: one per strand
    assert prof["lck_from_scratch"] == int((window < 2).sum())
    assert prof["lck_fallbacks"] >= 1
    assert prof["trace_margin"] == q - (q - 1) // 16


def test_reference_lengths_around_multiples_of_the_window(oracle):
    """Strands of k*q, k*q - 1, k*q + 1 columns, one shorter than two windows and one shorter than the query."""
    rng = np.random.default_rng(102)
    q = 250
    lens = [1000, 999, 1001, 499, 300, 120]
    ref = _ref(rng, lens, False)
    rows, off = [], [0]
    for c, n in enumerate(lens):
        if n < q:
            continue
        for s in (0, (n - q) // 2, n - q):  # first, middle and the very last columns of the strand
            for arr in (ref.forward[c], ref.reverse[c]):
                rows.append(arr[s:s + q] + rng.normal(0, 0.05, q).astype(np.float32))
                off.append(off[-1] + q)
    qs, q_off = np.concatenate(rows).astype(np.float32), np.array(off, np.int64)
    want = oracle.align_batch(qs, q_off, _oracle_ref(oracle, ref), 0, threads=8)
    assert len(set(want["rid"].tolist())) == 5
    _run(ref, 0, qs, q_off, want)


@pytest.mark.parametrize("qmax,R", [(250, 16), (120, 8), (60, 4)])
def test_mixed_quads_and_ragged_batches(oracle, qmax, R):
    """Reads whose lengths agree modulo the rows per lane share a wave: every slot has its own window length, cut points and
    buffer parity.  Then a ragged batch whose lengths leave partly filled waves.  R = 16, 8 and 4 (q = 250, 120, 60)."""
    rng = np.random.default_rng(103 + R)
    n = 10 * qmax + qmax // 3  # >= 8 windows of the longest read and a partial one
    ref = _ref(rng, [n], False)
    mixed = [qmax - R * j for j in range(4)] * 3  # 250 / 234 / 218 / 202 at R = 16
    ragged = [int(x) for x in rng.integers(qmax // 2 + 1, qmax + 1, size=27)]
    qlens = mixed + ragged
    starts = [int(rng.integers(0, n - l + 1)) for l in qlens]
    starts[:4] = [0, 3 * qmax, n - qlens[2], 2 * qlens[3]]
    qs, q_off = _planted(rng, ref.forward[0], starts, qlens)
    want = oracle.align_batch(qs, q_off, _oracle_ref(oracle, ref), 0, threads=8)
    assert np.abs(want["pos_end"] - (np.array(starts) + np.array(qlens) - 1)).max() <= 2  # the winners are the planted positions
    _run(ref, 0, qs, q_off, want)


def test_rna_reversed_queries(oracle):
    """RNA: one strand, query rows are the events reversed."""
    rng = np.random.default_rng(104)
    q, n = 250, 2600
    ref = _ref(rng, [n], True)
    qlens = [250, 250, 250, 250, 234, 218, 202, 250, 170]
    starts = [0, 130, 251, 520, 777, 1500, 2398, 2350, 2430]
    qs, q_off = _planted(rng, ref.forward[0], starts, qlens, reverse=True)
    want = oracle.align_batch(qs, q_off, _oracle_ref(oracle, ref), S.RNA, threads=8)
    assert np.abs(want["pos_end"] - (np.array(starts) + np.array(qlens) - 1)).max() <= 2  # the winners are the planted positions
    _run(ref, S.RNA, qs, q_off, want)


def test_paths_longer_than_the_head_start_back_off_to_the_sparse_store(oracle):
    """64 reads on a strand whose levels each last two or three columns, one event per level: the alignments span 500 .. 750
    columns, far more than the one window of head start, so pass 2 finds the path beginning before the saved snapshot and goes on
    to the sparse HBM store (one record per 32 768 steps on this 70 000-column strand, written at cuts of the wave) or the start
    of the strand.  The plain scheme (every snapshot in HBM) must give the same rows."""
    rng = np.random.default_rng(105)
    q, n = 250, 70000
    base = rng.normal(size=n // 2).astype(np.float32)
    fw = np.repeat(base, rng.integers(2, 4, size=len(base)))[:n]
    col0 = np.concatenate([[0], np.cumsum(np.diff(fw) != 0)])  # level index of every column
    ref = S.RefModel(["c0"], [n + 5], [n], [0], [fw], None)
    first = [int(x) for x in np.linspace(0, col0[n - 1] - q - 1, 64)]  # first level of every read
    first[1], first[2] = int(col0[32768 + 300]), int(col0[65536 + 200])  # winners right behind a record of the sparse store
    rows = [base[b:b + q][::-1] + rng.normal(0, 0.05, q).astype(np.float32) for b in first]
    qs = np.concatenate(rows).astype(np.float32)
    q_off = (np.arange(65) * q).astype(np.int64)
    want = oracle.align_batch(qs, q_off, _oracle_ref(oracle, ref), S.RNA, threads=8)
    assert ((want["pos_end"] - want["pos_st"]) > 2 * q - 20).sum() >= 60
    assert (want["pos_end"] > 33000).sum() >= 24
    prof = _run(ref, S.RNA, qs, q_off, want)
    assert prof["lck_fallbacks"] > 0
    with S.Aligner(ref, S.RNA) as al:
        for k, v in (("lane_widening", 1), ("lds_ckpt", 0)):
            al.set_option(k, v)
        plain = al.align_db(qs, q_off)
        assert al.profile()["lds_ckpt"] == 0 and al.profile()["lck_fallbacks"] == 0
    _assert_bitwise(plain, want, "lds_ckpt=0")
