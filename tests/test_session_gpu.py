"""Alignment sessions on the GPU (sfa_session_*, sdtw_session.hpp): after EVERY extend a slot's row equals the oracle's row for the
slot's concatenated events so far, bit for bit (scores as uint32 views; no tolerance anywhere)."""
import numpy as np
import pytest

import sigfish_amd as S

pytestmark = pytest.mark.gpu


def _small_ref(rng, lens, rna, quant=True):
    def arr(n):
        return (rng.integers(-6, 7, n) / 4).astype(np.float32) if quant else rng.normal(size=n).astype(np.float32)
    fw = [arr(n) for n in lens]
    rv = None if rna else [arr(n) for n in lens]
    return S.RefModel([f"c{i}" for i in range(len(lens))], [n + 5 for n in lens], lens,
                      rng.integers(1, 4, len(lens)) if rna else [0] * len(lens), fw, rv)


def _oref(O, ref):
    return O.RefSynth(ref.names, ref.seq_lengths, ref.ref_lengths, ref.st_offset, ref.forward, ref.reverse)


def _events(rng, n, quant):
    return (rng.integers(-6, 7, n) / 4).astype(np.float32) if quant else rng.normal(size=n).astype(np.float32)


def assert_rows(got, want, starts=True, what=""):
    assert np.array_equal(got["valid"], want["valid"]), (what, got["valid"], want["valid"])
    v = want["valid"] == 1
    g, w = got[v], want[v]
    for f in ("rid", "strand", "mapq"):
        assert np.array_equal(g[f], w[f]), (what, f, g[f], w[f])
    for f in ("score", "score2"):
        assert np.array_equal(g[f].view(np.uint32), w[f].view(np.uint32)), (what, f, g[f], w[f])
    if starts:
        for f in ("pos_st", "pos_end"):
            assert np.array_equal(g[f], w[f]), (what, f, g[f], w[f])
    else:  # the coordinate that needs the start column is -1: pos_st on '+', pos_end on '-' (the flip)
        plus = w["strand"] == ord("+")
        assert np.array_equal(g["pos_end"][plus], w["pos_end"][plus]), what
        assert (g["pos_st"][plus] == -1).all(), what
        assert np.array_equal(g["pos_st"][~plus], w["pos_st"][~plus]), what
        assert (g["pos_end"][~plus] == -1).all(), what


class Oracle:
    """oracle.align_batch over prefixes, every distinct prefix once (shared by the runs with and without start columns)."""

    def __init__(self, O, ref, flag):
        self.O, self.oref, self.flag, self.memo = O, _oref(O, ref), flag, {}

    def rows(self, prefixes):
        out = np.zeros(len(prefixes), S.RESULT_DTYPE)
        for i, p in enumerate(prefixes):
            key = p.tobytes()
            if key not in self.memo:
                self.memo[key] = self.O.align_batch(p, np.array([0, len(p)], np.int64), self.oref, self.flag)[0].copy()
            out[i] = self.memo[key]
        return out


def run_schedule(sess, orc, sched, data, starts, order_rng):
    """sched[slot] = chunk length per call (None: the slot is not named in that call); data[slot] = its events.  After every call
    the rows of the named slots are compared with the oracle; -> {slot: events consumed}."""
    used = {sl: 0 for sl in sched}
    n_calls = max(len(v) for v in sched.values())
    for c in range(n_calls):
        named = [sl for sl, v in sched.items() if c < len(v) and v[c] is not None]
        order_rng.shuffle(named)
        chunks = [data[sl][used[sl]:used[sl] + sched[sl][c]] for sl in named]
        ev_off = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
        got = sess.extend(named, np.concatenate(chunks) if chunks else np.zeros(0, np.float32), ev_off)
        for sl in named:
            used[sl] += sched[sl][c]
        assert_rows(got, orc.rows([data[sl][:used[sl]] for sl in named]), starts, f"call {c}, slots {named}")
        assert list(sess.lengths(named)) == [used[sl] for sl in named]
    return used


REFS = {  # (flag, contig lengths)
    "dna_short_contig": (0, [900, 300, 57]),  # a contig shorter than the queries
    "dna_one": (0, [700]),
    "dna_many_jobs": (0, [160] * 12),
    "rna_inv_offsets": (S.RNA | S.INV, [1200, 400]),  # non-zero ref_st_offset
}
# slot ids unordered and sparse, different schedules in the same calls, only a subset of the slots named per call
SCHED = {
    11: [25] * 12,                                        # equal chunks
    0: [7, 1, 64, 3, 129, 250],                           # ragged chunks
    6: [256, 257],                                        # class edges
    2: [None, 16, 17, 1024, 1025],                        # class edges; joins late
    9: [0, 30, 0, None, None, 0, 40, 0],                  # zero-length chunks before, between and after real ones
    4: [50, None, None, None, None, None, None, None, None, 50],  # untouched for many calls: keeps its state
    13: [None, None, 2049, 100],                          # longer than one launch
    5: [129, 1, 1, 33],                                   # shares waves with slot 0's and 11's chunks by length modulo R
}
N_SLOTS = 14


@pytest.mark.parametrize("quant", [True, False], ids=["ties", "normal"])
@pytest.mark.parametrize("refname", list(REFS))
def test_rows_after_every_extend(oracle, refname, quant):
    flag, lens = REFS[refname]
    rng = np.random.default_rng(len(refname) * 7 + quant)
    ref = _small_ref(rng, lens, bool(flag & S.RNA), quant)
    data = {sl: _events(rng, sum(x or 0 for x in v), quant) for sl, v in SCHED.items()}
    orc = Oracle(oracle, ref, flag)
    with S.Aligner(ref, flag) as al:
        for starts in (True, False):
            with al.session(N_SLOTS, starts=starts) as se:
                run_schedule(se, orc, SCHED, data, starts, np.random.default_rng(3))
                full = se.lengths()
                assert full[1] == 0 and full[11] == 300 and full[13] == 2149
                # a slot that never received an event: valid = 0
                assert se.extend([1], np.zeros(0, np.float32), [0, 0])["valid"][0] == 0


@pytest.mark.parametrize("starts", [True, False])
def test_reset_poison_and_no_leaked_state(oracle, starts):
    rng = np.random.default_rng(21)
    ref = _small_ref(rng, [900, 300, 57], False)
    orc = Oracle(oracle, ref, 0)
    a, b, d = _events(rng, 180, True), _events(rng, 140, True), _events(rng, 90, True)
    with S.Aligner(ref, 0) as al, al.session(8, starts=starts) as se:
        run_schedule(se, orc, {3: [60, 70, 50], 6: [90]}, {3: a, 6: d}, starts, rng)
        # slot 3 reset and reused with other data, slot 6 untouched; a fresh slot (5) gets the same data: equal rows
        se.reset([3])
        assert list(se.lengths([3, 6])) == [0, 90]
        assert se.extend([3], np.zeros(0, np.float32), [0, 0])["valid"][0] == 0
        for lo, hi in ((0, 33), (33, 97), (97, 140)):
            got = se.extend([5, 3], np.concatenate([b[lo:hi], b[lo:hi]]), [0, hi - lo, 2 * (hi - lo)])
            assert got[0].tobytes() == got[1].tobytes()
            assert_rows(got, orc.rows([b[:hi], b[:hi]]), starts)
        assert_rows(se.extend([6], np.zeros(0, np.float32), [0, 0]), orc.rows([d]), starts)  # kept its row
        # an inf in chunk 2 poisons slot 3 from then on; the other slots of the same calls are unaffected
        se.reset([3, 5])
        bad = a.copy()
        bad[75] = np.inf
        for c, (lo, hi) in enumerate(((0, 50), (50, 100), (100, 150))):
            got = se.extend([3, 5, 6], np.concatenate([bad[lo:hi], a[lo:hi], a[lo:hi]]), [0, hi - lo, 2 * (hi - lo), 3 * (hi - lo)])
            assert got["valid"][0] == (1 if c == 0 else 0)
            if c == 0:
                assert_rows(got[:1], orc.rows([a[:hi]]), starts)
            assert al.profile()["non_finite_reads"] == (0 if c == 0 else 1)
            assert_rows(got[1:], orc.rows([a[:hi], np.concatenate([d, a[:hi]])]), starts)
        assert se.extend([3], np.zeros(0, np.float32), [0, 0])["valid"][0] == 0
        nan = b.copy()
        nan[0] = np.nan
        assert se.extend([7], nan[:40], [0, 40])["valid"][0] == 0  # (a first chunk)
        # clean again after reset; reset-all clears every slot
        se.reset([3])
        assert_rows(se.extend([3], b[:64], [0, 64]), orc.rows([b[:64]]), starts)
        se.reset()
        assert not se.lengths().any()
        got = se.extend([7, 6, 3], np.concatenate([b[:25], b[:25], b[:25]]), [0, 25, 50, 75])
        assert_rows(got, orc.rows([b[:25]] * 3), starts)


def test_interleaved_batch_call_and_two_sessions(oracle):
    rng = np.random.default_rng(33)
    ref = _small_ref(rng, [700, 300], False)
    orc = Oracle(oracle, ref, 0)
    x, y = _events(rng, 400, True), _events(rng, 400, False)
    qlens = [100, 250, 64, 300, 0, 600]
    q_off = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int64)
    q = _events(rng, int(q_off[-1]), True)
    with S.Aligner(ref, 0) as al:
        plain = al.align_db(q, q_off)
        with al.session(4) as s1, al.session(3, starts=False) as s2:
            assert_rows(s1.extend([2], x[:120], [0, 120]), orc.rows([x[:120]]))
            assert_rows(s2.extend([2, 0], np.concatenate([y[:70], x[:70]]), [0, 70, 140]), orc.rows([y[:70], x[:70]]), False)
            assert al.align_db(q, q_off).tobytes() == plain.tobytes()  # rows of a batch call as without a session
            assert_rows(s1.extend([2, 1], np.concatenate([x[120:300], y[:50]]), [0, 180, 230]), orc.rows([x[:300], y[:50]]))
            assert_rows(s2.extend([2], y[70:200], [0, 130]), orc.rows([y[:200]]), False)
            pr = al.profile()  # of the extend: new events x columns, one task per (wave of slots, contig, strand)
            assert pr["cells"] == 130 * ref.total_columns() and pr["n_tasks"] == 4 and pr["fill_ms"] > 0 and pr["total_ms"] >= pr["fill_ms"]
            assert_rows(s1.extend([2], x[300:], [0, 100]), orc.rows([x]))
            assert_rows(s2.extend([0], x[70:], [0, 330]), orc.rows([x]), False)


def test_session_outlives_nothing():
    """sfa_destroy frees the sessions a context still has: the Python objects are then closed."""
    rng = np.random.default_rng(5)
    ref = _small_ref(rng, [300], False)
    al = S.Aligner(ref, 0)
    se = al.session(2)
    se.extend([0], _events(rng, 30, True), [0, 30])
    al.close()
    with pytest.raises(S.SfaError):
        se.extend([0], _events(rng, 30, True), [0, 30])
    se.close()


def test_refusals():
    rng = np.random.default_rng(44)
    rna = _small_ref(rng, [400, 300], True)
    dna = _small_ref(rng, [400, 300], False)
    for ref, flag, kw in ((rna, S.RNA, {}), (rna, S.RNA | S.DTW, {}), (rna, S.RNA | S.DTW | S.INV, {}), (dna, 0, {"devices": [0, 0]})):
        with S.Aligner(ref, flag, **kw) as al:
            with pytest.raises(S.SfaError):
                al.session(4)
    ev = _events(rng, 60, True)
    with S.Aligner(dna, 0) as al:
        with pytest.raises(S.SfaError):
            al.session(0)
        with al.session(4) as se:
            for slots in ([4], [-1], [1, 1], [0, 2, 0]):
                off = np.arange(len(slots) + 1, dtype=np.int64) * 20
                with pytest.raises(S.SfaError):
                    se.extend(slots, ev, off)
            with pytest.raises(S.SfaError):
                se.reset([4])
            with pytest.raises(S.SfaError):
                se.lengths([9])
            assert not se.lengths().any()  # a refused call changes nothing
            assert se.extend([1], ev[:20], [0, 20])["valid"][0] == 1
