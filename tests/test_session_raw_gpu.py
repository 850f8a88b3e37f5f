"""Raw-signal sessions on the GPU (sfa_session_extend_raw, events_stream.hpp): samples go in chunk by chunk, and after EVERY call
  * the slot's device event table equals what the host twin (EventStream) fed the same chunks has emitted, bit for bit;
  * the frozen normalisation equals a sequential np.float32 restatement over events [skip, skip + norm), as uint32 views;
  * the row equals Aligner.align_db on the same context for the query ((mean_e - mean) / sd in np.float32) so far.
No tolerance anywhere."""
import numpy as np
import pytest

import sigfish_amd as S
from tests.test_session_gpu import _small_ref, assert_rows

pytestmark = pytest.mark.gpu

META = dict(digitisation=8192.0, offset=6.0, range=1467.61)
SCALING = (META["digitisation"], META["offset"], META["range"])
REFS = {"dna_short_contig": (0, [900, 300, 57]), "dna_one": (0, [700]), "rna_inv_offsets": (S.RNA | S.INV, [1200, 400])}
SHAPES = [(3, 25, 70), (0, 25, 25)]  # skip, norm, query
N_SLOTS = 40


def synth_signal(rng, n):
    """piecewise-constant levels ~N(90, 12) pA, dwell 6..12 samples, noise sd 1.5, as ADC counts"""
    n_lv = n // 6 + 2
    pa = np.repeat(rng.normal(90, 12, n_lv), rng.integers(6, 13, n_lv))[:n] + rng.normal(0, 1.5, n)
    return np.round(pa * META["digitisation"] / META["range"] - META["offset"]).astype(np.int16)


def norm_stats(m):
    """sfa_znormalise's mean and sd: two sequential fp32 loops, sqrt in double"""
    cnt = np.float32(len(m))
    mean = np.float32(0)
    for v in m:
        mean = np.float32(mean + v)
    mean = np.float32(mean / cnt)
    var = np.float32(0)
    for v in m:
        d = np.float32(v - mean)
        var = np.float32(var + np.float32(d * d))
    var = np.float32(var / cnt)
    return mean, np.float32(np.sqrt(np.float64(var)))


def same_events(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    assert np.array_equal(got["start"], want["start"]), what
    for f in ("length", "mean", "stdv"):
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), (what, f)


class Twin:
    """what a slot must hold: the host detector fed the same chunks, the normalisation restated"""

    def __init__(self, rna, shape):
        self.rna, (self.skip, self.norm, self.query) = rna, shape
        self.reset()

    def reset(self):
        self.es = S.EventStream(META, self.rna)
        self.ev = np.zeros(0, S.EVENT_DTYPE)
        self.n, self.ended, self.stats = 0, False, None

    def feed(self, chunk, end):
        if not self.ended:  # (an ended slot is only named with empty chunks)
            self.ev = np.concatenate([self.ev, self.es.push(chunk)] + ([self.es.finish()] if end else []))
        self.n += len(chunk)
        self.ended = self.ended or end

    def final(self):
        return self.ev[:self.skip + self.query]

    def query_so_far(self):
        ev = self.final()
        if len(ev) < self.skip + self.norm:
            return None
        if self.stats is None:
            self.stats = norm_stats(ev["mean"][self.skip:self.skip + self.norm])
        return ((ev["mean"][self.skip:] - self.stats[0]) / self.stats[1]).astype(np.float32)


class Rows:
    """Aligner.align_db per distinct query, once (shared by the runs with and without start columns)"""

    def __init__(self, al):
        self.al, self.memo = al, {}

    def rows(self, queries):
        new = {q.tobytes(): q for q in queries if q is not None and q.tobytes() not in self.memo}
        if new:
            qs = list(new.values())
            got = self.al.align_db(np.concatenate(qs), np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.int64))
            for k, r in zip(new, got):
                self.memo[k] = r.copy()
        out = np.zeros(len(queries), S.RESULT_DTYPE)
        for i, q in enumerate(queries):
            if q is not None:
                out[i] = self.memo[q.tobytes()]
        return out


def check_call(se, twins, named, got, info, rows, starts, what):
    want_q = []
    for i, sl in enumerate(named):
        t = twins[sl]
        fin = t.final()
        same_events(se.events(sl), fin, (what, sl))
        assert info["n_samples"][i] == t.n and info["n_events"][i] == len(fin), (what, sl)
        q = t.query_so_far()
        st = int(info["status"][i])
        assert bool(st & S.RAW_CALIBRATED) == (q is not None) and bool(st & S.RAW_ENDED) == t.ended, (what, sl, st)
        assert bool(st & S.RAW_FULL) == (len(fin) == t.skip + t.query) and not st & S.RAW_POISONED, (what, sl, st)
        if q is None:
            assert got["valid"][i] == 0 and info["q_events"][i] == 0 and info["norm_sd"][i] == 0, (what, sl)
        else:
            assert info["norm_mean"][i:i + 1].view(np.uint32)[0] == t.stats[0].view(np.uint32), (what, sl)
            assert info["norm_sd"][i:i + 1].view(np.uint32)[0] == t.stats[1].view(np.uint32), (what, sl)
            assert info["q_events"][i] == len(q), (what, sl)
        want_q.append(q)
    assert_rows(got, rows.rows(want_q), starts, what)
    assert list(se.lengths(named)) == [0 if q is None else len(q) for q in want_q]


def cut(n, sizes):
    out, at, i = [], 0, 0
    while at < n:
        c = min(sizes[i % len(sizes)], n - at)
        out.append(c)
        at += c
        i += 1
    return out


def build_plan(rng):
    """{slot: [(signal, per call: None (not named) | (samples, end of read) | "reset")]}: every kind of schedule in the same calls"""
    sig = lambda n: synth_signal(rng, n)  # noqa: E731
    plan = {}

    def add(slot, signal, ops):
        plan.setdefault(slot, []).extend((signal, op) for op in ops)

    def with_end(chunks):  # the end of the read comes with the last samples
        return [(c, False) for c in chunks[:-1]] + [(chunks[-1], True)]

    a = sig(1500)
    add(11, a, with_end(cut(len(a), [64])))                                             # equal chunks of 64
    a = sig(1100)
    add(0, a, [(c, False) for c in cut(len(a), [1, 5, 6, 7, 11, 12, 13, 400])] + [(0, True), (0, False), (0, True)])  # ragged; ends in an empty call
    a = sig(900)
    add(2, a, [None, None, None] + with_end(cut(len(a), [100])))                        # joins late
    a = sig(800)
    add(9, a, [(0, False), (130, False), (0, False), None, None, (0, False), (140, False), (0, False), (530, False)])  # empty chunks
    a = sig(2500)
    add(4, a, [(300, False)] + [None] * 12 + [(300, False), (1900, True)])              # untouched for many calls
    a = sig(90)
    add(13, a, [(40, False), (50, True), (0, False)])                                   # ends before it calibrates
    a, b = sig(1000), sig(1300)
    add(5, a, [(200, False)] * 4)                                                       # reset midway, then another read
    add(5, b, ["reset"] + with_end(cut(len(b), [260])))
    a = sig(2400)
    add(21, a, [(len(a), True)])                                                        # the whole read at once
    a = sig(600)
    add(30, a, [(c, False) for c in cut(len(a), [37])])                                 # never ends
    a = sig(1700)
    add(17, a, with_end(cut(len(a), [256, 512])))
    a = sig(700)
    add(39, a, [None] * 5 + with_end(cut(len(a), [11, 12, 13])))                        # the cuts around 2 w_long of both detectors
    a = sig(1200)
    add(8, a, with_end(cut(len(a), [27, 1, 1, 300])))
    a = sig(650)
    add(26, a, [(1, False)] * 40 + [(610, True)])                                       # sample by sample over 2 w_long
    a = sig(2000)
    add(33, a, [None, (1000, False), None, (1000, False), (0, True)])
    return plan


def run_plan(se, al_rows, plan, rna, shape, starts, order_rng):
    twins = {sl: Twin(rna, shape) for sl in plan}
    at = {sl: 0 for sl in plan}
    n_calls = max(len(v) for v in plan.values())
    calibrated = full = 0
    for c in range(n_calls):
        named, chunks, ends = [], [], []
        for sl, ops in plan.items():
            if c >= len(ops) or ops[c][1] is None:
                continue
            signal, op = ops[c]
            if op == "reset":
                se.reset([sl])
                twins[sl].reset()
                at[sl] = 0
                assert se.lengths([sl])[0] == 0 and len(se.events(sl)) == 0
                continue
            named.append((sl, signal[at[sl]:at[sl] + op[0]], op[1]))
            at[sl] += op[0]
        order_rng.shuffle(named)
        slots = [x[0] for x in named]
        raw_off = np.concatenate([[0], np.cumsum([len(x[1]) for x in named])]).astype(np.int64)
        raw = np.concatenate([x[1] for x in named]) if named else np.zeros(0, np.int16)
        got, info = se.extend_raw(slots, raw, raw_off, [SCALING] * len(slots), [x[2] for x in named])
        if c == 0:  # the profile of THIS call (check_call's align_db would replace it): a whole read of 2400 samples is walked here
            pr = al_rows.al.profile()
            assert pr["events_ms"] > 0 and pr["normalise_ms"] > 0 and pr["fill_ms"] > 0, pr
            assert pr["total_ms"] >= pr["fill_ms"] + pr["events_ms"], pr
        for sl, chunk, end in named:
            twins[sl].feed(chunk, end)
        check_call(se, twins, slots, got, info, al_rows, starts, f"call {c}")
    for t in twins.values():
        calibrated += t.query_so_far() is not None
        full += len(t.final()) == t.skip + t.query
    return twins, calibrated, full


@pytest.mark.parametrize("shape", SHAPES, ids=["skip3_norm25_q70", "skip0_norm25_q25"])
@pytest.mark.parametrize("refname", list(REFS))
def test_events_normalisation_and_rows_after_every_call(refname, shape):
    flag, lens = REFS[refname]
    rna = bool(flag & S.RNA)
    rng = np.random.default_rng(len(refname) + shape[0])
    ref = _small_ref(rng, lens, rna, quant=False)
    plan = build_plan(rng)
    with S.Aligner(ref, flag) as al:
        rows = Rows(al)
        for starts in (True, False):
            with al.session(N_SLOTS, starts=starts) as se:
                se.configure_raw(*shape)
                twins, calibrated, full = run_plan(se, rows, plan, rna, shape, starts, np.random.default_rng(3))
                assert calibrated >= len(plan) - 3 and full >= len(plan) // 2, (calibrated, full)  # the schedules reach every state
                assert twins[13].query_so_far() is None  # ended before it calibrated
                # a slot that was never named: no samples, no events, no row
                got, info = se.extend_raw([1], np.zeros(0, np.int16), [0, 0], [SCALING])
                assert got["valid"][0] == 0 and info["n_samples"][0] == 0 and info["status"][0] == 0 and len(se.events(1)) == 0


def test_zero_variance_calibration_poisons_the_slot():
    """a sawtooth whose events all have the same mean, an integer with unit scaling, so that the fp32 sums are exact (checked below
    on the host detector): sd = 0, no query can be made of it"""
    unit = dict(digitisation=8192.0, offset=0.0, range=8192.0)
    rng = np.random.default_rng(9)
    ref = _small_ref(rng, [400, 300], True, quant=False)
    saw = np.tile(500 + 8 * np.arange(10), 60).astype(np.int16)
    ok = synth_signal(rng, 1500)
    ev = S.detect_events(saw, unit, True)
    assert len(ev) > 40 and (ev["mean"][1:27] == 536).all() and norm_stats(ev["mean"][1:26])[1] == 0
    with S.Aligner(ref, S.RNA | S.INV) as al, al.session(4) as se:
        se.configure_raw(1, 25, 40)
        for c, (lo, hi) in enumerate(((0, 200), (200, 400), (400, 600))):
            got, info = se.extend_raw([2, 0], np.concatenate([saw[lo:hi], ok[lo:hi]]), [0, hi - lo, 2 * (hi - lo)], [(8192.0, 0.0, 8192.0), SCALING])
            poisoned = info["n_events"][0] >= 26
            assert bool(info["status"][0] & S.RAW_POISONED) == poisoned and got["valid"][0] == 0 and info["q_events"][0] == 0
            assert not info["status"][1] & S.RAW_POISONED
            assert al.profile()["non_finite_reads"] == int(poisoned)
        assert poisoned and info["norm_sd"][0] == 0 and got["valid"][1] == 1
        same_events(se.events(2), ev[:info["n_events"][0]], "the events of a poisoned slot stay")
        # clean again after the reset: the other signal calibrates and is swept
        se.reset([2])
        got, info = se.extend_raw([2], ok[:600], [0, 600], [SCALING])
        got0, info0 = se.extend_raw([0], np.zeros(0, np.int16), [0, 0], [SCALING])
        assert info["status"][0] & S.RAW_CALIBRATED and not info["status"][0] & S.RAW_POISONED and got["valid"][0] == 1
        assert got.tobytes() == got0.tobytes() and info.tobytes() == info0.tobytes()  # slot 0 had the same samples


def test_refusals():
    rng = np.random.default_rng(44)
    ref = _small_ref(rng, [400, 300], False)
    a = synth_signal(rng, 400)
    with S.Aligner(ref, 0) as al, al.session(4) as se:
        with pytest.raises(S.SfaError):  # not in raw mode yet
            se.extend_raw([0], a, [0, 400], [SCALING])
        for bad in ((-1, 25, 25), (0, 24, 30), (0, 30, 29)):
            with pytest.raises(S.SfaError):
                se.configure_raw(*bad)
        se.extend([1], np.zeros(30, np.float32), [0, 30])
        with pytest.raises(S.SfaError):  # a slot holds events
            se.configure_raw(0, 25, 25)
        se.reset()
        se.configure_raw(0, 25, 25)
        with pytest.raises(S.SfaError):  # extend on a raw session
            se.extend([1], np.zeros(30, np.float32), [0, 30])
        se.extend_raw([0, 3], np.concatenate([a[:100], a[:100]]), [0, 100, 200], [SCALING] * 2, [False, True])
        with pytest.raises(S.SfaError):  # changed scaling
            se.extend_raw([0], a[100:200], [0, 100], [(8192.0, 7.0, 1467.61)])
        with pytest.raises(S.SfaError):  # samples after the end of the read
            se.extend_raw([3], a[100:200], [0, 100], [SCALING])
        for slots in ([4], [-1], [1, 1]):
            with pytest.raises(S.SfaError):
                se.extend_raw(slots, a[:20 * len(slots)], np.arange(len(slots) + 1) * 20, [SCALING] * len(slots))
        with pytest.raises(S.SfaError):  # a slot in use
            se.configure_raw(0, 25, 30)
        # the refused calls changed nothing: slot 0 goes on where it was
        got, info = se.extend_raw([0, 3], a[100:400], [0, 300, 300], [SCALING] * 2)
        assert list(info["n_samples"]) == [400, 100] and info["status"][1] & S.RAW_ENDED
        with S.EventStream(META) as es:
            same_events(se.events(0), es.push(a)[:25], "slot 0")
        se.reset([3])  # a reset slot takes another scaling
        se.extend_raw([3], a[:50], [0, 50], [(8192.0, 7.0, 1467.61)])


def test_many_slots_one_call():
    """300 slots in one call: several waves of slots, ragged chunk lengths inside every wave, a second call on the carried state"""
    rng = np.random.default_rng(17)
    ref = _small_ref(rng, [300], False)
    n = 300
    sigs = [synth_signal(rng, 512) for _ in range(n)]
    first = [256 if i % 3 else int(rng.integers(0, 257)) for i in range(n)]
    slots = rng.permutation(n + 20)[:n]
    with S.Aligner(ref, 0) as al, al.session(n + 20) as se:
        se.configure_raw(0, 25, 30)
        twins = [S.EventStream(META) for _ in range(n)]
        want = [np.zeros(0, S.EVENT_DTYPE)] * n
        for lo, hi, end in (([0] * n, first, False), (first, [f + 256 for f in first], True)):
            chunks = [s[a:b] for s, a, b in zip(sigs, lo, hi)]
            raw_off = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
            got, info = se.extend_raw(slots, np.concatenate(chunks), raw_off, [SCALING] * n, [end] * n)
            for i in range(n):
                want[i] = np.concatenate([want[i], twins[i].push(chunks[i])] + ([twins[i].finish()] if end else []))
                same_events(se.events(int(slots[i])), want[i][:30], i)
            assert np.array_equal(info["n_events"], [min(len(w), 30) for w in want])
        assert (info["status"] & S.RAW_CALIBRATED).all() and got["valid"].all()


def test_destroy_with_an_open_raw_session():
    rng = np.random.default_rng(5)
    ref = _small_ref(rng, [300], False)
    al = S.Aligner(ref, 0)
    se = al.session(2)
    se.configure_raw(0, 25, 25)
    se.extend_raw([0], synth_signal(rng, 300), [0, 300], [SCALING])
    al.close()
    with pytest.raises(S.SfaError):
        se.extend_raw([0], synth_signal(rng, 30), [0, 30], [SCALING])
    se.close()
