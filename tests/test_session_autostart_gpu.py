"""The automatic query start of raw sessions on the GPU (sfa_session_raw_auto_start: ev_auto_append_kernel, ev_auto_eval_kernel,
ev_stream_norm_kernel<true>).  70 slots -- a full wave of the one-slot-per-lane kernels and a partial one -- over the RNA
reference of the golden case rna_q500_pauto, query 100, norm 25, the doubling points and SFA_RECAL_AT_END, a point every 1600
samples, the largest skip 4000.  After EVERY call of four schedules
  * sfa_session_auto_start equals the host restatement of the rule (tests/autostart_oracle.py) field for field;
  * the events equal the host stream's, the counts and status bits follow from them and the slot's own skip;
  * the row equals Aligner.align_db of events [skip, skip + W) normalised over themselves, W the window rule's;
and the four schedules leave identical final state.  No tolerance anywhere."""
import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import synth
from tests.autostart_oracle import AutoTwin, cut
from tests.test_session_gpu import assert_rows
from tests.test_session_raw_gpu import Rows, same_events
from tests.util import load_case

pytestmark = pytest.mark.gpu

KINDS = ["normal", "adaptor_edge", "two_low", "polya_edge", "no_adaptor", "no_polya", "polya_at_end", "n2000", "n2001", "constant", "outside"]
N_SLOTS, EVERY, MAX_SKIP, NORM, QUERY = 70, 1600, 4000, 25, 100
AT = tuple(S.recal_double(NORM, QUERY))
SEED = 2  # chosen on the CPU so that the oracle alone meets the conditions of test_conditions_of_the_inputs
BIG = 1 << 20


def _reads():
    return synth.make_rna_polya_reads(N_SLOTS, seed=SEED, kinds=KINDS, body=(3000, 6000))


def _ref():
    c = load_case("rna_q500_pauto")
    return S.RefModel.from_fasta(c["fasta"], c["levels"], c["k"], S.RNA, QUERY)


def schedule(name, n):
    """the chunk lengths of a read of n samples"""
    if name == "chunks":
        return cut(n, [EVERY])
    if name == "whole":
        return [n]
    if name == "three_points":  # the third call carries the slot over 4800, 6400 and 8000
        head, left = [], n
        for c in (EVERY, EVERY, 3 * EVERY):
            if left > 0:
                head.append(min(c, left))
                left -= head[-1]
        return head + cut(left, [EVERY])
    assert name == "ones"       # one-sample chunks around every point: N_k - 1, N_k and N_k + 1 end a call each
    edges = sorted({e for k in range(1, n // EVERY + 2) for e in (k * EVERY - 1, k * EVERY, k * EVERY + 1) if 0 < e < n} | {n})
    return list(np.diff([0] + edges))


class SlotTwin(AutoTwin):
    """the rule's twin plus the window of the resweep session over the slot's own skip"""

    def reset(self):
        super().reset()
        self.window = 0

    def feed(self, chunk, end):
        super().feed(chunk, end)
        w = max(self.window, S.recal_window(self.q_avail(), self.ended, NORM, QUERY, AT, True))
        self.window = w

    def query_so_far(self):
        return S.znormalise(self.final()["mean"][self.skip:self.skip + self.window]) if self.window else None


def check_call(se, twins, slots, got, info, rows, what):
    au = se.auto_start(slots)
    want_q = []
    for i, sl in enumerate(slots):
        t = twins[sl]
        assert (int(au["target"][i]), int(au["frozen_at"][i]), int(au["skip"][i]), int(au["status"][i])) == t.state(), (what, sl, au[i], t.state())
        fin = t.final()
        same_events(se.events(sl), fin, (what, sl))
        assert info["n_samples"][i] == t.n and info["n_events"][i] == len(fin), (what, sl)
        st = int(info["status"][i])
        assert bool(st & S.RAW_CALIBRATED) == (t.window > 0) and bool(st & S.RAW_ENDED) == t.ended and not st & S.RAW_POISONED, (what, sl, st)
        assert bool(st & S.RAW_FULL) == (t.skip >= 0 and len(fin) >= t.skip + QUERY), (what, sl, st)
        assert info["norm_window"][i] == t.window and info["q_events"][i] == t.window, (what, sl, info[i], t.window)
        want_q.append(t.query_so_far())
    assert_rows(got, rows.rows(want_q), True, what)
    assert list(se.lengths(slots)) == [t.window for t in (twins[sl] for sl in slots)]
    a, b = se.query_span(slots)
    for i, sl in enumerate(slots):
        t = twins[sl]
        if t.window:
            ev = t.final()
            last = ev[t.skip + t.window - 1]
            assert (a[i], b[i]) == (ev["start"][t.skip], int(last["start"]) + int(last["length"])), (what, sl)
        else:
            assert (a[i], b[i]) == (0, 0), (what, sl)


def run(se, rows, reads, name, every, max_samples, check=True, max_skip=MAX_SKIP):
    """the reads, one per slot, under a schedule -> ({slot: final state}, twins)"""
    twins = {sl: SlotTwin(dict(digitisation=r[1], offset=r[2], range=r[3]), 0, every, max_samples, max_skip, QUERY) for sl, r in enumerate(reads)}
    plans = {sl: schedule(name, len(r[5])) for sl, r in enumerate(reads)}
    at = {sl: 0 for sl in plans}
    final = {}
    for c in range(max(len(p) for p in plans.values())):
        named = []
        for sl, p in plans.items():
            if c < len(p):
                named.append((sl, reads[sl][5][at[sl]:at[sl] + p[c]], c == len(p) - 1))
                at[sl] += p[c]
        slots = [x[0] for x in named]
        raw_off = np.concatenate([[0], np.cumsum([len(x[1]) for x in named])]).astype(np.int64)
        got, info = se.extend_raw(slots, np.concatenate([x[1] for x in named]), raw_off, [reads[sl][1:4] for sl in slots], [x[2] for x in named])
        for sl, chunk, end in named:
            twins[sl].feed(chunk, end)
        if check:
            check_call(se, twins, slots, got, info, rows, (name, c))
        au = se.auto_start(slots)
        for i, (sl, _, end) in enumerate(named):
            if end:
                one = info[i:i + 1].copy()
                one["status"] &= 15
                final[sl] = (au[i].tobytes(), got[i].tobytes(), one.tobytes())
    return final, twins


@pytest.fixture(scope="module")
def world():
    reads = _reads()
    with S.Aligner(_ref(), S.RNA) as al:
        yield dict(al=al, reads=reads, rows=Rows(al), finals={})


def _session(al, every, max_samples, norm=NORM, at=AT, max_skip=MAX_SKIP):
    return al.session(N_SLOTS, resweep=True, auto_start=dict(skip=max_skip, norm=norm, query=QUERY, recalibrate=at, at_end=True, every=every, max_samples=max_samples))


def _final_of(world, name):
    if name not in world["finals"]:
        with _session(world["al"], EVERY, BIG) as se:
            world["finals"][name] = run(se, world["rows"], world["reads"], name, EVERY, BIG)
    return world["finals"][name]


def test_conditions_of_the_inputs():
    """on the oracle alone, before any comparison: a pass cannot hide a path that never ran"""
    reads = _reads()
    mid = fallback = later = capped = 0
    for r in reads:
        meta = dict(digitisation=r[1], offset=r[2], range=r[3])
        t, t_cap, at = AutoTwin(meta, 0, EVERY, BIG, MAX_SKIP, QUERY), AutoTwin(meta, 0, EVERY, 8192, MAX_SKIP, QUERY), 0
        chunks = cut(len(r[5]), [EVERY])
        for i, c in enumerate(chunks):
            for tw in (t, t_cap):
                tw.feed(r[5][at:at + c], i == len(chunks) - 1)
            at += c
        mid += t.target >= 0 and not t.status & S.AUTO_AT_FINAL
        fallback += t.failed()
        later += t.target >= 0 and t.resolved_call > t.frozen_call
        capped += t_cap.frozen_at == 8192 and bool(t_cap.status & S.AUTO_AT_FINAL)
    assert mid >= N_SLOTS / 3 and fallback >= N_SLOTS / 10 and capped >= 3 and later >= 1, (mid, fallback, capped, later)


@pytest.mark.parametrize("name", ["chunks", "ones", "three_points", "whole"])
def test_every_call_of_a_schedule(world, name):
    final, twins = _final_of(world, name)
    assert len(final) == N_SLOTS
    if name == "three_points":  # (about this test's own inputs: one call passes two points and freezes at the third, or at the second)
        assert {t.frozen_at for t in twins.values() if t.frozen_call == 3} >= {4 * EVERY, 5 * EVERY}


def test_schedules_leave_identical_state(world):
    runs = [_final_of(world, name)[0] for name in ("chunks", "ones", "three_points", "whole")]
    for other in runs[1:]:
        for sl in range(N_SLOTS):
            assert runs[0][sl] == other[sl], sl


def test_reads_that_reach_the_cap(world):
    with _session(world["al"], EVERY, 8192) as se:
        final, twins = run(se, world["rows"], world["reads"], "chunks", EVERY, 8192)
    assert sum(t.frozen_at == 8192 and bool(t.status & S.AUTO_AT_FINAL) for t in twins.values()) >= 3


def cut_without_event(r):
    """the shortest prefix of read r whose target has no event at or behind it (the read ends there), or None"""
    meta = dict(digitisation=r[1], offset=r[2], range=r[3])
    whole = S.auto_start_target(r[5], meta, 0)
    if whole < 0:
        return None
    for n in range(whole + 1, min(whole + 600, len(r[5]))):
        t = S.auto_start_target(r[5][:n], meta, 0)
        if t >= 0:
            ev = S.detect_events(r[5][:n], meta, True)
            return r[:5] + (r[5][:n],) if not (ev["start"] >= t).any() else None
    return None


def _failure_inputs():
    """(reads cut so that they end with no event behind their target, the reads of the small-skip runs)"""
    reads = _reads()
    cuts = []
    for c in (cut_without_event(r) for r in reads):
        if c is not None:  # (a shorter prefix may freeze another target at a mid-read point: those reads are not what is wanted)
            t = AutoTwin(dict(digitisation=c[1], offset=c[2], range=c[3]), 0, EVERY, BIG, MAX_SKIP, QUERY)
            t.feed(c[5], True)
            if t.status & 15 == S.AUTO_NO_EVENT:
                cuts.append(c)
    return cuts, reads[:N_SLOTS]


def test_conditions_of_the_failure_inputs():
    """on the oracle alone: the two failures the big run never meets are met here, BEYOND_MAX in both of its forms"""
    cuts, reads = _failure_inputs()
    assert len(cuts) >= 2
    for r in cuts:
        t = AutoTwin(dict(digitisation=r[1], offset=r[2], range=r[3]), 0, EVERY, BIG, MAX_SKIP, QUERY)
        t.feed(r[5], True)
        assert t.status & 15 == S.AUTO_NO_EVENT and t.skip == 50 and t.target >= 0, t.state()
    full = part = 0
    for max_skip in (60, 400):
        for r in reads:
            t, at = AutoTwin(dict(digitisation=r[1], offset=r[2], range=r[3]), 0, EVERY, BIG, max_skip, QUERY), 0
            chunks = cut(len(r[5]), [EVERY])
            for i, c in enumerate(chunks):
                t.feed(r[5][at:at + c], i == len(chunks) - 1)
                at += c
            full += t.status & 15 == S.AUTO_BEYOND_MAX and t.table_full
            part += t.status & 15 == S.AUTO_BEYOND_MAX and not t.table_full
    assert full >= 3 and part >= 3, (full, part)


def test_read_that_ends_with_no_event_behind_its_target(world):
    cuts, _ = _failure_inputs()
    for name in ("chunks", "whole"):
        with _session(world["al"], EVERY, BIG) as se:
            final, twins = run(se, world["rows"], cuts, name, EVERY, BIG)
        assert all(t.status & 15 == S.AUTO_NO_EVENT for t in twins.values())


@pytest.mark.parametrize("max_skip", [60, 400])
def test_skip_beyond_the_largest(world, max_skip):
    """a small largest skip: the event behind the target lies beyond it, in the table (400) or behind a table that is full (60)"""
    _, reads = _failure_inputs()
    with _session(world["al"], EVERY, BIG, max_skip=max_skip) as se:
        final, twins = run(se, world["rows"], reads, "chunks", EVERY, BIG, max_skip=max_skip)
    assert sum(t.status & 15 == S.AUTO_BEYOND_MAX for t in twins.values()) >= 3


def test_whole_read_is_align_raw(world):
    """every_samples = 0, a cap above every read, norm = query and SFA_RECAL_AT_END: after the end of read the slot's skip, its
    fallback bit and its row are those of align_raw(prefix_size = -1)"""
    al, reads = world["al"], world["reads"]
    raw = np.concatenate([r[5] for r in reads])
    off = np.concatenate([[0], np.cumsum([len(r[5]) for r in reads])]).astype(np.int64)
    scal = np.array([r[1:4] for r in reads], np.float64)
    with _session(al, 0, BIG, norm=QUERY, at=()) as se:
        got, info = se.extend_raw(list(range(N_SLOTS)), raw, off, scal, [True] * N_SLOTS)
        au = se.auto_start(list(range(N_SLOTS)))
    want, winfo = al.align_raw(raw, off, scal, -1, QUERY)
    assert np.array_equal(got["valid"], want["valid"]) and 20 <= want["valid"].sum()
    v = want["valid"] == 1
    assert got[v].tobytes() == want[v].tobytes()
    assert np.array_equal(au["skip"][v], winfo["qstart"][v])
    failed = (au["status"] & 15) >= S.AUTO_NO_TARGET
    assert np.array_equal(failed[v], (winfo["status"][v] & 4) != 0) and failed[v].any() and not failed[v].all()
    assert (au["status"] & S.AUTO_AT_FINAL).all()


def test_reset_reuses_a_slot(world):
    reads, rows = world["reads"], world["rows"]
    with _session(world["al"], EVERY, BIG) as se:
        twins = {}
        for order in ((0, 1, 2), (2, 0, 1)):  # the second pass gives every slot another read
            for sl in range(3):
                r = reads[order[sl]]
                twins[sl] = SlotTwin(dict(digitisation=r[1], offset=r[2], range=r[3]), 0, EVERY, BIG, MAX_SKIP, QUERY)
                at, chunks = 0, cut(len(r[5]), [3 * EVERY + 7])
                for i, c in enumerate(chunks):
                    got, info = se.extend_raw([sl], r[5][at:at + c], [0, c], [r[1:4]], [i == len(chunks) - 1])
                    twins[sl].feed(r[5][at:at + c], i == len(chunks) - 1)
                    check_call(se, twins, [sl], got, info, rows, ("reset", order, sl, i))
                    at += c
            se.reset([0, 1, 2])
            au = se.auto_start([0, 1, 2])
            assert (au["target"] == -1).all() and (au["skip"] == -1).all() and (au["status"] == 0).all() and (au["frozen_at"] == 0).all()


def test_a_session_without_the_feature_is_untouched(world):
    """What this shows: a slot whose automatic start fell back to 50 ends with the row, window and normalisation of a slot of a
    plain resweep session with the fixed skip 50 fed the same samples (whole read in one call there, chunks here), and a plain
    session refuses auto_start().  That the plain session itself returns what it returned before this feature is what the
    existing session suites check (they run ev_stream_norm_kernel<false> and ev_query_span_kernel<false>), not this test."""
    al, reads = world["al"], world["reads"]
    final, twins = _final_of(world, "chunks")
    back = [sl for sl, t in twins.items() if t.failed()]
    assert len(back) >= N_SLOTS / 10
    with al.session(N_SLOTS, resweep=True) as se:
        se.configure_raw(50, NORM, QUERY, recalibrate=AT, at_end=True)
        with pytest.raises(S.SfaError, match="no automatic query start"):
            se.auto_start([0])
        plain = {}
        for sl in back:
            r = reads[sl]
            got, info = se.extend_raw([sl], r[5], [0, len(r[5])], [r[1:4]], [True])
            plain[sl] = (got[0].tobytes(), info[0])
    for sl in back:
        row, info = final[sl][1], np.frombuffer(final[sl][2], S.SESSION_RAW_INFO_DTYPE)[0]
        assert row == plain[sl][0], sl
        for f in ("n_samples", "q_events", "norm_mean", "norm_sd", "norm_window"):
            assert info[f].tobytes() == plain[sl][1][f].tobytes(), (sl, f)


def test_refusals(world):
    al = world["al"]
    with al.session(4, resweep=True) as se:
        with pytest.raises(S.SfaError, match="not in raw mode"):
            se.configure_auto_start(EVERY, 8192)
        se.configure_raw(49, NORM, QUERY)
        with pytest.raises(S.SfaError, match="must hold the fallback"):
            se.configure_auto_start(EVERY, 8192)
        se.configure_raw(50, NORM, QUERY)
        for every, cap in ((-1, 8192), (EVERY, -1), (EVERY, BIG + 1)):
            with pytest.raises(S.SfaError, match="need every_samples"):
                se.configure_auto_start(every, cap)
        se.configure_auto_start(EVERY, 8192)
        assert se.auto_start([3])["skip"][0] == -1
        se.configure_auto_start(EVERY, 0)  # off
        with pytest.raises(S.SfaError, match="no automatic query start"):
            se.auto_start([3])
        se.configure_auto_start(EVERY, 8192)
        se.configure_raw(50, NORM, QUERY)  # ... and so does configure_raw
        with pytest.raises(S.SfaError, match="no automatic query start"):
            se.auto_start([3])
        se.configure_auto_start(EVERY, 8192)
        r = world["reads"][0]
        se.extend_raw([1], r[5][:100], [0, 100], [r[1:4]])
        with pytest.raises(S.SfaError, match="not empty"):
            se.configure_auto_start(EVERY, 8192)
    ref = _ref()
    with S.Aligner(ref, S.RNA | S.INV) as inv, inv.session(4, resweep=True) as se:
        se.configure_raw(50, NORM, QUERY)
        with pytest.raises(S.SfaError, match="not compatible with auto query start detection"):
            se.configure_auto_start(EVERY, 8192)
