"""Recalibration of raw sessions on the GPU (sfa_session_raw_recalibrate, ev_stream_norm_kernel): after EVERY call
  * events, norm_mean / norm_sd, norm_window and the status bits (bit 4, the re-sweep, included) equal the host twin extended by
    the window rule (api.recal_window): mean and sd are a sequential np.float32 restatement over events [skip, skip + W);
  * the row equals Aligner.align_db of the twin's query: every available event normalised with that mean and sd;
  * state and rows depend on the samples a slot has received, not on how they were cut into calls, and the carried row equals
    oracle.last_row of the renormalised query.
The schedules are built from event counts (on the host detector, so without a GPU: tests/test_recal_cpu.py asserts the same
coverage) so that every case of CASES occurs.  No tolerance anywhere."""
import numpy as np
import pytest

import sigfish_amd as S
from tests.test_session_gpu import _small_ref, assert_rows
from tests.test_session_raw_gpu import META, SCALING, Rows, Twin, check_call, norm_stats, synth_signal

pytestmark = pytest.mark.gpu

SHAPE, AT = (3, 30, 70), (35, 50, 70)  # skip, norm, query; the recalibration points
N_SLOTS = 16
CASES = {"no_point", "exact_point", "two_points", "first_call_at_point", "point_and_full", "end_short", "end_tiny", "end_in_empty_chunk", "mixed_call", "after_recal"}


class RecalTwin(Twin):
    """Twin with the window rule: what a slot must hold when its normalisation grows with the read"""

    def __init__(self, rna, shape, at=(), at_end=False):
        self.at, self.at_end = tuple(at), at_end
        super().__init__(rna, shape)

    def reset(self):
        super().reset()
        self.window, self.swept, self.resweep, self.first, self.new_events, self.prev_window = 0, 0, False, False, 0, 0

    def q_avail(self):
        return max(0, min(len(self.ev) - self.skip, self.query))

    def feed(self, chunk, end):
        before = self.q_avail()
        super().feed(chunk, end)
        qa = self.q_avail()
        self.prev_window = self.window
        w = max(self.window, S.recal_window(qa, self.ended, self.norm, self.query, self.at, self.at_end))
        self.resweep = w != self.window and self.swept > 0
        self.first = w != self.window and self.swept == 0
        if w != self.window:
            self.window, self.stats = w, norm_stats(self.final()["mean"][self.skip:self.skip + w])
        self.new_events = qa - before
        self.swept = qa if self.window else 0

    def query_so_far(self):
        if not self.window:
            return None
        return ((self.final()["mean"][self.skip:] - self.stats[0]) / self.stats[1]).astype(np.float32)


def prefix_events(sig, rna=False):
    """E[n] = final events the streaming detector has emitted after n samples (whatever the chunking: tests/test_event_stream_cpu.py)"""
    out = np.zeros(len(sig) + 1, np.int64)
    with S.EventStream(META, rna) as es:
        for n in range(len(sig)):
            out[n + 1] = out[n] + len(es.push(sig[n:n + 1]))
    return out


def cut_at(E, q):
    """the first prefix with exactly q query events (skip + q final events)"""
    n = int(np.searchsorted(E, SHAPE[0] + q))
    assert n < len(E) and E[n] == SHAPE[0] + q, "the detector emitted two events at one sample: take another seed"
    return n


def build_plan(rng):
    """{slot: (signal, [per call: None (not named) | (samples, end of read)])} from query-event counts"""
    plan = {}

    def add(slot, n_samples, targets, lead=0, total_q=None):
        """targets: query events after each call | None | "end" (the rest, with the end of the read) | "empty_end"; total_q: cut the
        signal where the stream holds that many query events, so that the read ends a few events later"""
        sig = synth_signal(rng, n_samples)
        E = prefix_events(sig)
        if total_q is not None:
            sig = sig[:cut_at(E, total_q)]
        ops, at = [None] * lead, 0
        for t in targets:
            if t is None:
                ops.append(None)
            elif t == "end":
                ops.append((len(sig) - at, True))
                at = len(sig)
            elif t == "empty_end":
                ops.append((0, True))
            else:
                n = cut_at(E, t) if t < 10 ** 6 else len(sig)
                ops.append((n - at, False))
                at = n
        plan[slot] = (sig, ops)

    add(11, 1200, [20, 32, 34, 35, 44, 50, 60, 70, 10 ** 6, "empty_end"])       # lands on every point; 60 -> 70 is point and full at once
    add(0, 1200, [31, 55, 69, 10 ** 6])                                          # passes 35 and 50 in one call: 50 counts
    add(7, 1200, [None, None, None, 40, 52, "end"], total_q=58)                  # first call calibrates straight at 35; ends short of 70
    add(3, 600, [15, "end"], total_q=24)                                         # ends with 25 <= q < norm: calibrated only at the end
    add(9, 300, [5, "end"], total_q=10)                                          # ends with q < 25: never calibrated
    add(5, 1200, [40, 41, 45, 48, "empty_end", "empty_end"])                         # the end arrives alone: recalibrated without new samples
    add(14, 1200, [None, None, None, 33, 36, 49, 51, "end"], total_q=66)         # first chunk in the call where slot 11 lands on 35
    add(2, 1200, [10, 31, 32, 34, 41, 46, 10 ** 6])                              # carried chunks of other lengths beside them
    add(13, 1200, [70, None, None, 10 ** 6])                                     # full, and at the last point, in its first call
    return plan


def run_plan(plan, shape, at, at_end, on_call=None):
    """feeds the twins (and, through on_call(named, twins, c), a session) call by call; -> (twins, cases seen)"""
    twins = {sl: RecalTwin(False, shape, at, at_end) for sl in plan}
    pos = {sl: 0 for sl in plan}
    seen = set()
    for c in range(max(len(ops) for _, ops in plan.values())):
        named = []
        for sl, (sig, ops) in plan.items():
            if c < len(ops) and ops[c] is not None:
                named.append((sl, sig[pos[sl]:pos[sl] + ops[c][0]], ops[c][1]))
                pos[sl] += ops[c][0]
        before = {sl: (twins[sl].window, twins[sl].q_avail(), twins[sl].ended) for sl, _, _ in named}
        for sl, chunk, end in named:
            twins[sl].feed(chunk, end)
        if on_call:
            on_call(named, twins, c)
        carried_lens = set()
        for sl, chunk, end in named:
            t, (w0, q0, ended0) = twins[sl], before[sl]
            qa = t.q_avail()
            passed = [p for p in at if w0 < p <= qa]
            if w0 and t.window == w0 and t.new_events:
                seen.add("after_recal" if w0 > shape[1] else "no_point")
                carried_lens.add(t.new_events)
            if t.window != w0 and qa in at and t.window == qa and not t.ended:
                seen.add("exact_point")
            if t.window != w0 and len(passed) >= 2 and t.window == passed[-1]:
                seen.add("two_points")
            if w0 == 0 and q0 == 0 and t.window in at:
                seen.add("first_call_at_point")
            if t.window != w0 and t.window in at and qa == shape[2] and q0 < shape[2]:
                seen.add("point_and_full")
            if end and not ended0 and w0 == 0 and 25 <= qa < shape[1] and t.window == qa:
                seen.add("end_short")
            if end and not ended0 and qa < 25 and t.window == 0:
                seen.add("end_tiny")
            if end and not ended0 and len(chunk) == 0 and t.window != w0 and w0:
                seen.add("end_in_empty_chunk")
        if any(twins[sl].resweep for sl, _, _ in named) and any(twins[sl].first for sl, _, _ in named) and len(carried_lens) >= 2:
            seen.add("mixed_call")
    return twins, seen


def call_session(se, rows, starts, infos=None):
    def on_call(named, twins, c):
        slots = [x[0] for x in named]
        raw_off = np.concatenate([[0], np.cumsum([len(x[1]) for x in named])]).astype(np.int64)
        raw = np.concatenate([x[1] for x in named]) if named else np.zeros(0, np.int16)
        got, info = se.extend_raw(slots, raw, raw_off, [SCALING] * len(slots), [x[2] for x in named])
        check_call(se, twins, slots, got, info, rows, starts, f"call {c}")  # events, mean and sd, bits 0..3, rows, lengths
        for i, sl in enumerate(slots):
            t = twins[sl]
            assert info["norm_window"][i] == t.window, (c, sl, info["norm_window"][i], t.window)
            assert bool(info["status"][i] & S.RAW_RECALIBRATED) == t.resweep and not info["status"][i] & ~31, (c, sl, info["status"][i])
        if infos is not None:
            infos.append((slots, got.copy(), info.copy()))
    return on_call


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "nostart"])
def test_rule_after_every_call(starts):
    rng = np.random.default_rng(21)
    ref = _small_ref(rng, [400, 300], False, quant=False)
    plan = build_plan(np.random.default_rng(8))
    with S.Aligner(ref, 0) as al, al.session(N_SLOTS, starts=starts) as se:
        se.configure_raw(*SHAPE, recalibrate=AT, at_end=True)
        twins, seen = run_plan(plan, SHAPE, AT, True, call_session(se, Rows(al), starts))
        assert seen == CASES, CASES - seen  # (about this test's own inputs)
        assert twins[9].window == 0 and twins[3].window == twins[3].q_avail() and twins[11].window == 70


def test_resweep_in_pieces():
    """a query of 2100 events is swept again from event 0 when the slot reaches its one point: two pieces, 2048 + 52, over a
    contig shorter than a wave's columns"""
    shape, at = (3, 100, 2100), (2100,)
    rng = np.random.default_rng(33)
    ref = _small_ref(rng, [57], False, quant=False)
    sig = synth_signal(rng, 13000)
    twin = {0: RecalTwin(False, shape, at, False)}
    with S.Aligner(ref, 0) as al, al.session(2) as se:
        se.configure_raw(*shape, recalibrate=at)
        rows, windows, cells = Rows(al), [], []
        for c, (lo, hi) in enumerate(((0, 3000), (3000, 8000), (8000, 13000))):
            got, info = se.extend_raw([0], sig[lo:hi], [0, hi - lo], [SCALING], [False])
            pr = al.profile()
            twin[0].feed(sig[lo:hi], False)
            cells.append((pr["cells"], pr["fill_launches"]))
            check_call(se, twin, [0], got, info, rows, True, f"call {c}")
            assert info["norm_window"][0] == twin[0].window and bool(info["status"][0] & S.RAW_RECALIBRATED) == twin[0].resweep
            windows.append(int(info["norm_window"][0]))
        assert windows == [100, 100, 2100] and twin[0].resweep and info["status"][0] & S.RAW_FULL  # (about this test's own inputs)
        # cells counts what was swept: the last call swept all 2100 events again, in two launches
        assert cells[2] == (2100 * 2 * 57, 2), cells


CHUNKINGS = [[64], [1, 5, 6, 7, 11, 12, 13, 400], [10 ** 6]]


def test_chunk_independence(oracle):
    """the same samples under three chunkings: the same final rows, infos and carried rows, and the carried row is the oracle's
    last row of the renormalised query"""
    rng = np.random.default_rng(5)
    ref = _small_ref(rng, [400, 300], False, quant=False)
    short = synth_signal(rng, 520)
    sigs = {1: synth_signal(rng, 900), 4: short[:cut_at(prefix_events(short), 24)], 6: synth_signal(rng, 480), 9: synth_signal(rng, 300)}
    ends = {1: False, 4: True, 6: True, 9: False}
    finals = []
    with S.Aligner(ref, 0) as al:
        for sizes in CHUNKINGS:
            with al.session(N_SLOTS) as se:
                se.configure_raw(*SHAPE, recalibrate=AT, at_end=True)
                twins = {sl: RecalTwin(False, SHAPE, AT, True) for sl in sigs}
                last = {}
                at = {sl: 0 for sl in sigs}
                while any(at[sl] < len(sigs[sl]) for sl in sigs):
                    named = []
                    for i, sl in enumerate(sigs):
                        n = min(sizes[(at[sl] + i) % len(sizes)], len(sigs[sl]) - at[sl])
                        if n:
                            named.append((sl, sigs[sl][at[sl]:at[sl] + n], ends[sl] and at[sl] + n == len(sigs[sl])))
                            at[sl] += n
                    slots = [x[0] for x in named]
                    raw_off = np.concatenate([[0], np.cumsum([len(x[1]) for x in named])]).astype(np.int64)
                    got, info = se.extend_raw(slots, np.concatenate([x[1] for x in named]), raw_off, [SCALING] * len(slots), [x[2] for x in named])
                    for i, (sl, chunk, end) in enumerate(named):
                        twins[sl].feed(chunk, end)
                        one = info[i:i + 1].copy()
                        one["status"] &= 15  # (bit 4 belongs to a call, not to the slot)
                        last[sl] = (got[i].tobytes(), one.tobytes())
                carried = {}
                for sl, t in twins.items():
                    q = t.query_so_far()
                    assert q is not None and np.frombuffer(last[sl][1], S.SESSION_RAW_INFO_DTYPE)["norm_window"][0] == t.window
                    for contig in range(2):
                        for strand, arr in (("+", ref.forward), ("-", ref.reverse)):
                            cost, start = se.row(sl, contig, strand)
                            wc, ws = oracle.last_row(q, arr[contig], 0)
                            assert np.array_equal(cost.view(np.uint32), wc.view(np.uint32)) and np.array_equal(start, ws), (sizes, sl, contig, strand)
                            carried[(sl, contig, strand)] = cost.tobytes() + start.tobytes()
                finals.append((last, carried, {sl: t.window for sl, t in twins.items()}))
    assert finals[0] == finals[1] == finals[2]
    windows = set(finals[0][2].values())
    assert 70 in windows and windows - {30, 70} and finals[0][2][4] < 30  # (about this test's own inputs: a full slot, others between points, one calibrated at its end)


def test_refusals():
    rng = np.random.default_rng(44)
    ref = _small_ref(rng, [400, 300], False)
    a = synth_signal(rng, 400)
    with S.Aligner(ref, 0) as al, al.session(4) as se:
        with pytest.raises(S.SfaError):  # not in raw mode
            se.recalibrate((40,))
        se.configure_raw(3, 30, 70)
        for bad in ((40, 35), (40, 40), (30, 50), (29,), (50, 71), tuple(range(31, 64))):
            with pytest.raises(S.SfaError):
                se.recalibrate(bad)
        for flags in (2, 3, 0x80000000):
            with pytest.raises(S.SfaError):
                se.recalibrate((40,), flags=flags)
        se.recalibrate(tuple(range(31, 63)), True)  # 32 points
        se.recalibrate((70,))
        se.recalibrate(())  # off
        se.extend_raw([2], a[:100], [0, 100], [SCALING])
        with pytest.raises(S.SfaError):  # a slot in use
            se.recalibrate((40,))
        se.reset([2])
        se.recalibrate((40,), True)
        se.configure_raw(3, 45, 70)  # clears it: 40 would lie below this norm
        got, info = se.extend_raw([2], a, [0, 400], [SCALING], [True])
        assert info["norm_window"][0] in (0, 45) and not info["status"][0] & S.RAW_RECALIBRATED


def test_nothing_configured_changes_nothing():
    """one mixed schedule on a session on which sfa_session_raw_recalibrate was never called, on one where it was switched on and
    off again, and with norm_window following the frozen rule: the same bytes"""
    rng = np.random.default_rng(21)
    ref = _small_ref(rng, [400, 300], False, quant=False)
    plan = build_plan(np.random.default_rng(8))
    outs = []
    with S.Aligner(ref, 0) as al:
        rows = Rows(al)
        for touch in (False, True):
            with al.session(N_SLOTS) as se:
                se.configure_raw(*SHAPE)
                if touch:
                    se.recalibrate(AT, True)
                    se.recalibrate(())
                infos = []
                twins, _ = run_plan(plan, SHAPE, (), False, call_session(se, rows, True, infos))
                outs.append([(sl, r.tobytes(), i.tobytes()) for sl, r, i in infos])
                assert all(t.window in (0, SHAPE[1]) for t in twins.values())
                assert all(not (i["status"] & S.RAW_RECALIBRATED).any() and set(i["norm_window"]) <= {0, SHAPE[1]} for _, _, i in infos)
    assert outs[0] == outs[1]
