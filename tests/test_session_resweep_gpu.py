"""Resweep sessions on the GPU (SFA_SESSION_RESWEEP; ev_stream_norm_kernel's resweep / reversed arguments): a slot is swept only
when the window W of its normalisation changes, over events [skip, skip + W) -- reversed on an RNA context without INV.  After
EVERY call
  * every field of the row equals Aligner.align_db, on the same context, of the pA means of events [skip, skip + W) normalised
    over themselves with the library's znormalise and given in event order; W is api.recal_window of the host twin's counts;
  * info q_events, norm_window and lengths() are W, norm_mean / norm_sd equal the sequential fp32 restatement, the events equal
    the host twin's, query_span ends at event skip + W - 1, and status bit 4 is set exactly on the changes of W after the first;
  * state and rows depend on the samples a slot has received, not on how they were cut into calls.
No tolerance anywhere."""
import numpy as np
import pytest

import sigfish_amd as S
from tests.test_session_gpu import _small_ref
from tests.test_session_raw_gpu import SCALING, Rows, Twin, check_call, norm_stats, synth_signal
from tests.test_session_recal_gpu import prefix_events

pytestmark = pytest.mark.gpu

REFS = {"rna_offsets": (S.RNA, [1200, 400]), "rna_short_contigs": (S.RNA, [3, 63, 301]), "dna_one": (0, [700])}
SHAPE, POINTS = (10, 25, 200), (50, 100, 200)  # skip, norm, query; the recalibration points
CONFIGS = {"frozen": ((), False), "points": (POINTS, False), "points_at_end": (POINTS, True)}
N_SLOTS = 6
CASES = {"one_sample_change", "two_points", "waiting_events", "ended_between_points", "never_calibrated", "full", "after_reset"}


class SweepTwin(Twin):
    """what a slot of a resweep session must hold: the host detector fed the same chunks, the window rule, and the query of the
    window's events normalised over themselves"""

    def __init__(self, rna, shape, at=(), at_end=False):
        self.at, self.at_end = tuple(at), at_end
        super().__init__(rna, shape)

    def reset(self):
        super().reset()
        self.window, self.changed, self.resweep, self.grew = 0, False, False, False

    def q_avail(self):
        return max(0, min(len(self.ev) - self.skip, self.query))

    def feed(self, chunk, end):
        before = self.q_avail()
        super().feed(chunk, end)
        qa = self.q_avail()
        w = max(self.window, S.recal_window(qa, self.ended, self.norm, self.query, self.at, self.at_end))
        self.changed, self.resweep, self.grew = w != self.window, w != self.window and self.window > 0, qa > before
        if self.changed:
            self.window = w
            self.stats = norm_stats(self.final()["mean"][self.skip:self.skip + w])

    def query_so_far(self):
        """event order: align_db reverses it itself on an RNA context without INV"""
        if not self.window:
            return None
        return S.znormalise(self.final()["mean"][self.skip:self.skip + self.window])


def cut_at(E, q):
    """the first prefix with exactly q query events (skip + q final events)"""
    n = int(np.searchsorted(E, SHAPE[0] + q))
    assert n < len(E) and E[n] == SHAPE[0] + q, "the detector emitted two events at one sample: take another seed"
    return n


_PLANS = {}


def build_plan(rna):
    """{slot: [(signal, None (not named) | (samples, end of read) | "reset")]} from query-event counts of the host detector, once
    per detector"""
    if rna in _PLANS:
        return _PLANS[rna]
    rng = np.random.default_rng(70 + int(rna))
    plan = {}

    def add(slot, stops, lead=0, total_q=None):
        """stops: query events after each call | ("s", k): k more samples | ("before", q): one sample short of q query events |
        "end": the rest with the end of the read | "idle";
        total_q: the signal is cut where the stream holds that many query events"""
        sig = synth_signal(rng, 3000)
        E = prefix_events(sig, rna)
        if total_q is not None:
            sig = sig[:cut_at(E, total_q)]
        ops, at = [(sig, None)] * lead, 0
        for t in stops:
            if t == "idle":
                ops.append((sig, (0, False)))
                continue
            if isinstance(t, tuple):
                n = at + t[1] if t[0] == "s" else cut_at(E, t[1]) - 1
            else:
                n = len(sig) if t == "end" else cut_at(E, t)
            assert at <= n <= len(sig)
            ops.append((sig, (n - at, t == "end")))
            at = n
        plan.setdefault(slot, []).extend(ops)

    one = ("s", 1)
    # one-sample chunks around every point: the sample that closes event skip + point - 1 arrives alone, as do its neighbours
    add(0, [("before", 25), 25, one, ("before", 50), 50, one, ("before", 100), 100, one, ("before", 200), 200, one, "end"])
    add(1, [30, 120, 160, "end"], lead=1)                       # 30 -> 120 passes 50 and 100 in one call: 100 counts
    add(2, [40, 90, "end", "idle"], lead=2, total_q=130)        # ends between 100 and 200
    add(3, [5, "end", "idle"], lead=1, total_q=12)              # ends below skip + 25: never calibrated
    add(4, [("s", 700), ("s", 700), ("s", 700), ("s", 700), "end"])  # goes full; samples behind that are only counted
    add(5, [60, 110], lead=1)                                   # reset in the middle ...
    plan[5].append((None, "reset"))
    add(5, [26, 55, 101, "end"], total_q=140)                   # ... and another read
    _PLANS[rna] = plan
    return plan


def drive(se, plan, on_call, on_reset=None):
    """the calls of a plan on a session: on_call(c, [(slot, chunk, end)], rows, infos) after each"""
    at = {sl: 0 for sl in plan}
    for c in range(max(len(v) for v in plan.values())):
        named = []
        for sl, ops in plan.items():
            if c >= len(ops) or ops[c][1] is None:
                continue
            sig, op = ops[c]
            if op == "reset":
                se.reset([sl])
                at[sl] = 0
                assert se.lengths([sl])[0] == 0 and len(se.events(sl)) == 0 and tuple(x[0] for x in se.query_span([sl])) == (0, 0)
                if on_reset:
                    on_reset(sl)
                continue
            named.append((sl, sig[at[sl]:at[sl] + op[0]], op[1]))
            at[sl] += op[0]
        slots = [x[0] for x in named]
        raw_off = np.concatenate([[0], np.cumsum([len(x[1]) for x in named])]).astype(np.int64)
        raw = np.concatenate([x[1] for x in named]) if named else np.zeros(0, np.int16)
        got, info = se.extend_raw(slots, raw, raw_off, [SCALING] * len(slots), [x[2] for x in named])
        on_call(c, named, got, info)


def check_resweep_call(se, twins, named, got, info, rows, starts, what):
    """everything a call of a resweep session must leave behind (check_call: events, counts, bits 0..3, mean and sd, q_events and
    lengths() against the twin's query, every field of the rows against align_db)"""
    slots = [x[0] for x in named]
    check_call(se, twins, slots, got, info, rows, starts, what)
    a, b = se.query_span(slots)
    for i, sl in enumerate(slots):
        t = twins[sl]
        assert info["norm_window"][i] == t.window and info["q_events"][i] == t.window, (what, sl, info["norm_window"][i], info["q_events"][i], t.window)
        assert bool(info["status"][i] & S.RAW_RECALIBRATED) == t.resweep and not info["status"][i] & ~31, (what, sl, info["status"][i])
        if t.window:
            ev = t.final()
            last = ev[t.skip + t.window - 1]
            assert (a[i], b[i]) == (ev["start"][t.skip], int(last["start"]) + int(last["length"])), (what, sl)
        else:
            assert (a[i], b[i]) == (0, 0), (what, sl)


def with_twins(se, rna, at, at_end, rows, starts, seen, log=None):
    twins = {}

    def on_call(c, named, got, info):
        before = {sl: (twins[sl].window, twins[sl].ended) if sl in twins else (0, False) for sl, _, _ in named}
        for sl, chunk, end in named:
            twins.setdefault(sl, SweepTwin(rna, SHAPE, at, at_end)).feed(chunk, end)
        check_resweep_call(se, twins, named, got, info, rows, starts, f"call {c}")
        for i, (sl, chunk, end) in enumerate(named):
            t, (w0, ended0) = twins[sl], before[sl]
            qa = t.q_avail()
            if t.changed and len(chunk) == 1:
                seen.add("one_sample_change")
            if t.changed and len([p for p in at if w0 < p <= qa]) >= 2:
                seen.add("two_points")
            if not t.changed and t.window and t.grew and qa > t.window:
                seen.add("waiting_events")
            if end and not ended0 and t.window and any(p < qa for p in POINTS) and qa < SHAPE[2]:
                seen.add("ended_between_points")
            if end and not ended0 and t.window == 0:
                seen.add("never_calibrated")
            if info["status"][i] & S.RAW_FULL:
                seen.add("full")
            if log is not None:
                log.append((c, sl, t.changed, qa, t.window, got[i].tobytes(), info[i].tobytes()))

    def on_reset(sl):
        twins[sl].reset()
        seen.add("after_reset")

    return on_call, on_reset, twins


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("refname", list(REFS))
def test_rows_after_every_call(refname, config):
    flag, lens = REFS[refname]
    rna = bool(flag & S.RNA)
    at, at_end = CONFIGS[config]
    ref = _small_ref(np.random.default_rng(len(refname)), lens, rna, quant=False)
    assert not rna or all(ref.st_offset)  # (about this test's own inputs: non-zero ref_st_offset)
    plan = build_plan(rna)
    with S.Aligner(ref, flag) as al:
        rows = Rows(al)
        for starts in (True, False):
            with al.session(N_SLOTS, starts=starts, resweep=True) as se:
                se.configure_raw(*SHAPE, recalibrate=at, at_end=at_end)
                seen = set()
                on_call, on_reset, twins = with_twins(se, rna, at, at_end, rows, starts, seen)
                drive(se, plan, on_call, on_reset)
                want = CASES - ({"two_points"} if not at else set())
                assert seen >= want, want - seen  # (about this test's own inputs)
                assert twins[3].window == 0 and twins[4].window == (SHAPE[2] if at else SHAPE[1])
                assert twins[2].window == (twins[2].q_avail() if at_end else (100 if at else 25)) and 100 < twins[2].q_avail() < 200


CHUNKINGS = [[64], [1, 5, 58, 64, 128]]  # (the second cycle sums to 256: the two meet at 64, 128 and 256 of every 256 samples)


def test_chunking_independence():
    """the same samples under two schedules: equal rows and state wherever the two have sent a slot equally many samples"""
    flag, lens = REFS["rna_offsets"]
    rng = np.random.default_rng(6)
    ref = _small_ref(rng, lens, True, quant=False)
    full = synth_signal(rng, 2600)
    sigs = {0: full, 2: full[:1700], 3: synth_signal(rng, 900), 5: synth_signal(rng, 300)}
    ends = {0: False, 2: True, 3: True, 5: True}
    runs = []
    with S.Aligner(ref, flag) as al:
        for sizes in CHUNKINGS:
            with al.session(N_SLOTS, resweep=True) as se:
                se.configure_raw(*SHAPE, recalibrate=POINTS, at_end=True)
                at, calls, state = {sl: 0 for sl in sigs}, {sl: 0 for sl in sigs}, {}
                while any(at[sl] < len(sigs[sl]) for sl in sigs):
                    named = []
                    for sl in sigs:
                        n = min(sizes[calls[sl] % len(sizes)], len(sigs[sl]) - at[sl])
                        calls[sl] += 1
                        if n:
                            named.append((sl, sigs[sl][at[sl]:at[sl] + n], ends[sl] and at[sl] + n == len(sigs[sl])))
                            at[sl] += n
                    slots = [x[0] for x in named]
                    raw_off = np.concatenate([[0], np.cumsum([len(x[1]) for x in named])]).astype(np.int64)
                    got, info = se.extend_raw(slots, np.concatenate([x[1] for x in named]), raw_off, [SCALING] * len(slots), [x[2] for x in named])
                    a, b = se.query_span(slots)
                    for i, sl in enumerate(slots):
                        one = info[i:i + 1].copy()
                        one["status"] &= 15  # (bit 4 belongs to a call, not to the slot)
                        state[(sl, at[sl])] = (got[i].tobytes(), one.tobytes(), int(a[i]), int(b[i]), int(se.lengths([sl])[0]))
                runs.append(state)
    common = set(runs[0]) & set(runs[1])
    assert all((sl, len(sigs[sl])) in common for sl in sigs) and len(common) >= 20  # (about this test's own inputs)
    for key in sorted(common):
        assert runs[0][key] == runs[1][key], key
    windows = {sl: int(np.frombuffer(runs[0][(sl, len(sigs[sl]))][1], S.SESSION_RAW_INFO_DTYPE)["norm_window"][0]) for sl in sigs}
    assert windows[0] == 200 and 100 < windows[2] < 200 and 25 <= windows[3] < 100 and windows[5] in (0, 25), windows  # (inputs)


def test_window_beyond_one_launch(oracle):
    """query = 2100 with points ending at 2100 is the smallest window that crosses the 2048-event launch split: the reversed query
    is swept as pieces of 2048 + 52 events over the carried row of the first, on contigs shorter than a wave's columns"""
    flag, lens = REFS["rna_short_contigs"]
    shape, at = (10, 100, 2100), (1000, 2100)
    rng = np.random.default_rng(34)
    ref = _small_ref(rng, lens, True, quant=False)
    sig = synth_signal(rng, 24000)
    twins = {0: SweepTwin(True, shape, at, False)}
    with S.Aligner(ref, flag) as al, al.session(2, resweep=True) as se:
        se.configure_raw(*shape, recalibrate=at)
        rows, windows, launches = Rows(al), [], []
        for c, lo in enumerate(range(0, len(sig), 6000)):
            chunk = sig[lo:lo + 6000]
            got, info = se.extend_raw([0], chunk, [0, len(chunk)], [SCALING], [False])
            pr = al.profile()
            twins[0].feed(chunk, False)
            check_resweep_call(se, twins, [(0, chunk, False)], got, info, rows, True, f"call {c}")
            windows.append(int(info["norm_window"][0]))
            launches.append((pr["cells"], pr["fill_launches"]))
        assert windows[-1] == 2100 and 1000 in windows and info["status"][0] & S.RAW_FULL  # (about this test's own inputs)
        k = windows.index(2100)
        assert launches[k] == (2100 * sum(lens), 2) and launches[windows.index(1000)] == (1000 * sum(lens), 1), launches
        q = twins[0].query_so_far()
        assert len(q) == 2100
        for contig in range(len(lens)):
            cost, start = se.row(0, contig, "+")
            wc, ws = oracle.last_row(q, ref.forward[contig], flag)
            assert np.array_equal(cost.view(np.uint32), wc.view(np.uint32)) and np.array_equal(start, ws), contig


def test_forward_context_with_the_flag():
    """a forward query needs no resweep session, but may have one.  Both kinds follow the same window rule, so norm_window, mean
    and sd agree after every call; the rows agree at every call that changes W while the slot holds exactly W query events (the
    plain session's query is then the same W events; where a call brings more, the plain session has swept them too and the
    resweep session has them waiting, which is the difference between the two).  The one-sample chunks of slot 0 make that the
    case at every point, and at the end of a read W is all its events."""
    flag, lens = REFS["dna_one"]
    ref = _small_ref(np.random.default_rng(7), lens, False, quant=False)
    plan = build_plan(False)
    with S.Aligner(ref, flag) as al:
        log, plain = [], {}
        with al.session(N_SLOTS, resweep=True) as se:
            se.configure_raw(*SHAPE, recalibrate=POINTS, at_end=True)
            on_call, on_reset, _ = with_twins(se, False, POINTS, True, Rows(al), True, set(), log)
            drive(se, plan, on_call, on_reset)
        with al.session(N_SLOTS) as se:
            se.configure_raw(*SHAPE, recalibrate=POINTS, at_end=True)

            def on_call(c, named, got, info):
                for i, (sl, _, _) in enumerate(named):
                    plain[(c, sl)] = (got[i].tobytes(), info[i].tobytes())
            drive(se, plan, on_call)
    compared = set()
    for c, sl, changed, qa, window, row, info in log:
        a, b = (np.frombuffer(x, S.SESSION_RAW_INFO_DTYPE)[0] for x in (info, plain[(c, sl)][1]))
        for f in ("n_samples", "n_events", "norm_mean", "norm_sd", "norm_window"):
            assert a[f].tobytes() == b[f].tobytes(), (c, sl, f)
        if changed and qa == window:
            assert (row, info) == plain[(c, sl)], (c, sl, window)
            compared.add(window)
    assert compared >= {25, *POINTS} and compared - {25, *POINTS}, compared  # (inputs: every point, and a window at the end of a read)


def test_refusals():
    rng = np.random.default_rng(45)
    a = synth_signal(rng, 400)
    rna_ref = _small_ref(rng, [400, 300], True)
    with S.Aligner(rna_ref, S.RNA) as al:
        with pytest.raises(S.SfaError, match="reversed"):  # as before: an RNA context without INV and without the flag
            al.session(4)
        with pytest.raises(S.SfaError, match="reversed"):
            al.session(4, starts=False)
        for flags in (2, 6, 8, 12):  # 0x2 is not assigned; 0x8 does not exist
            with pytest.raises(S.SfaError):
                al.session(4, flags=flags)
        with al.session(4, resweep=True) as se:
            with pytest.raises(S.SfaError, match="swept again"):  # raw mode only, before ...
                se.extend([1], np.zeros(30, np.float32), [0, 30])
            with pytest.raises(S.SfaError):  # (not in raw mode yet)
                se.extend_raw([0], a, [0, 400], [SCALING])
            se.configure_raw(0, 25, 25)
            with pytest.raises(S.SfaError, match="swept again"):  # ... and after sfa_session_raw_config
                se.extend([1], np.zeros(30, np.float32), [0, 30])
            got, info = se.extend_raw([0], a, [0, 400], [SCALING])
            assert got["valid"][0] == 1 and info["q_events"][0] == 25
    with S.Aligner(rna_ref, S.RNA | S.DTW) as al:
        with pytest.raises(S.SfaError, match="SFA_DTW"):
            al.session(4, resweep=True)
    dna_ref = _small_ref(rng, [300], False)
    with S.Aligner(dna_ref, 0) as al:
        for flags in (2, 8):
            with pytest.raises(S.SfaError, match="unknown flag"):
                al.session(4, flags=flags)
        with al.session(4, flags=5) as se:  # SFA_SESSION_NO_START | SFA_SESSION_RESWEEP
            se.configure_raw(0, 25, 25)
            got, info = se.extend_raw([2], a, [0, 400], [SCALING])
            assert got["valid"][0] == 1 and info["q_events"][0] == 25 and list(se.lengths([2])) == [25]
            cost, start = se.row(2, 0, "+")  # (no start columns are carried)
            assert start is None and len(cost) == 300 and np.isfinite(cost).all()
