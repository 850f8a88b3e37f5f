"""Spread sessions on the GPU (SFA_SESSION_SPREAD, session_spread.hpp, the prologues in sfa_session.hip, sfa_session_targets.hip and sfa_session_state.hpp): a session whose slots are
dealt over the shards of a group context.  The yardstick is always a PLAIN session on a single-device context fed the same calls:
after every call every output of the spread session -- rows, lengths, statuses, candidates, spans, automatic-start records,
row(), events(), maps -- is the plain session's, byte for byte; one leg compares with the oracle's rows as well, so the test is
not only self-consistency.  Device lists: [0, 0] and [0, 0, 0] (a device listed twice is two shards) and, where the box has
several GPUs, all of them.  7 slots: the shards hold 4 + 3 and 3 + 2 + 2.  No tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime, synth
from tests.realtime_util import BIN, write_model
from tests.test_session_gpu import Oracle, _events, _small_ref, assert_rows
from tests.test_session_maps_gpu import row_bytes
from tests.test_session_raw_gpu import SCALING, synth_signal
from tests.util import distinct_device_list, load_case

pytestmark = pytest.mark.gpu

N_SLOTS = 7
DEVICE_LISTS = [[0, 0], [0, 0, 0]]
IDS = ["two_shards", "three_shards"]


def device_lists():
    every = distinct_device_list()
    return DEVICE_LISTS + ([every] if every else [])


class Both:
    """a plain session on a single-device aligner and a spread session on a group aligner: every call goes to both, and what
    comes back must be the same bytes (what the plain one raises, the spread one must raise)"""

    def __init__(self, plain, spread):
        self.plain, self.spread = plain, spread

    def __getattr__(self, name):
        def call(*a, **kw):
            try:
                want = getattr(self.plain, name)(*a, **kw)
            except S.SfaError:
                with pytest.raises(S.SfaError):
                    getattr(self.spread, name)(*a, **kw)
                raise
            got = getattr(self.spread, name)(*a, **kw)
            same(got, want, (name, a[:1]))
            return want
        return call


def same(got, want, what):
    if isinstance(want, tuple):
        assert len(got) == len(want), what
        for g, w in zip(got, want):
            same(g, w, what)
    elif isinstance(want, np.ndarray):
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (what, got, want)
    else:
        assert got == want, (what, got, want)


def offsets(chunks):
    return np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)


def cat(chunks, dtype):
    return np.concatenate(chunks).astype(dtype) if chunks else np.zeros(0, dtype)


class Pair:
    """the two aligners and a factory of session pairs"""

    def __init__(self, ref, flag, devices):
        self.one, self.many = S.Aligner(ref, flag), S.Aligner(ref, flag, devices=devices)
        assert self.many.n_devices() == len(devices)

    def session(self, n_slots, **kw):
        return Both(self.one.session(n_slots, **kw), self.many.session(n_slots, spread=True, **kw))

    def close(self):
        self.one.close()
        self.many.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- event mode ----
@pytest.mark.parametrize("devices", DEVICE_LISTS, ids=IDS)
@pytest.mark.parametrize("starts", [True, False], ids=["starts", "no_start"])
def test_event_mode(oracle, devices, starts):
    rng = np.random.default_rng(101)
    ref = _small_ref(rng, [400, 300], False)
    orc = Oracle(oracle, ref, 0)
    data = {sl: _events(rng, 200, True) for sl in range(N_SLOTS)}
    used = {sl: 0 for sl in range(N_SLOTS)}
    G = len(devices)

    def extend(se, slots, lens):
        chunks = [data[sl][used[sl]:used[sl] + n] for sl, n in zip(slots, lens)]
        got = se.extend(slots, cat(chunks, np.float32), offsets(chunks))
        for sl, n in zip(slots, lens):
            used[sl] += n
        return got

    with Pair(ref, 0, devices) as pair:
        se = pair.session(N_SLOTS, starts=starts)
        got = extend(se, [6, 5, 4, 3, 2, 1, 0], [60, 1, 17, 0, 33, 59, 8])  # all shards, descending slots, an empty chunk
        assert_rows(got, orc.rows([data[sl][:used[sl]] for sl in (6, 5, 4, 3, 2, 1, 0)]), starts, "against the oracle")
        pr_one, pr_many = pair.one.profile(), pair.many.profile()  # the profile after a call: summed counts, the slowest shard's times
        assert pr_many["cells"] == pr_one["cells"] == 178 * ref.total_columns() and pr_many["fill_ms"] > 0
        assert pr_many["non_finite_reads"] == pr_one["non_finite_reads"] == 0
        one_shard = [sl for sl in range(N_SLOTS) if sl % G == G - 1]  # one shard only (the last), then one slot, then no slot
        extend(se, one_shard, [23] * len(one_shard))
        assert pair.many.profile()["cells"] == pair.one.profile()["cells"] == 23 * len(one_shard) * ref.total_columns()  # (idle shards add nothing)
        extend(se, [3], [41])
        extend(se, [], [])
        se.lengths()
        se.lengths([5, 0, 5])
        for sl in range(N_SLOTS):  # the carried rows, read back from the owning shard
            if used[sl]:
                for strand in "+-":
                    se.row(sl, 1, strand)
        # a NaN poisons one slot on one shard; the other slots of the call, on that shard and the others, stay valid
        bad = data[4][used[4]:used[4] + 30].copy()
        bad[7] = np.nan
        chunks = [data[0][used[0]:used[0] + 30], bad, data[2][used[2]:used[2] + 30]]
        got = se.extend([0, 4, 2], cat(chunks, np.float32), offsets(chunks))
        used[0] += 30
        used[2] += 30
        assert list(got["valid"]) == [1, 0, 1]
        assert_rows(got[[0, 2]], orc.rows([data[0][:used[0]], data[2][:used[2]]]), starts, "beside a poisoned slot")
        assert pair.many.profile()["non_finite_reads"] == pair.one.profile()["non_finite_reads"] == 1
        assert extend(se, [4], [0])["valid"][0] == 0
        # reset of some slots, then of all
        se.reset([4, 1])
        used[4] = used[1] = 0
        assert list(se.lengths([4, 1, 0])) == [0, 0, used[0]]
        got = extend(se, [1, 4], [50, 50])
        assert_rows(got, orc.rows([data[1][:50], data[4][:50]]), starts, "after a reset")
        se.reset()
        assert not se.lengths().any()
        used.update({sl: 0 for sl in used})
        assert_rows(extend(se, [2, 3], [20, 20]), orc.rows([data[2][:20], data[3][:20]]), starts, "after a reset of every slot")
        se.close()


def test_one_slot_on_three_shards(oracle):
    """n_slots = 1 on [0, 0, 0]: two shards hold no sub-session"""
    rng = np.random.default_rng(102)
    ref = _small_ref(rng, [400, 300], False)
    ev = _events(rng, 90, True)
    with Pair(ref, 0, [0, 0, 0]) as pair:
        se = pair.session(1)
        se.extend([0], ev[:40], [0, 40])
        got = se.extend([0], ev[40:], [0, 50])
        assert_rows(got, Oracle(oracle, ref, 0).rows([ev]))
        assert pair.many.profile()["cells"] == 50 * ref.total_columns()
        assert list(se.lengths()) == [90]
        se.row(0, 0, "-")
        with pytest.raises(S.SfaError, match="out of range"):
            se.extend([1], ev[:10], [0, 10])
        se.reset([0])
        se.extend([0], ev[:25], [0, 25])
        se.reset()
        assert list(se.lengths()) == [0]
        se.configure_candidates(2)  # (configuration skips the shards without a sub-session)
        se.extend([0], ev[:25], [0, 25])
        se.candidates([0])
        se.close()
        se = pair.session(2)  # and a second session, created and destroyed with the aligner
        se.extend([1, 0], ev[:60], [0, 30, 60])


# ---- raw mode ----
def feed_raw(se, sigs, at, sizes, slots=None):
    """the next sizes[i] samples of every named slot that has samples left, in one call"""
    named = [sl for sl in (range(len(sigs)) if slots is None else slots) if at[sl] < len(sigs[sl])]
    chunks, ends = [], []
    for sl in named:
        n = min(sizes[sl % len(sizes)], len(sigs[sl]) - at[sl])
        chunks.append(sigs[sl][at[sl]:at[sl] + n])
        at[sl] += n
        ends.append(at[sl] == len(sigs[sl]))
    rows, info = se.extend_raw(named, cat(chunks, np.int16), offsets(chunks), [SCALING] * len(named), ends)
    return named, rows, info


@pytest.mark.parametrize("devices", device_lists(), ids=lambda d: f"{len(d)}_shards_on_{len(set(d))}")
def test_raw_mode(devices):
    """frozen normalisation, then recalibrate with a list and SFA_RECAL_AT_END; query_span; events() of a slot on the last shard"""
    rng = np.random.default_rng(103)
    ref = _small_ref(rng, [400, 300], False)
    sigs = [synth_signal(rng, int(rng.integers(600, 1500))) for _ in range(N_SLOTS)]
    G = len(devices)
    last = max(sl for sl in range(N_SLOTS) if sl % G == G - 1)
    with Pair(ref, 0, devices) as pair:
        se = pair.session(N_SLOTS)
        for recal in ((), (50, 70)):
            se.configure_raw(3, 25, 70, recal, bool(recal))
            at = [0] * N_SLOTS
            calibrated = resweeps = 0
            for call in range(8):
                named, rows, info = feed_raw(se, sigs, at, [300, 170, 450], None if call % 3 else [sl for sl in range(N_SLOTS) if sl != call % N_SLOTS])
                if not named:
                    break
                calibrated += int((info["status"] & S.RAW_CALIBRATED).astype(bool).sum())
                resweeps += int((info["status"] & S.RAW_RECALIBRATED).astype(bool).sum())
                se.query_span(named[::-1])
                se.lengths()
                se.events(last)
                if rows["valid"].any():
                    sl = named[int(np.flatnonzero(rows["valid"])[0])]
                    se.row(sl, 0, "+")
            assert calibrated > N_SLOTS and (resweeps > 0) == bool(recal)  # (about this test's own inputs)
            assert pair.many.profile()["events_ms"] > 0
            with pytest.raises(S.SfaError, match="end of read"):  # refused on its shard's account, for the whole call: no shard moves
                before = se.lengths().copy()
                ended = [sl for sl in range(N_SLOTS) if at[sl] == len(sigs[sl])][0]
                other = (ended + 1) % N_SLOTS
                se.extend_raw([other, ended], np.zeros(20, np.int16), [0, 10, 20], [SCALING] * 2, [False, False])
            assert np.array_equal(se.lengths(), before)
            with pytest.raises(S.SfaError, match="not empty"):
                se.configure_raw(3, 25, 70)
            se.reset()
        with pytest.raises(S.SfaError):  # a bad list is refused by every shard alike, and the session goes on working
            se.configure_raw(3, 25, 70, (60, 50), False)
        se.configure_raw(3, 25, 70)
        with pytest.raises(S.SfaError):
            se.recalibrate((20,), False)
        at = [0] * N_SLOTS
        _, rows, _ = feed_raw(se, sigs, at, [900])
        assert rows["valid"].sum() >= 4
        se.close()


def test_resweep_on_rna_without_inv():
    rng = np.random.default_rng(104)
    ref = _small_ref(rng, [400, 300], True)
    sigs = [synth_signal(rng, int(rng.integers(600, 1500))) for _ in range(N_SLOTS)]
    with Pair(ref, S.RNA, [0, 0, 0]) as pair:
        with pytest.raises(S.SfaError):
            pair.many.session(N_SLOTS, spread=True)  # (as without the flag: a reversed query cannot be extended)
        se = pair.session(N_SLOTS, resweep=True)
        se.configure_raw(3, 25, 70, (50, 70), True)
        at = [0] * N_SLOTS
        swept = 0
        for call in range(6):
            named, rows, info = feed_raw(se, sigs, at, [260, 410])
            if not named:
                break
            swept += int((info["status"] & S.RAW_RECALIBRATED).astype(bool).sum())
            se.query_span(named)
        assert swept > 0 and rows["valid"].any()
        with pytest.raises(S.SfaError):
            se.extend([0], np.zeros(5, np.float32), [0, 5])
        se.close()


def test_automatic_query_start():
    """as tests/test_session_autostart_gpu.py sets it up, on reads that resolve"""
    c = load_case("rna_q500_pauto")
    ref = S.RefModel.from_fasta(c["fasta"], c["levels"], c["k"], S.RNA, 100)
    reads = synth.make_rna_polya_reads(N_SLOTS, seed=2, kinds=["normal"], body=(3000, 3500))
    every = 1600
    with Pair(ref, S.RNA, [0, 0]) as pair:
        se = pair.session(N_SLOTS, resweep=True, auto_start=dict(skip=4000, norm=25, query=100, recalibrate=tuple(S.recal_double(25, 100)), at_end=True, every=every,
                                                                max_samples=1 << 20))
        at, resolved = [0] * N_SLOTS, set()
        while any(at[sl] < len(reads[sl][5]) for sl in range(N_SLOTS)):
            named = [sl for sl in range(N_SLOTS) if at[sl] < len(reads[sl][5])]
            chunks = [reads[sl][5][at[sl]:at[sl] + every] for sl in named]
            for sl, x in zip(named, chunks):
                at[sl] += len(x)
            se.extend_raw(named, cat(chunks, np.int16), offsets(chunks), [reads[sl][1:4] for sl in named], [at[sl] == len(reads[sl][5]) for sl in named])
            au = se.auto_start(named[::-1])
            resolved |= {sl for sl, a in zip(named[::-1], au) if (int(a["status"]) & 15) == S.AUTO_RESOLVED}
            se.query_span(named)
        assert len(resolved) >= 4 and {sl % 2 for sl in resolved} == {0, 1}, resolved  # (about the inputs: reads on both shards resolve)
        assert se.spread.auto_ms() >= 0 and se.plain.auto_ms() >= 0  # (a time: not compared)
        se.close()


# ---- candidates, kept events and maps ----
@pytest.mark.parametrize("devices", DEVICE_LISTS, ids=IDS)
def test_candidates_and_event_maps(devices):
    rng = np.random.default_rng(105)
    ref = _small_ref(rng, [400, 300], False, quant=False)
    data = {sl: _events(rng, 120, False) for sl in range(N_SLOTS)}
    with Pair(ref, 0, devices) as pair:
        se = pair.session(N_SLOTS, candidates=4, keep_events=128)
        chunks = [data[sl][:40 + 10 * sl] for sl in range(N_SLOTS)]
        rows = se.extend(list(range(N_SLOTS)), cat(chunks, np.float32), offsets(chunks))
        chunks = [data[sl][40 + 10 * sl:60 + 10 * sl] for sl in (5, 2)]
        rows[[5, 2]] = se.extend([5, 2], cat(chunks, np.float32), offsets(chunks))
        cand = se.candidates([6, 0, 3, 1])
        assert cand["valid"][:, 0].all()
        assert np.array_equal(cand["score"][:, 0].view(np.uint32), rows["score2"][[6, 0, 3, 1]].view(np.uint32))
        # primaries and candidates whose slots lie on different shards, in an order that is not the shards'; one slot named twice
        m_slots = [6, 1, 0, 3, 6, 2, 5, 0]
        m_rows = np.array([rows[6], rows[1], cand[1][0], cand[2][1], cand[0][0], rows[2], rows[5], rows[0]], S.RESULT_DTYPE)
        pairs, off, on_host = se.event_maps(m_rows, m_slots)
        assert on_host == 0 and (np.diff(off) > 0).sum() >= 6
        # one row to the host routine inside the call: a budget that the largest row alone exceeds
        need = sorted(row_bytes(int(se.plain.lengths([m_slots[k]])[0]), int(off[k + 1] - off[k])) for k in range(len(m_slots)) if off[k + 1] > off[k])
        try:
            for al in (pair.one, pair.many):
                al.set_option("map_scratch_bytes", need[-1] - 1)
            again = se.event_maps(m_rows, m_slots)
        finally:
            for al in (pair.one, pair.many):
                al.set_option("map_scratch_bytes", 2 << 30)
        assert again[2] >= 1 and again[0].tobytes() == pairs.tobytes()
        with pytest.raises(S.SfaError, match="out of range"):
            se.event_maps(m_rows[:1], [N_SLOTS])
        se.close()


# ---- refusals, lifetime ----
def test_refusals():
    rng = np.random.default_rng(106)
    ref = _small_ref(rng, [400, 300], False)
    ev = _events(rng, 60, True)
    with S.Aligner(ref, 0, devices=[0, 0]) as al:
        with pytest.raises(S.SfaError, match="one device"):
            al.session(4)  # spread=False: as before
        with pytest.raises(S.SfaError, match="unknown flag"):
            al.session(4, flags=S.SESSION_SPREAD | 0x2)
        with pytest.raises(S.SfaError, match="unknown flag"):
            al.session(4, flags=S.SESSION_SPREAD | 0x8)
        with pytest.raises(S.SfaError):
            al.session(0, spread=True)
        with al.session(N_SLOTS, spread=True) as se:
            se.extend([0, 1, 2], ev, [0, 20, 40, 60])
            before = se.lengths().copy()
            for slots in ([N_SLOTS], [-1], [1, 1], [0, 2, 0], [3, 4, N_SLOTS], [4, 3, 4]):  # the last two: refused after another shard's entries
                off = np.arange(len(slots) + 1, dtype=np.int64) * 20
                with pytest.raises(S.SfaError, match="out of range|named twice"):
                    se.extend(slots, ev, off)
                assert np.array_equal(se.lengths(), before)  # a refused call changes nothing, on any shard
            with pytest.raises(S.SfaError):
                se.reset([N_SLOTS])
            with pytest.raises(S.SfaError):
                se.lengths([9])
            with pytest.raises(S.SfaError):
                se.candidates([0])  # keeps none
            with pytest.raises(S.SfaError):
                se.query_span([0])  # not in raw mode
            assert np.array_equal(se.lengths(), before)
            assert se.extend([1], ev[:20], [0, 20])["valid"][0] == 1
    with S.Aligner(ref, 0) as al, al.session(4, spread=True) as se:  # a single device: accepted, the plain session
        assert se.extend([1], ev[:20], [0, 20])["valid"][0] == 1


def test_session_outlives_nothing():
    """closing the Aligner while a spread session is open closes the session (the sub-sessions before their shards)"""
    rng = np.random.default_rng(107)
    ref = _small_ref(rng, [300], False)
    al = S.Aligner(ref, 0, devices=[0, 0, 0])
    se = al.session(5, spread=True)
    se.extend([0, 4], _events(rng, 60, True), [0, 30, 60])
    other = al.session(2, spread=True)
    other.close()
    al.close()
    with pytest.raises(S.SfaError):
        se.extend([0], _events(rng, 30, True), [0, 30])
    se.close()


# ---- realtime ----
def test_realtime_binary_and_replay(tmp_path):
    """`sigfish-amd realtime --device 0,0 --spread` prints the bytes of the run without --spread, and so does replay(spread=True)"""
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    c = load_case("dna_default")
    model = write_model(tmp_path / "syn.model", c["k"])
    base = [BIN, "realtime", "--kmer-model", model, "--verbose", "0", *[str(a) for a in c["args"]], "--channels", "3", "--chunk-samples", "1600", "--norm-events", "50",
            "--min-events", "100", "--min-mapq", "20", "--candidates", "2"]

    def run(*extra):
        r = subprocess.run(base + list(extra) + [c["fasta"], c["blow5"]], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        return r.stdout

    want = run()
    assert want.count(b"\n") >= 3
    assert run("--device", "0,0", "--spread") == want
    assert run("--device", "0,0,0,0", "--spread") == want  # (more shards than channels)
    r = subprocess.run(base + ["--device", "0,0", c["fasta"], c["blow5"]], capture_output=True, timeout=300)
    assert r.returncode != 0 and b"exactly one GPU" in r.stderr
    # the Python twin
    levels, k = S.read_kmer_model(model)
    query, skip = int(c["query_size"]), 50
    ref = S.RefModel.from_fasta(c["fasta"], levels, k, 0, query)
    reads = list(S.Blow5File(c["blow5"]))

    def lines(al, **kw):
        out = []
        for tick, ch, index, row, info, span, why, cand in realtime.replay(al, reads, 3, 1600, skip, 50, query, 100, 20, candidates=2, **kw):
            rid, _, raw = reads[index]
            out.append(realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why))
            out.append(realtime.format_candidates(rid, len(raw), ref.names, ref.seq_lengths, row, cand, info, span, why))
        return "".join(out)

    with S.Aligner(ref, 0) as one, S.Aligner(ref, 0, devices=[0, 0]) as many:
        plain = lines(one)
        assert lines(many, spread=True) == plain
        assert plain.encode() == want
