"""Event maps of a session's rows from the device (sfa_session_event_maps, sfa_session_keep_events): the map of every row a
session returned -- primaries and candidates, raw mode, resweep and event mode -- equals the host routine's
(api.r2qevent_map on the slot's event table, or on the events sent), and the batch route's (Aligner.align_db + Aligner.event_maps
of the query so far).  Maps are integers: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib, synth
from tests.test_session_gpu import _events, _small_ref, assert_rows
from tests.test_session_raw_gpu import SCALING, synth_signal

pytestmark = pytest.mark.gpu

MAX_QUERY = 2048  # SFA_MAX_QUERY
NONE = np.iinfo(np.int32).min  # what Session.event_maps leaves where the library wrote nothing
EINVAL, ERANGE = "(-1)", "(-4)"
CLASSES = ((1, 64), (65, 128), (129, 256), (257, 512), (513, 1024), (1025, 2048))  # query events per band-fill class
META = synth.R9_DNA_META
SCALE = (META["digitisation"], META["offset"], META["range"])


def class_of(q):
    return next((i for i, (lo, hi) in enumerate(CLASSES) if lo <= q <= hi), len(CLASSES))


def host_map(ref, flag, row, events, qs, qe):
    """api.r2qevent_map of one row, None where the host routine returns SFA_EINVAL (the device leaves such a row unwritten)"""
    j, plus = int(row["rid"]), row["strand"] == ord("+")
    arr = ref.forward[j] if plus else ref.reverse[j]
    try:
        return S.r2qevent_map(row, events, qs, qe, arr, int(ref.st_offset[j]), flag)
    except S.SfaError:
        return None


def assert_maps(pairs, off, k, want, what):
    got = pairs[off[k]:off[k + 1]]
    if want is None:
        assert len(got) == 0 or (got == NONE).all(), what
    else:
        assert got.shape == want.shape and np.array_equal(got, want), (what, got[:6], want[:6])


def normalised(ev, skip, q, mean, sd):
    """the slot's event table with the query's means as the device normalised them: (mean_e - mean) / sd in fp32"""
    out = ev.copy()
    out["mean"][skip:skip + q] = ((ev["mean"][skip:skip + q] - np.float32(mean)) / np.float32(sd)).astype(np.float32)
    return out


def mapped(rows):
    return (rows["valid"] != 0) & (rows["rid"] >= 0)


@pytest.fixture(scope="module")
def dna():
    """three contigs of 2605 / 905 / 305 bases (2600 / 900 / 300 columns), the second repeating a stretch of the first; raw reads
    that follow them: one long enough for 2100 query events, the others 2000 .. 9000 samples"""
    k = 6
    levels = synth.kmer_levels(k, 21)
    c0 = synth.random_sequence(2605, 1)
    recs = [("c0", c0), ("c1", c0[700:1605]), ("c2", synth.random_sequence(305, 3))]
    ref = S.RefModel.from_records(recs, levels, k, 0, 250)
    assert list(ref.ref_lengths) == [2600, 900, 300]
    long_read = synth.make_dna_raw_reads(recs[:1], levels, k, 1, seed=8, samples=(24000, 24000), meta=META)
    reads = long_read + synth.make_dna_raw_reads(recs, levels, k, 7, seed=5, samples=(2000, 9000), kinds=("mapped", "mapped", "random"), meta=META)
    return dict(ref=ref, sigs=[r[5] for r in reads])


def feed(se, sigs, at, sizes):
    """one extend_raw call: slot i takes the next sizes[i] samples of its signal (slots whose signal is used up are not named)"""
    named = [sl for sl in range(len(sigs)) if at[sl] < len(sigs[sl]) and sizes[sl] > 0]
    chunks = []
    for sl in named:
        n = min(sizes[sl], len(sigs[sl]) - at[sl])
        chunks.append(sigs[sl][at[sl]:at[sl] + n])
        at[sl] += n
    raw_off = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
    rows, info = se.extend_raw(named, np.concatenate(chunks), raw_off, [SCALE] * len(named), [at[sl] == len(sigs[sl]) for sl in named])
    return named, rows, info


SKIP, NORM, QUERY = 3, 25, 2100
POINTS = (60, 120, 250, 500, 1000, 2048, 2100)  # windows change as a read grows, as under --recalibrate


def run_raw(al, dna, schedule, seen, batch_check_at=()):
    """a raw session over the workload; after every call that returns a valid row, the maps of all valid rows against the host
    routine.  schedule(call, slot) -> samples.  seen: the band-fill classes met; -> the largest n_on_host"""
    ref, sigs = dna["ref"], dna["sigs"]
    n_slots = len(sigs)
    most_on_host = 0
    with al.session(n_slots) as se:
        se.configure_raw(SKIP, NORM, QUERY, POINTS)
        at = [0] * n_slots
        call = 0
        while any(at[sl] < len(sigs[sl]) for sl in range(n_slots)):
            named, rows, info = feed(se, sigs, at, [schedule(call, sl) for sl in range(n_slots)])
            call += 1
            ok = mapped(rows)
            if not ok.any():
                continue
            pairs, off, on_host = se.event_maps(rows, named)
            assert len(off) == len(named) + 1 and off[-1] == len(pairs)
            q = info["q_events"]
            assert on_host == int((q[ok] > MAX_QUERY).sum()), (call, on_host, q)
            most_on_host = max(most_on_host, on_host)
            evn = {}
            for i, sl in enumerate(named):
                if not ok[i]:
                    assert off[i + 1] == off[i]
                    continue
                seen.add(class_of(int(q[i])))
                evn[sl] = normalised(se.events(sl), SKIP, int(q[i]), info["norm_mean"][i], info["norm_sd"][i])
                assert_maps(pairs, off, i, host_map(ref, 0, rows[i], evn[sl], SKIP, SKIP + int(q[i])), (call, sl, int(q[i])))
            if call in batch_check_at:  # the batch route: the query so far through align_db, its maps from Aligner.event_maps
                idx = [i for i in range(len(named)) if ok[i]]
                qs = [evn[named[i]]["mean"][SKIP:SKIP + int(q[i])].copy() for i in idx]
                q_off = np.concatenate([[0], np.cumsum([len(x) for x in qs])]).astype(np.int64)
                b_rows = al.align_db(np.concatenate(qs), q_off)
                assert_rows(rows[idx], b_rows, True, ("batch rows", call))
                before = al.event_maps()
                again, off2, _ = se.event_maps(rows, named)  # a session call in between ...
                after = al.event_maps()                       # ... leaves the batch maps as they were
                assert again.tobytes() == pairs.tobytes() and np.array_equal(off, off2)
                assert len(before) == len(after) == len(idx)
                for j, i in enumerate(idx):
                    assert before[j].tobytes() == after[j].tobytes()
                    got = pairs[off[i]:off[i + 1]]
                    assert (len(before[j]) == 0 and (got == NONE).all()) or before[j].tobytes() == got.tobytes(), (call, named[i])
                again, _, _ = se.event_maps(rows, named)      # and a batch call leaves the session's
                assert again.tobytes() == pairs.tobytes()
    return most_on_host


def test_raw_tracked_every_class_and_the_batch_route(dna):
    seen = set()
    uneven = (350, 150, 420, 1, 800, 1600, 3100, 333, 6000, 2500)
    with S.Aligner(dna["ref"], 0) as al:
        # 1600-sample chunks (a tick at 4 kHz): the long read grows through the classes above 128 events and beyond 2048
        most = run_raw(al, dna, lambda call, sl: 1600, seen, batch_check_at=(3, 15))
        assert most == 1  # one slot beyond SFA_MAX_QUERY: its map comes from the host routine inside the call, and is the same map
        # uneven chunks, other sizes per slot: the small classes, slots out of step with each other
        run_raw(al, dna, lambda call, sl: uneven[(call + 3 * sl) % len(uneven)], seen, batch_check_at=(6,))
    assert seen == set(range(len(CLASSES) + 1)), seen  # (about this test's own inputs: every class, and one beyond them)


def test_candidates_and_one_slot_named_five_times(dna):
    ref, sigs = dna["ref"], dna["sigs"]
    n_slots = len(sigs)
    n_cand_rows = n_two_loci = 0
    with S.Aligner(ref, 0) as al, al.session(n_slots, candidates=4) as se:
        se.configure_raw(SKIP, NORM, 250, (50, 100, 250))
        at = [0] * n_slots
        for call in range(4):
            named, rows, info = feed(se, sigs, at, [900] * n_slots)
            if not mapped(rows).any():
                continue
            cand = se.candidates(named)
            # primary + four candidates per slot, in one call: every slot is named five times
            m_rows = np.concatenate([np.concatenate([rows[i:i + 1], cand[i]]) for i in range(len(named))])
            m_slots = np.repeat(np.asarray(named, np.int32), 5)
            pairs, off, on_host = se.event_maps(m_rows, m_slots)
            assert on_host == 0
            for i, sl in enumerate(named):
                if not mapped(rows[i:i + 1])[0]:
                    assert off[5 * i + 5] == off[5 * i]
                    continue
                q = int(info["q_events"][i])
                evn = normalised(se.events(sl), SKIP, q, info["norm_mean"][i], info["norm_sd"][i])
                for k in range(5):
                    r = m_rows[5 * i + k]
                    if not mapped(m_rows[5 * i + k:5 * i + k + 1])[0]:
                        assert off[5 * i + k + 1] == off[5 * i + k]
                        continue
                    assert_maps(pairs, off, 5 * i + k, host_map(ref, 0, r, evn, SKIP, SKIP + q), (call, sl, k))
                    n_cand_rows += k > 0
                n_two_loci += len({int(r["rid"]) for r in m_rows[5 * i:5 * i + 5] if r["valid"]}) > 1
    assert n_cand_rows >= 8 and n_two_loci >= 1, (n_cand_rows, n_two_loci)  # (about this test's own inputs)


@pytest.mark.parametrize("name", ["rna_reversed", "dna_forward"])
def test_resweep(name):
    """the query is the window's W events as stored (reversed on the RNA context): maps against r2qevent_map over events
    [skip, skip + W) with the context's flag; a call that leaves W alone returns the same maps again"""
    flag, lens = {"rna_reversed": (S.RNA, [1200, 400]), "dna_forward": (0, [700, 301])}[name]
    rng = np.random.default_rng(31)
    ref = _small_ref(rng, lens, bool(flag & S.RNA), quant=False)
    skip, norm, query, points = 10, 25, 200, (50, 100, 200)
    n_slots = 5
    sigs = [synth_signal(rng, n) for n in (3000, 2600, 1500, 700, 2200)]
    windows, unchanged = set(), 0
    with S.Aligner(ref, flag) as al, al.session(n_slots, resweep=True) as se:
        se.configure_raw(skip, norm, query, points)
        at, last = [0] * n_slots, {}
        call = 0
        while any(at[sl] < len(sigs[sl]) for sl in range(n_slots)):
            call += 1
            named = [sl for sl in range(n_slots) if at[sl] < len(sigs[sl])]
            chunks = []
            for sl in named:
                n = min((160, 250, 90, 300, 210)[sl], len(sigs[sl]) - at[sl])
                chunks.append(sigs[sl][at[sl]:at[sl] + n])
                at[sl] += n
            raw_off = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
            rows, info = se.extend_raw(named, np.concatenate(chunks), raw_off, [SCALING] * len(named), [at[sl] == len(sigs[sl]) for sl in named])
            pairs, off, on_host = se.event_maps(rows, named)
            assert on_host == 0
            for i, sl in enumerate(named):
                if not mapped(rows[i:i + 1])[0]:
                    assert off[i + 1] == off[i]
                    continue
                W = int(info["q_events"][i])
                assert W == int(info["norm_window"][i])
                ev = se.events(sl)
                evn = ev.copy()
                evn["mean"][skip:skip + W] = S.znormalise(ev["mean"][skip:skip + W])
                assert_maps(pairs, off, i, host_map(ref, flag, rows[i], evn, skip, skip + W), (name, call, sl, W))
                got = pairs[off[i]:off[i + 1]].tobytes()
                if sl in last and last[sl][0] == W:
                    assert last[sl][1] == got and last[sl][2] == rows[i].tobytes()
                    unchanged += 1
                last[sl] = (W, got, rows[i].tobytes())
                windows.add(W)
    assert windows >= {25, 50, 100, 200} and unchanged >= 5, (windows, unchanged)  # (about this test's own inputs)


def extend(se, slots, chunks):
    ev_off = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
    return se.extend(slots, np.concatenate(chunks) if chunks else np.zeros(0, np.float32), ev_off)


def raw_events(x):
    """an event table whose means are the events sent (the host routine reads nothing else)"""
    ev = np.zeros(len(x), S.EVENT_DTYPE)
    ev["mean"] = x
    return ev


def test_event_mode_keep_events():
    rng = np.random.default_rng(17)
    ref = _small_ref(rng, [700, 301], False, quant=False)
    max_events = 400
    data = {0: _events(rng, 352, False), 1: _events(rng, 900, False), 2: _events(rng, 130, False), 3: _events(rng, 400, False)}
    # chunks of 1, 50 and 300 events; slot 1 outgrows max_events in its second chunk; slot 3 ends exactly at max_events
    sched = {0: [1, 1, 50, 300, None, 0], 1: [300, 300, 300, None, None, None], 2: [None, 50, 1, 50, 29, None], 3: [50, 300, 50, None, None, 0]}
    with S.Aligner(ref, 0) as al, al.session(4, keep_events=max_events) as se, al.session(4) as plain:
        used = {sl: 0 for sl in sched}
        for call in range(6):
            named = [sl for sl in sched if sched[sl][call] is not None]
            chunks = [data[sl][used[sl]:used[sl] + sched[sl][call]] for sl in named]
            for sl in named:
                used[sl] += sched[sl][call]
            rows = extend(se, named, chunks)
            assert rows.tobytes() == extend(plain, named, chunks).tobytes()  # the rows of a session without the feature, byte for byte
            fits = [i for i, sl in enumerate(named) if used[sl] <= max_events]
            over = [i for i, sl in enumerate(named) if used[sl] > max_events]
            pairs, off, on_host = se.event_maps(rows[fits], [named[i] for i in fits])
            assert on_host == 0
            for k, i in enumerate(fits):
                sl = named[i]
                assert mapped(rows[i:i + 1])[0]
                assert_maps(pairs, off, k, host_map(ref, 0, rows[i], raw_events(data[sl][:used[sl]]), 0, used[sl]), (call, sl, used[sl]))
            for i in over:  # still sweeping, still a row; only its maps are refused
                assert mapped(rows[i:i + 1])[0]
                with pytest.raises(S.SfaError, match="more than the 400"):
                    se.event_maps(rows[i:i + 1], [named[i]])
            if over:
                with pytest.raises(S.SfaError) as e:
                    se.event_maps(rows, named)
                assert EINVAL in str(e.value)
        with pytest.raises(S.SfaError, match="not empty"):
            se.keep_events(0)
        # after a reset the slot that had outgrown the session works again
        se.reset([1])
        rows = extend(se, [1], [data[1][:77]])
        pairs, off, _ = se.event_maps(rows, [1])
        assert_maps(pairs, off, 0, host_map(ref, 0, rows[0], raw_events(data[1][:77]), 0, 77), "after reset")
        assert len(pairs) > 0 and (pairs != NONE).all()
        # switched off while every slot is empty: maps are refused, rows go on
        se.reset()
        se.keep_events(0)
        rows = extend(se, [2], [data[2][:60]])
        with pytest.raises(S.SfaError, match="sfa_session_keep_events"):
            se.event_maps(rows, [2])


def row_bytes(q, m):
    """packed moves of one row (sfa_plan.hpp, map_row_bytes): (m + lanes - 1) x lanes x words x 4 in the class's shape"""
    R, lanes = ((4, 16), (8, 16), (16, 16), (32, 16), (32, 32), (32, 64))[class_of(q)]
    return (m + lanes - 1) * lanes * (2 if R == 32 else 1) * 4


def test_scratch_budget_slices_and_one_host_row(dna):
    ref, sigs = dna["ref"], dna["sigs"]
    n_slots = len(sigs)
    with S.Aligner(ref, 0) as al, al.session(n_slots) as se:
        se.configure_raw(SKIP, NORM, 600, (100, 300, 600))
        at = [0] * n_slots
        for sizes in ([5000, 1500, 2500, 900, 3000, 700, 1100, 2000], [1000] * n_slots):
            named, rows, info = feed(se, sigs, at, sizes)
        ok = mapped(rows)
        assert ok.sum() >= 6
        want, off, on_host = se.event_maps(rows, named)
        assert on_host == 0 and (want != NONE).all()
        need = sorted(row_bytes(int(info["q_events"][i]), int(off[i + 1] - off[i])) for i in range(len(named)) if ok[i])
        assert need[-1] > need[-2]
        try:
            al.set_option("map_scratch_bytes", need[-2])  # the largest row alone exceeds it; no two of the larger rows share a slice
            got, off2, on_host = se.event_maps(rows, named)
        finally:
            al.set_option("map_scratch_bytes", 2 << 30)
        assert on_host == 1 and np.array_equal(off, off2) and got.tobytes() == want.tobytes()
        assert sum(need[:-1]) > 2 * need[-2]  # (about this test's own inputs: the device rows cannot fit fewer than three slices)


def test_refusals_and_rows_that_write_nothing(dna):
    ref, sigs = dna["ref"], dna["sigs"]
    n_slots = len(sigs)
    L = _lib.load()
    with S.Aligner(ref, 0) as al:
        with al.session(n_slots) as se:
            se.configure_raw(SKIP, NORM, 250)
            at = [0] * n_slots
            named, rows, info = feed(se, sigs, at, [2500] * n_slots)
            assert named == list(range(n_slots)) and mapped(rows).sum() >= 6
            with pytest.raises(S.SfaError) as e:  # a slot out of range
                se.event_maps(rows[:1], [n_slots])
            assert EINVAL in str(e.value)
            with pytest.raises(S.SfaError) as e:
                se.event_maps(rows[:1], [-1])
            assert EINVAL in str(e.value)
            with pytest.raises(S.SfaError) as e:  # keep_events on a raw session: its query is kept already
                se.keep_events(100)
            assert EINVAL in str(e.value)
            bad = rows[:1].copy()  # a row whose band leaves its array, a contig that does not exist
            bad["pos_end"] = 10 ** 6
            with pytest.raises(S.SfaError) as e:
                se.event_maps(bad, [0])
            assert EINVAL in str(e.value)
            bad = rows[:1].copy()
            bad["rid"] = 3
            with pytest.raises(S.SfaError) as e:
                se.event_maps(bad, [0])
            assert EINVAL in str(e.value)
            # the C call itself: a gap too small is SFA_ERANGE; rows with valid = 0 write nothing, with sentinel words around
            off = S.map_offsets(rows)
            sl = np.asarray(named, np.int32)
            short = off.copy()
            k = int(np.argmax(mapped(rows)))
            short[k + 1:] -= 1
            buf = np.full(2 * int(off[-1]) + 16, 0x5A5A5A5A, np.int32)

            def call(r, offsets):
                return L.sfa_session_event_maps(se._h, r.ctypes.data_as(C.c_void_p), sl.ctypes.data_as(_lib.i32p), len(r), offsets.ctypes.data_as(_lib.i64p),
                                                buf[8:].ctypes.data_as(_lib.i32p), None)

            assert call(rows, short) == -4 and (buf == 0x5A5A5A5A).all()
            dead = rows.copy()
            dead["valid"][::2] = 0  # every other row is no row: its gap (left as it was) and the words around stay untouched
            assert call(dead, off) == 0
            assert (buf[:8] == 0x5A5A5A5A).all() and (buf[8 + 2 * int(off[-1]):] == 0x5A5A5A5A).all()
            for i in range(len(rows)):
                piece = buf[8 + 2 * int(off[i]):8 + 2 * int(off[i + 1])]
                if i % 2 == 0 or not mapped(rows[i:i + 1])[0]:
                    assert (piece == 0x5A5A5A5A).all(), i
                else:
                    assert len(piece) > 0 and (piece != 0x5A5A5A5A).all(), i
            # an emptied slot's rows are such rows; a stale valid row for it is refused
            se.reset([2])
            _, rows2, _ = feed(se, sigs, at, [0 if s != 2 else 10 for s in range(n_slots)])
            assert not rows2["valid"][0]
            pairs, off2, _ = se.event_maps(rows2, [2])
            assert len(pairs) == 0
            with pytest.raises(S.SfaError) as e:
                se.event_maps(rows[2:3], [2])
            assert EINVAL in str(e.value)
        with al.session(2, starts=False) as se:  # no start column, no band
            se.configure_raw(SKIP, NORM, 250)
            rows, info = se.extend_raw([0], sigs[1][:2500], [0, 2500], [SCALE], [False])
            assert rows["valid"][0]
            with pytest.raises(S.SfaError, match="SFA_SESSION_NO_START") as e:
                se.event_maps(rows, [0])
            assert EINVAL in str(e.value)
        rng = np.random.default_rng(3)
        with al.session(2) as se:  # event mode, no kept events
            rows = extend(se, [0], [_events(rng, 80, False)])
            with pytest.raises(S.SfaError, match="sfa_session_keep_events") as e:
                se.event_maps(rows, [0])
            assert EINVAL in str(e.value)
            with pytest.raises(S.SfaError, match="not empty") as e:  # keep_events with a slot in use
                se.keep_events(100)
            assert EINVAL in str(e.value)
            se.reset()
            se.keep_events(100)
            rows = extend(se, [1], [_events(rng, 80, False)])
            pairs, off, _ = se.event_maps(rows, [1])
            assert len(pairs) == int(rows["pos_end"][0] - rows["pos_st"][0] + 1)
