"""The streamed event detector on the host (sfa::EventStream, host/events.cpp) on the crafted reads of tests/events_edge_cases.py,
cut by every schedule of tests/stream_cuts.py: whatever the cuts, the pushes plus finish() ARE the batch detector's table
(events_edge_cases.host_a(), pinned to the compiled reference) -- `start` exactly, the floats as uint32 views -- and after every
push the events so far are a prefix of it.  Then the claims tests/test_stream_edges_gpu.py rests on are shown without a GPU: the
table has the reads, and the two session shapes the layouts, that the device kernel's edges need.  No GPU."""
import numpy as np
import pytest

import sigfish_amd as S
from tests import events_edge_cases as E
from tests import events_model as M
from tests import stream_cuts as K
from tests import stream_edges as P
from tests.test_event_stream_cpu import W_LONG, same_events

CHEM = [pytest.param(False, id="dna"), pytest.param(True, id="rna")]


def test_schedules_are_the_named_ones():
    for rna in (False, True):
        wl = W_LONG[rna]
        s = K.schedules(1600, rna, starts=[0, 40, 57, 80])
        assert set(s) == {"whole", "whole_then_end", "empty_first", "empty_between", "ones_then_rest", f"cut_{2 * wl - 1}", f"cut_{2 * wl}",
                          f"cut_{2 * wl + 1}", "chunks_31", "chunks_32", "chunks_33", "chunks_63", "chunks_64", "chunks_65", "last_32", "last_64",
                          "tail_1", "tail_w_short", "tail_w_long_minus_1", "tail_w_long", "event_0_plus_w_long", "event_1_plus_w_long",
                          "event_2_plus_w_long"}
        assert s["ones_then_rest"][:2 * wl + 2] == [(1, False)] * (2 * wl + 2) and len(s["ones_then_rest"]) == 2 * wl + 3
        assert s["whole_then_end"] == [(1600, False), (0, True)] and s["empty_first"][0] == (0, False)
        assert s["last_32"][-1] == (32, True) and s["last_64"][-1] == (64, True) and s["tail_w_long"][-1] == (wl, True)
        assert s["chunks_33"][:2] == [(33, False)] * 2 and s["chunks_33"][-1] == (1600 % 33, True)
        assert K.boundaries(s["event_1_plus_w_long"])[:2] == [40 + wl - 1, 40 + wl] and (0, False) in s["empty_between"]
        assert set(K.schedules(0, rna)) == {"whole", "whole_then_end", "empty_first"}
        assert "chunks_33" not in K.schedules(32, rna) and "last_32" in K.schedules(32, rna)
        long = K.long_schedules(18433)
        assert set(long) == {"whole", "chunks_64_then_rest"} and long["chunks_64_then_rest"][63:] == [(64, False), (18433 - 4096, True)]


@pytest.mark.parametrize("rna", CHEM)
def test_every_schedule_gives_the_batch_table(rna):
    """every read times every schedule, each with the read's own scaling"""
    batch, want = P.reads(rna), P.tables(rna)
    n_runs = 0
    for p in P.pairs(rna, P.SHAPE_A, every=True):
        name, raw, sc = batch[p.read]
        ev, at, count = want[p.read], 0, 0
        with S.EventStream(P.meta(sc), rna) as es:
            for c, end in p.calls[:-1]:   # (the trailing call is the session's)
                got = es.push(raw[at:at + c])
                at += c
                same_events(got, ev[count:count + len(got)], (name, p.sched, "the events after", at, "samples are no prefix of the table"))
                count += len(got)
                if end:
                    got = es.finish()
                    same_events(got, ev[count:], (name, p.sched, "finish"))
                    count += len(got)
        assert at == len(raw) and count == len(ev), (name, p.sched)
        n_runs += 1
    assert n_runs > 1500


@pytest.mark.parametrize("rna", CHEM)
def test_the_table_serves_the_stream(rna):
    batch, want, sp = P.reads(rna), P.tables(rna), P.split(rna)
    assert all(a[1] is b[1] and a[2] == b[2] for a, b in zip(batch, E.batch_a(rna))) and len(batch) == len(E.batch_a(rna)) + 1   # the same table,
    assert all(a is b for a, b in zip(want, E.host_a(rna))) and len(want) == len(batch)                                        # the same expected events
    names = [b[0] for b in batch]
    assert [p + f for p, f in sp] == [len(ev) for ev in want]
    # a read with samples and no cut at all ends with zero events; one read has all its events from the finish step's walk
    assert any(len(b[1]) >= 1600 and len(ev) == 0 for b, ev in zip(batch, want))
    # the last event of a read is the one finish() emits (test_every_schedule_gives_the_batch_table compared it), also where the
    # finish step's walk adds nothing before it, and where the samples alone have cut nothing
    assert any(p > 0 and f == 1 for p, f in sp) and any(p > 0 and f > 1 for p, f in sp) and any(p == 0 and f > 0 for p, f in sp)
    for content in ("range_inf", "tiny_offset"):
        assert any(n.startswith(content) for n in names)
    for i, (name, raw, sc) in enumerate(batch):   # ... and they are what they say: a non-finite unit, samples of 1e-30 pA
        if name.startswith("range_inf"):
            assert np.isinf(np.float32(sc[2]) / np.float32(sc[0])) and len(want[i]) == 0
        if name.startswith("tiny_offset"):
            assert sc[1] == 1e-30 and (raw == 0).sum() > 10 and len(want[i]) > 50
    scales = {b[2] for b in batch}
    assert {E.SCALE, E.UNIT_SCALE} <= scales and len(scales) == 5
    # the read added to the table: a finite scaling (a session takes it) under which fp32 squares overflow
    name, raw, sc = batch[-1]
    assert name == P.OVERFLOW[0] and np.isfinite(np.float32(sc[2]) / np.float32(sc[0])) and 0 < len(want[-1]) < P.NORM
    with np.errstate(over="ignore"):
        assert np.isfinite(M.picoamps(raw, sc)).all() and np.isinf(np.square(M.picoamps(raw, sc))).all() and np.isinf(want[-1]["mean"]).any()
    assert not any(p.name.startswith(P.REFUSED) for p in P.pairs(rna, P.SHAPE_A))   # (a session refuses them: the host twin alone has them)
    for shape in (P.SHAPE_A, P.shape_b(rna)):   # the end of the read in a call without samples, behind samples and behind nothing
        ends = [p for p in P.pairs(rna, shape) if (0, True) in p.calls]
        assert any(len(batch[p.read][1]) > 0 for p in ends) and any(len(batch[p.read][1]) == 0 for p in ends)
    # both kinds of reads: every schedule for the short ones, two for the long ones
    per_read = {}
    for p in P.pairs(rna, P.SHAPE_A):
        per_read.setdefault(p.read, []).append(p.sched)
    for i, (name, raw, _) in enumerate(batch):
        if name.startswith(P.REFUSED):
            assert i not in per_read
        elif len(raw) >= K.LONG_READ:
            assert {"whole", "chunks_64_then_rest"} <= set(per_read[i]) <= {"whole", "chunks_64_then_rest", "fills_on_last_sample", "fills_mid_chunk"}, name
        elif len(raw) >= 65:
            assert len(per_read[i]) >= 20, (name, per_read[i])
    assert sum(len(v) >= 20 for v in per_read.values()) >= 15


@pytest.mark.parametrize("rna", CHEM)
def test_shape_a_fits_most_reads_and_shape_b_meets_its_cap_in_four_ways(rna):
    want = P.tables(rna)
    cap_a = P.SHAPE_A[0] + P.SHAPE_A[2]
    whole = sum(len(ev) < cap_a for ev in want)
    assert 3 <= len(want) - whole <= 8   # most reads fit whole, some fill their slot
    skip, norm, query = P.shape_b(rna)
    cap = skip + query
    assert norm == P.NORM <= query and cap < 1000
    kinds = {}
    for p in P.pairs(rna, (skip, norm, query)):
        kinds.setdefault(P.fill_kind(rna, p.read, p.calls, cap), []).append((p.name, p.sched))
    for kind in ("mid", "last", "end", "short"):
        assert kinds.get(kind), kind
    # the event that fills the table is the very one the finish step emits behind its walk, for one read at least
    assert any(p + f == cap and f >= 1 for p, f in P.split(rna))
    # what fill_sample says, against a run sample by sample over one read
    read = next(i for i, (p, f) in enumerate(P.split(rna)) if p >= cap)
    _, raw, sc = P.reads(rna)[read]
    with S.EventStream(P.meta(sc), rna) as es:
        counts = np.cumsum([len(es.push(raw[j:j + 1])) for j in range(P.fill_sample(rna, read, cap) + 2)])
    at = P.fill_sample(rna, read, cap)
    assert counts[at - 2] < cap <= counts[at - 1]


@pytest.mark.parametrize("rna", CHEM)
def test_the_calls_are_laid_out_as_claimed(rna):
    batch = P.reads(rna)
    for shape in (P.SHAPE_A, P.shape_b(rna)):
        prs, slots, order, n_slots = P.layout(rna, shape)
        calls = P.calls_of(rna, shape)
        assert sorted(order) == list(range(len(prs))) and len(set(slots)) == len(prs) and max(slots) < n_slots
        assert order != sorted(order) and slots != sorted(slots)
        assert [k for k, _, _, _ in calls[0]] == order and 20 <= len(calls) <= 80
        assert len(calls[0]) >= 130 and sum(len(c) >= 130 and len(c) % 64 != 0 for c in calls) >= 2   # blocks 0, 1, ... and a partly filled last one
        sizes = sorted({len(c) for c in calls})
        assert sizes[0] < 64 < 128 < sizes[-1]
        # half-wave partners (entries i and i + 32 of a block) and the two entries staged together (2k and 2k + 1): one sample beside
        # the table's longest read, in block 1
        lens = [hi - lo for _, lo, hi, _ in calls[0]]
        assert (lens[68], lens[100], lens[69]) == (18433, 1, 1) and 68 // 64 == 100 // 64 == 1 and 68 % 64 + 32 == 100 % 64
        # one call mixes the four scalings
        assert len({batch[prs[k].read][2] for k, _, _, _ in calls[0][:192]}) == 4
        for k, p in enumerate(prs):   # every slot is named once more behind its end of read
            assert p.calls[-1] == P.TRAILING and p.calls[-2][1]
