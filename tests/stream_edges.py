"""What tests/test_stream_edges_cpu.py and tests/test_stream_edges_gpu.py share: the reads of events_edge_cases.batch_a() (and one more, reads()) cut by the
schedules of stream_cuts.py, one session slot per (read, schedule) pair, laid out as the extend_raw calls of one session.  No GPU
is needed to build any of it; the CPU module asserts what the layout claims, so that the GPU module cannot pass vacuously.

Two session shapes (skip, norm, query).  Shape A holds SFA_MAX_QUERY events per slot, the largest query one launch sweeps in a
single piece and what configure_raw() takes by default (the call itself takes whatever device memory holds): most reads of the table
fit whole, the densest ones fill their slot.  Shape B has the smallest cap at which the expected tables hold a read that ends one
event short of full and a read whose table is filled by the finish step; schedules cut at the sample that fills a table add the
two remaining kinds."""
import functools
from collections import namedtuple

import numpy as np

import sigfish_amd as S
from tests import events_edge_cases as E
from tests import stream_cuts as K

NORM = 25            # the smallest calibration window sfa_session_raw_config takes
SHAPE_A = (0, NORM, 2048)
SKIP_B = 3
TRAILING = (0, False)   # one more call for every slot behind its end of read: an ended (or full) slot keeps its table and bits

Pair = namedtuple("Pair", "read name sched calls")   # read: index into reads(rna); calls: [(samples, end), ...]
# A session refuses a scaling whose fp32 offset or unit is not finite (SFA_EINVAL), so the table's range_inf reads reach the host
# twin only.  What they are for -- statistics that are not finite -- reaches the device through a finite range at which the fp32
# square of a sample overflows: the sums of squares are inf, their differences NaN, the means of most events inf.
REFUSED = "range_inf"
OVERFLOW = ("overflow_1600", "range_inf_1600", 1e38)   # name, the read whose samples it has, its range


@functools.lru_cache(maxsize=None)
def reads(rna):
    """events_edge_cases.batch_a(rna) and the overflowing read behind it -> list of (name, raw, scaling)"""
    name, of, rng = OVERFLOW
    raw, sc = E.cases(rna)[of]
    return E.batch_a(rna) + [(name, raw, (sc[0], sc[1], rng))]


@functools.lru_cache(maxsize=None)
def tables(rna):
    """the expected events: events_edge_cases.host_a(rna), and the batch detector's table of the read added here"""
    return E.host_a(rna) + [E.host_events(raw, sc, rna) for _, raw, sc in reads(rna)[len(E.batch_a(rna)):]]


def meta(sc):
    return dict(digitisation=sc[0], offset=sc[1], range=sc[2])


@functools.lru_cache(maxsize=None)
def split(rna):
    """per read of reads(rna): (events push() returns for the whole read, events finish() returns)"""
    out = []
    for _, raw, sc in reads(rna):
        with S.EventStream(meta(sc), rna) as es:
            out.append((len(es.push(raw)), len(es.finish())))
    return out


@functools.lru_cache(maxsize=None)
def fill_sample(rna, read, cap):
    """The number of samples at which the streamed detector emits event number `cap` (counting from 1) of a read, None where the
    samples alone never do.  The count after N samples does not depend on the cuts, so N is found by bisection."""
    _, raw, sc = reads(rna)[read]
    if split(rna)[read][0] < cap:
        return None

    def count(n):
        with S.EventStream(meta(sc), rna) as es:
            return len(es.push(raw[:n]))
    lo, hi = 0, len(raw)   # count(lo) < cap <= count(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if count(mid) >= cap else (mid, hi)
    return hi


def fill_kind(rna, read, calls, cap):
    """How a slot of `cap` events fed `calls` meets its cap: "mid" (the table fills inside a chunk), "last" (on a chunk's last
    sample), "end" (by an event of the finish step), "short" (the read ends one event short of full), or None."""
    pushed, fin = split(rna)[read]
    if pushed + fin == cap - 1:
        return "short"
    if pushed < cap:
        return "end" if pushed + fin >= cap else None
    return "last" if fill_sample(rna, read, cap) in K.boundaries([c for c in calls if c[0] > 0]) else "mid"


@functools.lru_cache(maxsize=None)
def shape_b(rna):
    """(skip, norm, query) with the smallest skip + query >= SKIP_B + NORM for which the expected tables hold a read one event short
    of full and a read of exactly that many events: its table is filled by the event the finish step emits."""
    sp = split(rna)
    totals = {p + f for p, f in sp}
    for cap in range(SKIP_B + NORM, max(totals) + 1):
        if cap - 1 in totals and cap in totals:   # (a read's last event is the one the finish step emits behind its walk)
            return (SKIP_B, NORM, cap - SKIP_B)
    raise AssertionError("no cap serves shape B")


def fill_schedules(n, at):
    """two schedules around the sample `at` that fills a slot's table: a chunk that ends on it, a chunk that has it in its middle"""
    s = {"fills_on_last_sample": K._cuts(n, [at])}
    if 3 <= at and at + 4 <= n:
        s["fills_mid_chunk"] = K._cuts(n, [at - 3, at + 4])
    return s


@functools.lru_cache(maxsize=None)
def pairs(rna, shape, every=False):
    """The (read, schedule) pairs of one session.  every: all of stream_cuts.schedules() for the long reads too, and the reads a
    session refuses (the CPU module)."""
    cap = shape[0] + shape[2]
    want = tables(rna)
    out = []
    for i, (name, raw, _) in enumerate(reads(rna)):
        if name.startswith(REFUSED) and not every:
            continue
        n = len(raw)
        sch = dict(K.schedules(n, rna, want[i]["start"]) if every else K.for_read(n, rna, want[i]["start"]))
        at = fill_sample(rna, i, cap)
        if at is not None:
            sch.update(fill_schedules(n, at))
        out += [Pair(i, name, k, tuple(v) + (TRAILING,)) for k, v in sch.items()]
    return out


def _find(prs, name, sched):
    return next(k for k, p in enumerate(prs) if p.name == name and p.sched == sched)


@functools.lru_cache(maxsize=None)
def layout(rna, shape):
    """-> (pairs, slot of each pair, order of the pairs inside every call, number of slots of the session).
    The order is one fixed shuffle; then the whole 18 433-sample read goes to entry 68 (block 1, lane 4) and two slots that are fed
    sample by sample to entries 100 (its partner in the other half of the wave) and 69 (the entry staged beside it: the two halves
    stage entries 2k and 2k + 1 together).  Every pair is in call 0, so the entries of call 0 are this order."""
    prs = pairs(rna, shape)
    rng = np.random.default_rng(20 + rna)
    order = [int(x) for x in rng.permutation(len(prs))]
    n_slots = len(prs) + 7
    slots = [int(x) for x in rng.permutation(n_slots)[:len(prs)]]
    ones = [k for k, p in enumerate(prs) if p.sched == "ones_then_rest"]
    for pos, k in ((68, _find(prs, "len_18433", "whole")), (100, ones[0]), (69, ones[1])):
        at = order.index(k)
        order[at], order[pos] = order[pos], order[at]
    return prs, slots, order, n_slots


def calls_of(rna, shape):
    """The session's extend_raw calls -> list of calls, each a list of (pair index, first sample, one behind the last, end)."""
    prs, _, order, _ = layout(rna, shape)
    at = [0] * len(prs)
    out = []
    for c in range(max(len(p.calls) for p in prs)):
        call = []
        for k in order:
            if c < len(prs[k].calls):
                n, end = prs[k].calls[c]
                call.append((k, at[k], at[k] + n, end))
                at[k] += n
        out.append(call)
    return out


def expected(rna, read, count, cap):
    """the first `count` events of the read's expected table, as far as the slot holds them"""
    return tables(rna)[read][:min(count, cap)]
