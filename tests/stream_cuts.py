"""Cut schedules for the streamed event detector (tests/test_stream_edges_cpu.py, tests/test_stream_edges_gpu.py): the ways of
cutting one read into calls at which ev_stream_kernel and sfa::EventStream take another path.  Plain Python, no GPU.

A schedule is a list of calls (samples, end): `samples` more samples of the read, and `end` true in the one call that carries the
end of the read, which is always the last.  The samples of a schedule add up to the read."""
from tests import events_model as M
from tests.test_event_stream_cpu import W_LONG

CHUNKS = (31, 32, 33, 63, 64, 65)   # around the tile of 32 samples the kernel stages per slot, and around two of them
LONG_READ = 1601   # a read of this many samples or more gets the two schedules of long_schedules() only (the table has none
                   # between 1600 and 3000 samples)


def _cuts(n, at):
    """calls that end at the sample counts `at` (ascending, <= n), the rest of the read with the end behind the last of them"""
    out, seen = [], 0
    for a in at:
        out.append((a - seen, False))
        seen = a
    return out + [(n - seen, True)]


def _chunks(n, k, upto=None):
    """chunks of k samples over the first `upto` samples (the whole read by default), then the rest; the end with the last samples"""
    upto = n if upto is None else min(upto, n)
    sizes = [k] * (upto // k) + ([upto % k] if upto % k else []) + ([n - upto] if n > upto else [])
    return [(c, False) for c in sizes[:-1]] + [(sizes[-1], True)]


def schedules(n, rna, starts=()):
    """Every named schedule that fits a read of n samples -> {name: [(samples, end), ...]}.  `starts`: the starts of the expected
    table's events; the first three give the cuts around the first call in which an event that ends there may exist."""
    wl, ws = W_LONG[rna], M.params(rna).w1   # the long and the short detector's window
    assert wl == M.params(rna).w2
    s = {"whole": [(n, True)],
         "whole_then_end": [(n, False), (0, True)],
         "empty_first": [(0, False), (n, True)]}
    if n >= 2 * wl + 2:   # sample by sample through the first walk at n == 2 w_long, which covers w_long + 1 positions at once
        s["ones_then_rest"] = [(1, False)] * (2 * wl + 2) + [(n - 2 * wl - 2, True)]
    for c in (2 * wl - 1, 2 * wl, 2 * wl + 1):
        if n >= c:
            s[f"cut_{c}"] = _cuts(n, [c])
    for k in CHUNKS:
        if n >= k:
            s[f"chunks_{k}"] = _chunks(n, k)
    for k in (32, 64):   # the end step falls into a tile of its own, in which no lane has a sample
        if n >= k:
            s[f"last_{k}"] = _cuts(n, [n - k])
    for name, t in (("1", 1), ("w_short", ws), ("w_long_minus_1", wl - 1), ("w_long", wl)):   # the last walk, over the zeros
        if n >= t:
            s[f"tail_{name}"] = _cuts(n, [n - t])
    if n >= 2:
        s["empty_between"] = [(n // 2, False), (0, False), (n - n // 2, True)]
    for k, st in enumerate(list(starts)[:3]):
        st = int(st)
        if st + wl <= n and st + wl - 1 >= 0:
            s[f"event_{k}_plus_w_long"] = _cuts(n, [st + wl - 1, st + wl])
    for calls in s.values():
        assert sum(c for c, _ in calls) == n and [e for _, e in calls] == [False] * (len(calls) - 1) + [True]
    return s


def long_schedules(n):
    """What a long read is fed: the whole read in one call, and chunks of 64 over its first 4096 samples, then the rest."""
    return {"whole": [(n, True)], "chunks_64_then_rest": _chunks(n, 64, upto=4096)}


def for_read(n, rna, starts=()):
    return long_schedules(n) if n >= LONG_READ else schedules(n, rna, starts)


def boundaries(calls):
    """sample counts after each call"""
    out, seen = [], 0
    for c, _ in calls:
        seen += c
        out.append(seen)
    return out
