"""The streaming event detector on the host (sfa_event_stream_*, host/events.cpp) against the batch detector sfa_detect_events:
whatever the chunking, everything push() returned plus what finish() returned IS the batch table over the whole signal -- all four
fields, the floats compared as uint32 views, no tolerance.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib
from tests.util import GOLD, ROOT

W_LONG = {False: 6, True: 14}  # the long detector's window, DNA / RNA (src/events.c:47-58)


def _fixture_reads(name):
    f = S.Blow5File(os.path.join(GOLD, "data", name))
    out = [(meta, np.array(sig, np.int16)) for _, meta, sig in f]
    f.close()
    return out


FIX = {False: "sp1_dna.blow5", True: "sequin_rna.blow5"}


@pytest.fixture(scope="module")
def fixture_reads():
    return {rna: _fixture_reads(name) for rna, name in FIX.items()}


def synth_signal(rng, n, meta):
    """piecewise-constant levels ~N(90, 12) pA, dwell 6..12 samples, noise sd 1.5, as ADC counts of `meta`"""
    n_lv = n // 6 + 2
    pa = np.repeat(rng.normal(90, 12, n_lv), rng.integers(6, 13, n_lv))[:n] + rng.normal(0, 1.5, n)
    return np.round(pa * meta["digitisation"] / meta["range"] - meta["offset"]).astype(np.int16)


def same_events(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    assert np.array_equal(got["start"], want["start"]), what
    for f in ("length", "mean", "stdv"):
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), (what, f)


def stream(raw, meta, rna, chunks):
    """-> (list of event arrays, one per push, samples seen after each push, what finish returned)"""
    per_push, seen, at = [], [], 0
    with S.EventStream(meta, rna) as es:
        for c in chunks:
            per_push.append(es.push(raw[at:at + c]))
            at += c
            seen.append(at)
        assert at == len(raw)
        fin = es.finish()
        with pytest.raises(S.SfaError):  # samples after the end, a second end
            es.push(raw[:1])
        with pytest.raises(S.SfaError):
            es.finish()
    return per_push, seen, fin


def cut(n, sizes):
    """chunk lengths: `sizes` cycled until n samples are covered"""
    out, at, i = [], 0, 0
    while at < n:
        c = min(sizes[i % len(sizes)], n - at)
        out.append(c)
        at += c
        i += 1
    return out


def schedules(rng, n, rna):
    wl = W_LONG[rna]
    s = {"whole": [n],
         "random": cut(n, list(rng.integers(1, 401, 64))),
         "with_empty": cut(n, [0, 37, 0, 0, 250, 0]) + [0],
         "around_2w": cut(n, [2 * wl - 1, 1, 1, 300])}
    if n <= 600:
        s["ones"] = [1] * n
    return s


def check_signal(raw, meta, rna, rng, what):
    want = S.detect_events(raw, meta, rna)
    counts_at = {}  # samples seen -> events emitted so far: must not depend on the chunking (c)
    for name, chunks in schedules(rng, len(raw), rna).items():
        per_push, seen, fin = stream(raw, meta, rna, chunks)
        before = np.concatenate(per_push) if per_push else np.zeros(0, S.EVENT_DTYPE)
        same_events(np.concatenate([before, fin]), want, (what, name))  # (a)
        same_events(before, want[:len(before)], (what, name, "prefix"))  # (b)
        total = 0
        for ev, n_seen in zip(per_push, seen):
            total += len(ev)
            assert counts_at.setdefault(n_seen, total) == total, (what, name, n_seen)
            if n_seen < 2 * W_LONG[rna]:
                assert total == 0  # nothing is processed while N < 2 w_long
    return want, counts_at


@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna"])
def test_fixture_reads_any_chunking(fixture_reads, rna):
    rng = np.random.default_rng(5 + rna)
    n_events = 0
    for k, (meta, raw) in enumerate(fixture_reads[rna]):
        n_events += len(check_signal(raw, meta, rna, rng, f"read {k}")[0])
    assert n_events > 1000


@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna"])
def test_synthetic_signals_any_chunking(fixture_reads, rna):
    meta = fixture_reads[rna][0][0]
    rng = np.random.default_rng(11 + rna)
    with_events = 0
    for k in range(100):
        n = int(rng.integers(30, 600)) if k % 4 == 0 else int(rng.integers(600, 3000))
        want, _ = check_signal(synth_signal(rng, n, meta), meta, rna, rng, f"signal {k} of {n}")
        with_events += len(want) > 0
    assert with_events > 80


@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna"])
def test_nothing_is_withheld(fixture_reads, rna):
    """(d) after N samples the count is the count a 1-sample-chunk run reports at N -- an implementation that waits for finish, or
    for the end of a larger chunk's window, fails here."""
    meta = fixture_reads[rna][0][0]
    rng = np.random.default_rng(3)
    raw = synth_signal(rng, 600, meta)
    per_push, seen, fin = stream(raw, meta, rna, [1] * len(raw))
    ones = np.cumsum([len(e) for e in per_push])
    assert ones[-1] > 20 and len(fin) >= 1
    for chunks in ([600], cut(600, [97]), cut(600, [400, 1, 150])):
        per, seen, _ = stream(raw, meta, rna, chunks)
        for total, n_seen in zip(np.cumsum([len(e) for e in per]), seen):
            assert total == ones[n_seen - 1], (chunks[:3], n_seen)
    # ... and the picker has walked j <= N - w_long and no further: an event is out exactly when its closing peak has fired, which
    # is at the earliest w_long samples after the peak's position (the t-statistics there need that much signal)
    starts = np.concatenate(per_push)["start"]
    first_seen = np.repeat(np.arange(1, len(raw) + 1), [len(e) for e in per_push])
    ends = np.concatenate([starts[1:], S.detect_events(raw, meta, rna)["start"][len(starts):len(starts) + 1]])
    assert (first_seen >= ends + W_LONG[rna]).all()


@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna"])
def test_edge_cases(fixture_reads, rna):
    meta = fixture_reads[rna][0][0]
    rng = np.random.default_rng(8)
    wl = W_LONG[rna]
    for n in (0, 1, wl, 2 * wl - 1, 2 * wl, 2 * wl + 1):  # shorter than, and right at, 2 w_long
        raw = synth_signal(rng, max(n, 1), meta)[:n]
        per_push, _, fin = stream(raw, meta, rna, cut(n, [5]))
        want = S.detect_events(raw, meta, rna) if n else np.zeros(0, S.EVENT_DTYPE)
        same_events(np.concatenate(per_push + [fin]), want, n)
    # no peak at all: no events
    per_push, _, fin = stream(np.full(900, 700, np.int16), meta, rna, cut(900, [64]))
    assert sum(len(e) for e in per_push) == 0 and len(fin) == 0
    # cap too small: the needed count comes back, nothing is consumed, the next call delivers the same events
    L = _lib.load()
    raw = synth_signal(rng, 1500, meta)
    want = S.detect_events(raw, meta, rna)
    EP = C.POINTER(_lib.SfaEvent)
    es = L.sfa_event_stream_create(meta["digitisation"], meta["offset"], meta["range"], int(rna))
    try:
        p = raw.ctypes.data_as(C.POINTER(C.c_int16))
        small = np.zeros(3, S.EVENT_DTYPE)
        need = L.sfa_event_stream_push(es, p, 1000, C.cast(small.ctypes.data, EP), 3)
        assert need > 3
        assert L.sfa_event_stream_push(es, p, 1000, None, 0) == need  # still nothing consumed
        big = np.zeros(need, S.EVENT_DTYPE)
        assert L.sfa_event_stream_push(es, p, 1000, C.cast(big.ctypes.data, EP), need) == need
        same_events(big, want[:need])
        rest = np.zeros(len(want), S.EVENT_DTYPE)
        k = L.sfa_event_stream_push(es, raw[1000:].ctypes.data_as(C.POINTER(C.c_int16)), 500, C.cast(rest.ctypes.data, EP), len(rest))
        assert L.sfa_event_stream_finish(es, None, 0) == len(want) - need - k > 0  # too small as well
        m = L.sfa_event_stream_finish(es, C.cast(rest[k:].ctypes.data, EP), len(rest) - k)
        same_events(np.concatenate([big, rest[:k + m]]), want)
    finally:
        L.sfa_event_stream_destroy(es)


NEW_SYMBOLS = ["sfa_event_stream_create", "sfa_event_stream_push", "sfa_event_stream_finish", "sfa_event_stream_destroy", "sfa_session_raw_config",
               "sfa_session_extend_raw", "sfa_session_events", "sfa_session_raw_bytes"]


def test_symbols_and_null_arguments():
    header = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    L = _lib.load()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\(" % sym, header), sym
        assert sym in _lib.SYMBOLS and getattr(L, sym)
    assert "sfa_session_raw_info_t" in header
    ev = np.zeros(4, S.EVENT_DTYPE)
    evp = C.cast(ev.ctypes.data, C.POINTER(_lib.SfaEvent))
    one = np.ones(4, np.int16)
    rp = one.ctypes.data_as(C.POINTER(C.c_int16))
    es = L.sfa_event_stream_create(8192.0, 6.0, 1467.61, 0)
    assert es
    EINVAL = -1
    assert L.sfa_event_stream_push(None, rp, 4, evp, 4) == EINVAL
    assert L.sfa_event_stream_push(es, None, 4, evp, 4) == EINVAL
    assert L.sfa_event_stream_push(es, rp, 4, None, 4) == EINVAL
    assert L.sfa_event_stream_push(es, rp, -1, evp, 4) == EINVAL
    assert L.sfa_event_stream_finish(None, evp, 4) == EINVAL
    assert L.sfa_event_stream_finish(es, None, 4) == EINVAL
    assert L.sfa_event_stream_push(es, None, 0, None, 0) == 0  # an empty chunk needs neither pointer
    L.sfa_event_stream_destroy(es)
    L.sfa_event_stream_destroy(None)
    # the session entry points refuse null handles before they touch a device
    assert L.sfa_session_raw_config(None, 0, 25, 25) == EINVAL
    assert L.sfa_session_extend_raw(None, None, None, None, None, None, 1, None, None) == EINVAL
    assert L.sfa_session_events(None, 0, 0, None, 0) == EINVAL


def test_session_raw_bytes_formula():
    """per slot: (skip + query) events of 24 bytes, query floats, 592 bytes of detector state"""
    assert C.sizeof(_lib.SfaEvent) == 24
    for n_slots, skip, query in ((1, 0, 25), (512, 50, 2048), (14, 3, 70), (100000, 1000, 100000)):
        assert S.session_raw_bytes(n_slots, skip, query) == n_slots * ((skip + query) * 24 + query * 4 + 592)
    L = _lib.load()
    for bad in ((0, 0, 25), (-1, 0, 25), (4, -1, 25), (4, 0, 0)):
        assert L.sfa_session_raw_bytes(*bad) == -1
    assert L.sfa_session_raw_bytes(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) == -4  # SFA_ERANGE
    with pytest.raises(S.SfaError):
        S.session_raw_bytes(0)
