"""Session event maps, the parts that need no GPU: the three symbols (header, library, ctypes signatures), the memory arithmetic
of sfa_session_keep_bytes, the session flag bits that stay refused, format_sam_line against sam_row_from_map, and the refusal of
replay(sam=True) on a session without start columns."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib, realtime
from tests.util import ROOT

EINVAL, ERANGE = -1, -4
NEW = ("sfa_session_event_maps", "sfa_session_keep_events", "sfa_session_keep_bytes")


def test_error_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    assert int(re.search(r"SFA_EINVAL = (-?\d+)", text).group(1)) == EINVAL
    assert int(re.search(r"SFA_ERANGE = (-?\d+)", text).group(1)) == ERANGE


def test_symbols_in_header_library_and_loader():
    text = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    L = _lib.load()
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, text), sym
        assert sym in _lib.SYMBOLS
        getattr(L, sym)
    vp = C.c_void_p
    assert L.sfa_session_event_maps.argtypes == [vp, vp, _lib.i32p, C.c_int32, _lib.i64p, _lib.i32p, _lib.i32p]
    assert L.sfa_session_keep_events.argtypes == [vp, C.c_int32]
    assert L.sfa_session_keep_bytes.argtypes == [C.c_int32, C.c_int32] and L.sfa_session_keep_bytes.restype == C.c_int64
    # the header's prototypes, argument by argument
    proto = re.search(r"int sfa_session_event_maps\(([^;]*)\);", text).group(1)
    assert [a.strip().rsplit(" ", 1)[0] for a in proto.replace("\n", " ").split(",")] == \
        ["sfa_session_t", "const sfa_result_t", "const int32_t", "int32_t", "const int64_t", "int32_t", "int32_t"]
    assert re.search(r"int sfa_session_keep_events\(sfa_session_t \*s, int32_t max_events\);", text)
    assert re.search(r"int64_t sfa_session_keep_bytes\(int32_t n_slots, int32_t max_events\);", text)


def test_keep_bytes():
    L = _lib.load()
    for n_slots, max_events in ((1, 1), (16, 300), (512, 2048), (7, 12345), (2 ** 31 - 1, 1), (1, 2 ** 31 - 1), (2 ** 20, 2 ** 31 - 1)):
        assert L.sfa_session_keep_bytes(n_slots, max_events) == n_slots * max_events * 4
        assert S.session_keep_bytes(n_slots, max_events) == n_slots * max_events * 4
    for bad in ((0, 10), (-1, 10), (10, 0), (10, -5)):
        assert L.sfa_session_keep_bytes(*bad) == EINVAL
        with pytest.raises(S.SfaError):
            S.session_keep_bytes(*bad)
    # a product beyond 2^63: (2^31 - 1)^2 x 4 is just below 2^64
    big = 2 ** 31 - 1
    assert big * big * 4 >= 2 ** 63
    assert L.sfa_session_keep_bytes(big, big) == ERANGE
    assert L.sfa_session_keep_bytes(2 ** 30, 2 ** 31 - 1) == 2 ** 63 - 2 ** 32  # the largest products still fit ...
    assert L.sfa_session_keep_bytes(2 ** 30 + 1, 2 ** 31 - 1) == ERANGE        # ... and the next one does not
    with pytest.raises(S.SfaError):
        S.session_keep_bytes(big, big)
    # the same codes as sfa_session_raw_bytes, for the same mistakes
    assert L.sfa_session_raw_bytes(0, 0, 10) == EINVAL and L.sfa_session_raw_bytes(10, 0, 0) == EINVAL
    assert L.sfa_session_raw_bytes(big, big, big) == ERANGE


def test_unassigned_session_flag_bits_stay_refused():
    L = _lib.load()
    assert L.sfa_session_bytes(1000, 4, 0) == 1000 * 4 * 8
    assert L.sfa_session_bytes(1000, 4, 2) < 0
    assert L.sfa_session_bytes(1000, 4, 8) < 0


def _events(n):
    ev = np.zeros(n, S.EVENT_DTYPE)
    ev["length"] = 5 + np.arange(n) % 4
    ev["start"] = np.concatenate([[0], np.cumsum(ev["length"][:-1])]).astype(np.uint64) + 17
    ev["mean"] = 90
    return ev


def _row(rid, st, end, strand="+", mapq=33):
    r = np.zeros(1, S.RESULT_DTYPE)[0]
    r["rid"], r["pos_st"], r["pos_end"], r["score"], r["score2"], r["strand"], r["mapq"], r["valid"] = rid, st, end, 1.5, 2.5, ord(strand), mapq, 1
    return r


def test_format_sam_line_is_sam_row_from_map_plus_tags():
    ev = _events(40)
    info = np.zeros(1, S.SESSION_RAW_INFO_DTYPE)[0]
    info["q_events"], info["n_samples"] = 12, 4321
    names = ["c0", "c1"]
    # six columns: plain, two events, a blank one, then singles; query events 0..11 inside events [3, 15)
    pairs = np.array([[0, 1], [2, 4], [-1, -1], [5, 5], [6, 9], [10, 11]], np.int32)
    for flag, strand in ((0, "+"), (0, "-"), (S.RNA, "+")):
        row = _row(1, 100, 105, strand)
        for secondary in (False, True):
            base = S.sam_row_from_map(row, "read-7", "c1", ev, 3, 15, pairs, flag, secondary)
            assert base.endswith("\n") and base.startswith("read-7\t")
            got = realtime.format_sam_line("read-7", names, row, info, "E", ev, 3, 15, pairs, flag, secondary)
            assert got == base[:-1] + "\tne:i:12\tns:i:4321\tdc:A:E\n"
            assert int(got.split("\t")[1]) & 256 == (256 if secondary else 0)
    # the automatic start's two tags follow, as in format_line
    auto = np.zeros(1, S.SESSION_AUTO_DTYPE)[0]
    auto["skip"], auto["status"] = 3, S.AUTO_RESOLVED
    row = _row(0, 7, 12)
    got = realtime.format_sam_line("r", names, row, info, "F", ev, 3, 15, pairs, 0, auto=auto)
    assert got == S.sam_row_from_map(row, "r", "c0", ev, 3, 15, pairs, 0)[:-1] + "\tne:i:12\tns:i:4321\tdc:A:F\tqs:i:3\tas:A:P\n"
    # no record: a row that is not mapped, a row without a map, an RNA map whose last column is blank
    unmapped = row.copy()
    unmapped["valid"] = 0
    assert realtime.format_sam_line("r", names, unmapped, info, "R", ev, 3, 15, pairs, 0) == ""
    assert realtime.format_sam_line("r", names, row, info, "R", ev, 3, 15, None, 0) == ""
    blank_last = pairs.copy()
    blank_last[-1] = (-1, -1)
    assert realtime.format_sam_line("r", names, row, info, "R", ev, 3, 15, blank_last, S.RNA) == ""
    assert realtime.format_sam_line("r", names, row, info, "R", ev, 3, 15, blank_last, 0) != ""
    # format_sam: the primary, then the valid candidates as secondaries; refused rows are counted
    cand = np.zeros(4, S.RESULT_DTYPE)
    cand[0], cand[1] = _row(0, 20, 25, "-", 0), _row(1, 30, 35, "+", 0)
    sam = dict(events=ev, qstart=3, qend=15, map=pairs, cand_maps=[pairs, blank_last, None, None])
    text, refused = realtime.format_sam("r", names, row, info, "E", sam, S.RNA, cand=cand)
    assert refused == 1 and text == (realtime.format_sam_line("r", names, row, info, "E", ev, 3, 15, pairs, S.RNA)
                                     + realtime.format_sam_line("r", names, cand[0], info, "E", ev, 3, 15, pairs, S.RNA, True))
    assert realtime.format_sam("r", names, unmapped, info, "R", sam, 0) == ("", 0)


def test_replay_sam_refused_on_a_session_without_starts():
    class NoStarts:
        starts = False

        def __getattr__(self, name):  # any call at all is a failure of the test
            raise AssertionError(f"replay called session.{name} before refusing")

    reads = [("r0", dict(digitisation=8192.0, offset=6.0, range=1467.61), np.zeros(100, np.int16))]
    with pytest.raises(S.SfaError, match="starts=False"):
        next(realtime.replay(None, reads, 1, 50, 3, 25, 70, 30, 5, session=NoStarts(), sam=True))
