"""The crafted zlib streams of tests/deflate_craft.py, without a GPU: the table is what it claims (checked against zlib alone,
by counts), the host reader's decoder (sigfish_amd/csrc/host/inflate.cpp through sfa_inflate_zlib) gives zlib's bytes or declines,
and which sound streams the device's lane decoder (blow5_kernels.hpp: inflate_zlib_lane) may decline.  The lane decoder itself runs
on these cases as a stand-alone host program under ASan + UBSan in tests/test_c_host.py (tests/c/device_inflate_host.cpp)."""
import collections
import ctypes as C

import numpy as np

from sigfish_amd import _lib
from tests import deflate_craft as D

# (group, claim) -> cases, counted by hand from the lists of deflate_craft.py: a slip of the bit writer that turns sound streams
# into refused ones (or the other way round) changes these
COUNTS = {
    ("header", "accepted"): 8 + 4,               # CINFO 0..7, FLEVEL 0..3
    ("header", "refused"): 2 + 4 + 2 + 1 + 6,    # CINFO 8 and 15, CM, FCHECK, FDICT, 0..5 bytes
    ("stored", "accepted"): 2 + 8 + 6 + 2,       # LEN 0, LEN 0 at every bit phase, zlib's flushes, LEN 65535
    ("stored", "refused"): 2 + 3 + 1,            # NLEN, LEN past the end, block type 3
    ("fixed", "accepted"): 29 + 30 + 26 + 3,     # length symbols, distance symbols (min; max where there are extra bits), overlaps
    ("fixed", "refused"): 30 + 26 + 2 + 2 + 3,   # each distance one position early, symbols 286 / 287 / 30 / 31, no end of block
    ("dynamic", "accepted"): 16,
    ("dynamic", "refused"): 23,
    ("bitreader", "accepted"): 41 + 38 + 21,     # totals 8..48 (fixed), 11..48 (stored), 1..7 trailing bytes on three streams
    ("bitreader", "refused"): 5 * (41 + 38),     # each cut by 1..5 bytes
}
# sound streams a decoder may decline, by name; everything else sound must DECODE (a decline is a silent fall-back to the slow path)
HOST_MAY_DECLINE = set()  # (FDICT is refused by zlib.decompress as well; bytes behind the stream are ignored as zlib ignores them)
LANE_MAY_DECLINE = {n for n, i in D.INFO.items() if i.lane_declines}  # bytes behind the stream: the Adler-32 is taken from the record's end


def test_the_table_is_what_it_claims():
    counts = collections.Counter()
    for name, stream in D.CASES:
        info = D.INFO[name]
        want = D.expected(stream)
        assert (want is not None) == (info.claim == "accepted"), name
        if want is not None:
            assert len(want) <= 70 * 1024, name
            assert info.lane_declines or len(want) == info.room, name  # (the writer's own book-keeping agrees with zlib)
        counts[(info.group, info.claim)] += 1
    assert dict(counts) == COUNTS
    for g in D.GROUPS:
        assert counts[(g, "accepted")] >= 1 and counts[(g, "refused")] >= 1
    sizes = [len(D.expected(s) or b"") for _, s in D.CASES]
    assert sum(n <= 1024 for n in sizes) > 0.9 * len(sizes)
    assert len(LANE_MAY_DECLINE) == 21 and all("trailing_bytes" in n for n in LANE_MAY_DECLINE)
    names = dict(D.CASES)
    # the cases other tests name
    for n in ("cinfo_8", "cinfo_15", "fcheck_plus_1", "distance_symbol_29_max_at_32768", "distance_symbol_29_max_at_32767", "len_65535"):
        assert n in names, n
    assert D.INFO["distance_symbol_29_max_at_32768"].claim == "accepted" and D.INFO["distance_symbol_29_max_at_32767"].claim == "refused"


def test_the_bit_writer_against_zlibs_own_streams():
    """the writer's fixed code, bit order and Adler-32 give, for a text without repeats, the very bytes zlib's Z_FIXED writes"""
    import zlib
    text = bytes(range(40, 140))  # (8-bit codes only: with the 9-bit ones zlib would rather store these bytes)
    co = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    d = D.Deflate().fixed(1).lits(text).eob()
    assert D.wrap(d.done(), d.plain, flevel=0) == co.compress(text) + co.flush()
    assert D.adler32(text * 40) == zlib.adler32(text * 40)


def test_host_decoder_gives_zlibs_bytes_or_declines():
    L = _lib.load()
    out = np.zeros(1 << 17, np.uint8)
    wrong, taken, declined = [], 0, []
    for name, stream in D.CASES:
        want = D.expected(stream)
        out[:] = 0xa5
        r = L.sfa_inflate_zlib(stream, len(stream), out.ctypes.data_as(C.c_void_p), out.size)
        if r >= 0:
            taken += 1
            if want is None or out[:r].tobytes() != want:  # other bytes, or accepted what zlib refuses
                wrong.append((name, r))
        elif want is not None and name not in HOST_MAY_DECLINE:
            declined.append(name)
    assert not wrong, wrong[:10]
    assert not declined, declined[:10]
    assert taken == sum(1 for _, s in D.CASES if D.expected(s) is not None)
