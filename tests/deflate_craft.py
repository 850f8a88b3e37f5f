"""Crafted zlib streams (RFC 1950 / 1951) for the record decoders: the edges of the format that a compressor never writes and a
decoder must still answer -- largest distances at the first legal position, 15-bit codes, HLIT / HDIST at and beyond their limits,
reserved symbols, empty and one-code distance sets, code-length runs that cross from the literal set into the distance set, empty
stored blocks at every bit phase, every residue of the bit reader's loads.  Plain Python, no GPU.

CASES is a list of (name, stream).  The EXPECTED ANSWER of a case is never written here: it is zlib.decompress(stream), or None
where zlib raises (expected()).  What this file does claim per case (INFO[name]) is its group, whether zlib takes it ("accepted" /
"refused": tests/test_deflate_craft_cpu.py checks the claim and the counts against zlib), how many bytes a decoder may write before
it can know the verdict (`room`: the slot a refused case needs so that it is refused for ITS reason, not for a full slot) and
whether the one-record-per-lane decoder declines it by design (`lane_declines`: bytes behind the stream, see below).

The writer keeps the text its symbols stand for (Deflate.plain) -- only to place symbols ("the first position where this
distance is legal") and to compute the Adler-32 trailer; a slip there makes zlib refuse the stream and the counts fail."""
import collections
import zlib

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
# a complete code-length code over all 19 symbols (13 / 16 + 6 / 32 = 1): HCLEN 19
DEFAULT_CL = [4] * 13 + [5] * 6
# complete codes over the largest alphabets a dynamic block may declare: 286 symbols (226 / 256 + 60 / 512) and 30 (2 / 16 + 28 / 32)
LIT286 = [8] * 226 + [9] * 60
DIST30 = [4] * 2 + [5] * 28
PERIOD = 251  # fill(): the text repeats with this (prime) period, so that a copy from a wrong distance brings other bytes


def canonical(lengths):
    """{symbol: (code, length)} by the rule of RFC 1951 3.2.2.  Over-subscribed sets still get codes (cut to their length when
    written): such a block is refused at its header and what follows is never looked at."""
    count = collections.Counter(l for l in lengths if l)
    code, nxt = 0, {}
    for bits in range(1, 16):
        code = (code + count.get(bits - 1, 0)) << 1
        nxt[bits] = code
    out = {}
    for sym, l in enumerate(lengths):
        if l:
            out[sym] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return out


def lens_of(n, table):
    """code lengths of an alphabet of n symbols from {symbol: length}"""
    out = [0] * n
    for s, l in table.items():
        out[s] = l
    return out


class BitWriter:
    """bits into bytes, least significant bit first (RFC 1951 3.1.1)"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0  # bits waiting in acc = the bit phase of whatever is written next

    def bits(self, value, count):
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """a Huffman code: most significant bit first"""
        for k in range(length - 1, -1, -1):
            self.bits((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.out.append(self.acc & 255)
            self.acc = 0
            self.n = 0

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def pad_ones(self):
        """fill the last byte with ones (seven zeros would be the fixed code's end of block)"""
        if self.n:
            self.bits(255, 8 - self.n)
        return self

    def done(self):
        self.align()
        return bytes(self.out)


class Deflate(BitWriter):
    """a DEFLATE stream symbol by symbol; `plain` is the text the symbols written so far stand for"""

    def __init__(self):
        super().__init__()
        self.plain = bytearray()
        self.lc = self.dc = None

    # ---- blocks ----
    def stored(self, data, final=0, nlen=None, declared=None):
        declared = len(data) if declared is None else declared
        self.bits(final, 1)
        self.bits(0, 2)
        self.align()
        self.raw(declared.to_bytes(2, "little") + ((declared ^ 0xffff) if nlen is None else nlen).to_bytes(2, "little"))
        self.raw(data)
        self.plain += data
        return self

    def fixed(self, final=0):
        self.bits(final, 1)
        self.bits(1, 2)
        self.lc, self.dc = canonical(FIXED_LIT), canonical(FIXED_DIST)
        return self

    def dynamic(self, final, lit_lens, dist_lens, items=None, hlit=None, hdist=None, cl_lens=None, hclen=None):
        """A dynamic block's header from explicit code lengths.  items: the code-length symbols to send as (symbol, extra bits'
        value) -- default: every length as itself, no repeats; hlit / hdist: the symbol counts to DECLARE (default: what is sent);
        cl_lens: the 19 lengths of the code-length code; hclen: how many of them to send (default: up to the last one used)."""
        hlit = len(lit_lens) if hlit is None else hlit
        hdist = len(dist_lens) if hdist is None else hdist
        cl_lens = DEFAULT_CL if cl_lens is None else cl_lens
        if items is None:
            items = [(l, 0) for l in list(lit_lens) + list(dist_lens)]
        if hclen is None:
            hclen = max([4] + [k + 1 for k, s in enumerate(CL_ORDER) if cl_lens[s]])
        self.bits(final, 1)
        self.bits(2, 2)
        self.bits(hlit - 257, 5)
        self.bits(hdist - 1, 5)
        self.bits(hclen - 4, 4)
        for k in range(hclen):
            self.bits(cl_lens[CL_ORDER[k]], 3)
        cc = canonical(cl_lens)
        for sym, extra in items:
            self.code(*cc[sym])
            if sym >= 16:
                self.bits(extra, {16: 2, 17: 3, 18: 7}[sym])
        self.lc, self.dc = canonical(lit_lens), canonical(dist_lens)
        return self

    # ---- symbols ----
    def sym(self, s):
        self.code(*self.lc[s])
        return self

    def lit(self, b):
        self.sym(b)
        self.plain.append(b)
        return self

    def lits(self, data):
        for b in data:
            self.lit(b)
        return self

    def eob(self):
        return self.sym(256)

    def raw_match(self, len_sym, len_extra, dist_sym, dist_extra):
        """length symbol 257 + len_sym and distance symbol dist_sym with these extra bits, whatever they mean"""
        self.sym(257 + len_sym)
        if len_sym < 29:
            self.bits(len_extra, LEN_EXTRA[len_sym])
        self.code(*self.dc[dist_sym])
        if dist_sym < 30:
            self.bits(dist_extra, DIST_EXTRA[dist_sym])
        if len_sym < 29 and dist_sym < 30:
            n, d = LEN_BASE[len_sym] + len_extra, DIST_BASE[dist_sym] + dist_extra
            for _ in range(n):  # (a copy from before the start of the text is what some cases are about: they are refused)
                self.plain.append(self.plain[-d] if d <= len(self.plain) else 0)
        return self

    def match(self, length, dist):
        ls = max(k for k in range(29) if LEN_BASE[k] <= length)
        ds = max(k for k in range(30) if DIST_BASE[k] <= dist)
        return self.raw_match(ls, length - LEN_BASE[ls], ds, dist - DIST_BASE[ds])

    def fill(self, upto):
        """text up to position `upto` in few bytes: PERIOD distinct literals, then copies from PERIOD back (the block's codes must
        hold the literals 0..250, the lengths and distance symbol 15)"""
        while len(self.plain) < upto:
            left = upto - len(self.plain)
            if len(self.plain) < PERIOD:
                self.lit(len(self.plain))
            elif left >= 3:
                self.match(min(left, 258), PERIOD)
            else:
                self.lit(self.plain[-PERIOD])
        return self


def adler32(data):
    a, b = 1, 0
    for x in data:
        a = (a + x) % 65521
        b = (b + a) % 65521
    return (b << 16) | a


def wrap(deflate, plain, cinfo=7, cm=8, flevel=2, fdict=0, fcheck_off=0):
    """the zlib wrapper of RFC 1950: CMF, FLG with FCHECK computed (fcheck_off: then spoiled), the data, Adler-32 big endian"""
    cmf = (cinfo << 4) | cm
    flg = (flevel << 6) | (fdict << 5)
    flg += (31 - (cmf * 256 + flg) % 31) % 31
    flg = (flg + fcheck_off) & 255
    return bytes([cmf, flg]) + bytes(deflate) + adler32(plain).to_bytes(4, "big")


def expected(stream):
    """the reference: zlib's answer, None where it refuses"""
    try:
        return zlib.decompress(stream)
    except zlib.error:
        return None


GROUPS = ("header", "stored", "fixed", "dynamic", "bitreader")
Info = collections.namedtuple("Info", "group claim room lane_declines")
CASES = []
INFO = {}


def add(group, claim, name, stream, room=0, lane_declines=False):
    assert group in GROUPS and claim in ("accepted", "refused") and name not in INFO, name
    CASES.append((name, bytes(stream)))
    INFO[name] = Info(group, claim, room, lane_declines)


def add_deflate(group, claim, name, d, **wrap_args):
    add(group, claim, name, wrap(d.done(), d.plain, **wrap_args), room=len(d.plain))


# ---------------------------------------------------------------- header
def _header_cases():
    text = b"a zlib header in front of a short text, a short text, a short text"
    body = zlib.compress(text, 9)[2:-4]
    for cinfo in range(8):
        add("header", "accepted", f"cinfo_{cinfo}", wrap(body, text, cinfo=cinfo), len(text))
    for cinfo in (8, 15):
        add("header", "refused", f"cinfo_{cinfo}", wrap(body, text, cinfo=cinfo), len(text))
    for cm in (0, 7, 9, 15):
        add("header", "refused", f"cm_{cm}", wrap(body, text, cm=cm), len(text))
    for off in (1, 30):
        add("header", "refused", f"fcheck_plus_{off}", wrap(body, text, fcheck_off=off), len(text))
    add("header", "refused", "fdict", wrap(body, text, fdict=1), len(text))
    for flevel in range(4):
        add("header", "accepted", f"flevel_{flevel}", wrap(body, text, flevel=flevel), len(text))
    whole = wrap(Deflate().fixed(1).eob().done(), b"")  # the shortest zlib stream there is: 8 bytes
    for n in range(6):
        add("header", "refused", f"only_{n}_bytes", whole[:n])


# ---------------------------------------------------------------- stored blocks
def _stored_cases():
    add_deflate("stored", "accepted", "final_len_0", Deflate().stored(b"", 1))
    add_deflate("stored", "accepted", "len_0_between_stored", Deflate().stored(b"one").stored(b"").stored(b"").stored(b"two", 1))
    for k in range(8):  # fixed block of 3 + 9 k + 7 bits: the next block header starts at bit phase (2 + k) mod 8
        d = Deflate().fixed(0).lits(bytes(range(200, 200 + k))).eob()
        phase = d.n
        assert phase == (2 + k) % 8
        d.stored(b"").fixed(0).lits(b"after the empty block").eob().stored(b"").stored(b"stored", 0).fixed(1).lits(b"end").eob()
        add_deflate("stored", "accepted", f"len_0_at_phase_{phase}", d)
    text = bytes((i * 7 + i // 300) & 255 for i in range(900))
    for name, mode in (("sync", zlib.Z_SYNC_FLUSH), ("full", zlib.Z_FULL_FLUSH), ("partial", zlib.Z_PARTIAL_FLUSH)):
        for level in (1, 9):
            co = zlib.compressobj(level)
            s = co.compress(text[:300]) + co.flush(mode) + co.compress(text[300:301]) + co.flush(mode) + co.flush(mode) + co.compress(text[301:]) + co.flush()
            add("stored", "accepted", f"zlib_{name}_flush_level_{level}", s, len(text))
    big = bytes((i * i >> 3) & 255 for i in range(65535))
    add_deflate("stored", "accepted", "len_65535", Deflate().stored(big, 1))
    add_deflate("stored", "accepted", "len_65535_then_fixed", Deflate().stored(big).fixed(1).match(258, 32768).match(3, 32768).eob())
    add_deflate("stored", "refused", "nlen_mismatch", Deflate().stored(b"stored text", 1, nlen=0xfff5))
    add_deflate("stored", "refused", "nlen_equals_len", Deflate().stored(b"stored text", 1, nlen=11))
    add_deflate("stored", "refused", "len_past_the_end", Deflate().stored(b"ten bytes.", 1, declared=100))
    add_deflate("stored", "refused", "len_65535_past_the_end", Deflate().stored(b"ten bytes.", 1, declared=65535))
    add_deflate("stored", "refused", "len_reaches_into_the_trailer", Deflate().stored(b"ten bytes.", 1, declared=12))
    d = Deflate()
    d.bits(1, 1)
    d.bits(3, 2)  # block type 3
    add_deflate("stored", "refused", "block_type_3", d)


# ---------------------------------------------------------------- fixed code
def _fixed_cases():
    for ls in range(29):  # every length symbol with its smallest and its largest extra bits (284 + 31 = 258, and 285)
        d = Deflate().fixed(1).lits(b"xyz").raw_match(ls, 0, 2, 0).lit(33).raw_match(ls, (1 << LEN_EXTRA[ls]) - 1, 3, 0).eob()
        add_deflate("fixed", "accepted", f"length_symbol_{257 + ls}", d)
    for ds in range(30):  # every distance symbol, at the first position where it is legal and one position earlier
        for which, extra in (("min", 0), ("max", (1 << DIST_EXTRA[ds]) - 1)):
            if which == "max" and DIST_EXTRA[ds] == 0:
                continue
            dist = DIST_BASE[ds] + extra
            for op, claim in ((dist, "accepted"), (dist - 1, "refused")):
                d = Deflate().fixed(1).fill(op).raw_match(1, 0, ds, extra).lit(65).eob()
                assert len(d.plain) == op + 5
                add_deflate("fixed", claim, f"distance_symbol_{ds}_{which}_at_{op}", d)
    assert DIST_BASE[29] + (1 << 13) - 1 == 32768
    for dist in (1, 2, 3):  # overlapping copies of the longest length
        add_deflate("fixed", "accepted", f"overlap_258_at_distance_{dist}", Deflate().fixed(1).lits(b"pqr"[:dist]).match(258, dist).match(258, dist).lit(0).eob())
    for s in (286, 287):
        add_deflate("fixed", "refused", f"literal_length_symbol_{s}", Deflate().fixed(1).lits(b"abc").sym(s).eob())
    for ds in (30, 31):
        add_deflate("fixed", "refused", f"distance_symbol_{ds}", Deflate().fixed(1).lits(b"abc").raw_match(0, 0, ds, 0).eob())
    add_deflate("fixed", "refused", "no_end_of_block", Deflate().fixed(1).lits(b"the block never ends").pad_ones())
    add_deflate("fixed", "refused", "no_end_of_block_after_a_match", Deflate().fixed(1).lits(b"ab").match(20, 2).pad_ones())
    add_deflate("fixed", "refused", "not_final_and_nothing_follows", Deflate().fixed(0).lits(b"abc").eob())


# ---------------------------------------------------------------- dynamic code
def _dynamic_cases():
    small = lens_of(257, {97: 1, 98: 2, 256: 2})  # a, b, end of block
    ab200 = lens_of(284, {97: 1, 98: 2, 256: 3, 283: 3})  # ... and the lengths 195 .. 226
    # HLIT / HDIST at and beyond their limits
    add_deflate("dynamic", "accepted", "hlit_29_hdist_29", Deflate().dynamic(1, LIT286, DIST30).fill(300).raw_match(28, 0, 0, 0).raw_match(27, 31, 15, 63).raw_match(0, 0, 1, 0).eob())
    for n in (287, 288):
        add_deflate("dynamic", "refused", f"hlit_{n - 257}", Deflate().dynamic(1, LIT286 + [0] * (n - 286), [1, 1]).lits(b"abc").eob())
    for n in (31, 32):
        add_deflate("dynamic", "refused", f"hdist_{n - 1}", Deflate().dynamic(1, small, DIST30 + [0] * (n - 30)).lits(b"abab").eob())
    # HCLEN: with 4 only 16, 17, 18 and 0 have codes -- every length is 0 and there is no end-of-block code; 5 adds the 8
    add_deflate("dynamic", "refused", "hclen_4", Deflate().dynamic(1, [0] * 257, [0], items=[(18, 127), (18, 109)], cl_lens=lens_of(19, {16: 2, 17: 2, 18: 2, 0: 2})))
    cl5 = lens_of(19, {8: 1, 0: 2, 16: 3, 17: 4, 18: 4})
    d = Deflate().dynamic(1, [0] + [8] * 256, [0], cl_lens=cl5, items=[(0, 0), (8, 0)] + [(16, 3)] * 42 + [(16, 0), (0, 0)])
    assert 1 + 1 + 42 * 6 + 3 == 257 and max(k + 1 for k, s in enumerate(CL_ORDER) if cl5[s]) == 5
    add_deflate("dynamic", "accepted", "hclen_5", d.lits(b"\x01\xff codes of eight bits \x80").eob())
    add_deflate("dynamic", "accepted", "hclen_19", Deflate().dynamic(1, ab200, [1, 1]).lits(b"abba").match(200, 2).eob())
    add_deflate("dynamic", "refused", "code_length_code_incomplete", Deflate().dynamic(1, [0] + [8] * 256, [0], cl_lens=lens_of(19, {0: 1, 8: 2})).lits(b"\x01\x02").eob())
    add_deflate("dynamic", "refused", "code_length_code_one_code", Deflate().dynamic(1, [8] * 257, [8], cl_lens=lens_of(19, {8: 1})).lits(b"\x01\x02").eob())
    add_deflate("dynamic", "refused", "code_length_code_oversubscribed", Deflate().dynamic(1, [0] + [8] * 256, [0], cl_lens=lens_of(19, {0: 1, 8: 1, 7: 1})).lits(b"\x01\x02").eob())
    add_deflate("dynamic", "refused", "code_length_code_empty", Deflate().dynamic(1, small, [0], items=[], cl_lens=[0] * 19))
    # the code-length symbols
    add_deflate("dynamic", "refused", "symbol_16_first", Deflate().dynamic(1, small, [0], items=[(16, 0)] + [(l, 0) for l in small[3:]] + [(0, 0)]).lits(b"ab").eob())
    add_deflate("dynamic", "refused", "repeat_past_the_end", Deflate().dynamic(1, small, [0], items=[(l, 0) for l in small] + [(17, 0)]).lits(b"ab").eob())
    add_deflate("dynamic", "refused", "repeat_18_past_the_end", Deflate().dynamic(1, small, [0], items=[(l, 0) for l in small[:250]] + [(18, 127)]).lits(b"ab").eob())
    # ... crossing from the literal/length lengths into the distance lengths: 16 (copies the 3 of symbol 256), 17, 18 (zeros);
    # the matches behind them show that every length landed on its symbol
    lit = lens_of(258, {97: 1, 255: 2, 256: 3, 257: 3})
    d = Deflate().dynamic(1, lit, [3, 3, 2, 1], items=[(l, 0) for l in lit[:257]] + [(16, 0), (2, 0), (1, 0)])
    add_deflate("dynamic", "accepted", "repeat_16_crosses_into_distances", d.lits(b"aa\xffa").match(3, 1).match(3, 2).match(3, 3).match(3, 4).eob())
    lit = lens_of(261, {97: 1, 255: 2, 256: 3, 257: 3})
    d = Deflate().dynamic(1, lit, [0, 0, 1, 1], items=[(l, 0) for l in lit[:258]] + [(17, 5 - 3), (1, 0), (1, 0)])
    add_deflate("dynamic", "accepted", "repeat_17_crosses_into_distances", d.lits(b"a\xffaa").match(3, 3).match(3, 4).eob())
    lit = lens_of(281, {97: 1, 255: 2, 256: 3, 257: 3})
    d = Deflate().dynamic(1, lit, [0] * 5 + [1, 1], items=[(l, 0) for l in lit[:258]] + [(18, 28 - 11), (1, 0), (1, 0)])
    add_deflate("dynamic", "accepted", "repeat_18_crosses_into_distances", d.lits(b"a\xffaa\xffaaa\xff").match(3, 7).match(3, 9).eob())
    # the literal/length code
    add_deflate("dynamic", "refused", "no_code_for_256", Deflate().dynamic(1, lens_of(257, {97: 1, 98: 1}), [0]).lits(b"abab"))
    steps = {65 + k: k + 1 for k in range(14)}  # 'A' 1 bit, 'B' 2 ... 'N' 14, 'O' and end of block 15: a literal at every length
    steps.update({79: 15, 256: 15})
    d = Deflate().dynamic(1, lens_of(257, steps), [0]).lits(b"ABCDEFGHIJKLMNO" + b"ONMLKJIHGFEDCBA" + b"IJIJJIAJAIOAOJOI" * 3).eob()
    add_deflate("dynamic", "accepted", "lengths_1_to_15_literals", d)
    steps = {65 + k: k + 1 for k in range(8)}  # ... and with length symbols on both sides of a 9-bit first-level table
    steps.update({257: 9, 258: 10, 73: 11, 74: 12, 264: 13, 75: 14, 285: 15, 256: 15})
    d = Deflate().dynamic(1, lens_of(286, steps), [1, 1]).lits(b"ABCDEFGHIJK").match(3, 1).match(4, 2).match(10, 2).match(258, 1).match(3, 2).lits(b"HIJKA").match(4, 1).eob()
    add_deflate("dynamic", "accepted", "lengths_1_to_15_with_length_symbols", d)
    add_deflate("dynamic", "refused", "literal_code_incomplete", Deflate().dynamic(1, lens_of(257, {97: 2, 98: 2, 256: 2}), [0]).lits(b"abab").eob())
    add_deflate("dynamic", "refused", "literal_code_one_code_of_2_bits", Deflate().dynamic(1, lens_of(257, {256: 2}), [0]).eob())
    add_deflate("dynamic", "refused", "literal_code_oversubscribed", Deflate().dynamic(1, lens_of(257, {97: 1, 98: 1, 256: 1}), [0]).lits(b"ab").eob())
    add_deflate("dynamic", "accepted", "literal_code_is_one_bit_for_256", Deflate().dynamic(1, lens_of(257, {256: 1}), [0]).eob())
    d = Deflate().dynamic(1, lens_of(257, {256: 1}), [0])
    d.bits(1, 1)  # the other, unassigned pattern
    add_deflate("dynamic", "refused", "literal_code_is_one_bit_other_pattern", d)
    # distance sets
    withlen = lens_of(258, {97: 1, 256: 2, 257: 2})  # a, end of block, length 3
    add_deflate("dynamic", "accepted", "distances_empty_literals_only", Deflate().dynamic(1, withlen, [0]).lits(b"aaaa").eob())
    add_deflate("dynamic", "accepted", "distances_empty_30_declared", Deflate().dynamic(1, withlen, [0] * 30).lits(b"aaaa").eob())
    d = Deflate().dynamic(1, withlen, [0]).lits(b"aaaa").sym(257)
    d.bits(0, 1)
    add_deflate("dynamic", "refused", "distances_empty_length_used", d.eob())
    add_deflate("dynamic", "accepted", "distances_one_code_of_1_bit", Deflate().dynamic(1, withlen, [1]).lits(b"aa").match(3, 1).eob())
    add_deflate("dynamic", "accepted", "distances_one_code_of_1_bit_symbol_3", Deflate().dynamic(1, withlen, [0, 0, 0, 1]).lits(b"aaaa").match(3, 4).eob())
    d = Deflate().dynamic(1, withlen, [1]).lits(b"aa").sym(257)
    d.bits(1, 1)  # the other, unassigned pattern
    add_deflate("dynamic", "refused", "distances_one_code_of_1_bit_other_pattern", d.eob())
    add_deflate("dynamic", "refused", "distances_one_code_of_2_bits", Deflate().dynamic(1, withlen, [2]).lits(b"aa").match(3, 1).eob())
    add_deflate("dynamic", "refused", "distances_two_codes_of_2_bits", Deflate().dynamic(1, withlen, [2, 2]).lits(b"aa").match(3, 1).eob())
    add_deflate("dynamic", "refused", "distances_oversubscribed", Deflate().dynamic(1, withlen, [1, 1, 1]).lits(b"aa").match(3, 1).eob())
    add_deflate("dynamic", "refused", "distances_oversubscribed_at_15_bits", Deflate().dynamic(1, withlen, list(range(1, 16)) + [15, 15]).lits(b"aa").match(3, 1).eob())
    # complete with 30 symbols and lengths up to 15: 1 .. 10 on the far distances, 14 and 15 bits on the near ones, which the text reaches
    deep = [15] * 8 + [14] * 12 + list(range(10, 0, -1))
    d = Deflate().dynamic(1, LIT286, deep)
    d.fill(PERIOD)
    for ds in range(20):
        d.fill(DIST_BASE[ds] + (1 << DIST_EXTRA[ds]) - 1).raw_match(ds % 8, 0, ds, (1 << DIST_EXTRA[ds]) - 1).raw_match(1, 0, ds, 0)
    add_deflate("dynamic", "accepted", "distances_30_codes_up_to_15_bits", d.eob())
    d = Deflate().dynamic(1, LIT286, deep).fill(24577).raw_match(0, 0, 29, 0).fill(40000).raw_match(5, 0, 29, 8191).raw_match(28, 0, 0, 0).eob()
    add_deflate("dynamic", "accepted", "distances_30_codes_symbol_29_in_1_bit", d)
    # several blocks with their own codes, a stored one between them
    d = Deflate().dynamic(0, LIT286, DIST30).fill(400).eob().stored(b"between").dynamic(0, ab200, [1, 1]).lits(b"abba").match(200, 2).eob().fixed(0).match(258, 411).eob()
    add_deflate("dynamic", "accepted", "blocks_of_every_type", d.dynamic(1, lens_of(257, {256: 1}), [0]).eob())


# ---------------------------------------------------------------- the bit reader
def _bitreader_cases():
    """Sound streams of every total length from 8 bytes -- no zlib stream is shorter: two bytes of header, a final fixed block
    with nothing but its end (10 bits), four of Adler-32 -- to 48: every residue of the reader's 4-byte words and 16-byte loads.
    (Lengths 6 and 7 exist as cuts of the 8- and 9-byte streams.)  Each cut short by 1 .. 5 bytes; some with bytes behind them."""
    sound = []
    for k in range(41):  # 2 + ceil((10 + 8 k) / 8) + 4 = 8 + k bytes
        d = Deflate().fixed(1).lits(bytes((37 * j + k) % 144 for j in range(k))).eob()
        sound.append((f"fixed_total_{8 + k}", wrap(d.done(), d.plain), len(d.plain)))
        assert len(sound[-1][1]) == 8 + k
    for k in range(38):  # 2 + 5 + k + 4 = 11 + k bytes
        d = Deflate().stored(bytes((91 * j + k) & 255 for j in range(k)), 1)
        sound.append((f"stored_total_{11 + k}", wrap(d.done(), d.plain), len(d.plain)))
        assert len(sound[-1][1]) == 11 + k
    for name, s, room in sound:
        add("bitreader", "accepted", name, s, room)
        for cut in range(1, 6):
            add("bitreader", "refused", f"{name}_cut_{cut}", s[:-cut], room)
    text = b"bytes behind a stream, behind a stream, behind a stream: zlib leaves them alone"
    co = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    d = Deflate().stored(text[:30]).stored(text[30:], 1)
    for name, s in (("dynamic", zlib.compress(text * 3, 9)), ("fixed", co.compress(text) + co.flush()), ("stored", wrap(d.done(), d.plain))):
        for k in range(1, 8):
            # zlib (and the host decoder) stop at the end of the stream; the lane decoder takes the Adler-32 from the END of the
            # record, as the record's framing gives it, so it declines
            add("bitreader", "accepted", f"{name}_and_{k}_trailing_bytes", s + bytes((0x5a + 41 * j) & 255 for j in range(k)), 3 * len(text), lane_declines=True)


_header_cases()
_stored_cases()
_fixed_cases()
_dynamic_cases()
_bitreader_cases()


def flat_file(path, cases=None):
    """the cases as tests/c/device_inflate_host.cpp reads them: u32 count, then per case u32 kind (1 sound, 0 refused, 2 sound for
    zlib but declined by the lane decoder by design), u32 plain bytes, u32 stream bytes, plain, stream"""
    import struct
    cases = CASES if cases is None else cases
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for name, s in cases:
            want = expected(s)
            kind = 0 if want is None else 2 if INFO[name].lane_declines else 1
            want = want or b""
            f.write(struct.pack("<III", kind, len(want), len(s)) + want + s)
