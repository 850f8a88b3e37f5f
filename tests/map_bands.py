"""The bands tests/test_maps_model_cpu.py and tests/test_event_maps_bands_gpu.py put in front of the event-map routines, as data:
result rows the caller writes -- any band on any resident query -- instead of rows the aligner just produced, whose band is
always the sDTW optimum of its query (a width near the query's length, similar widths in one wave, a complete map).

A case is a flag, contigs, query lengths and a list of Band(read, contig, strand, col_st, m, planted): band columns
[col_st, col_st + m) of the strand's array of `contig`, for the query of `read`.  A PLANTED band is itself a valid alignment of
its query x (in DP order: reversed for RNA without --invert): y[col_st + j] = x[idx[j]] with idx[0] = 0 and idx[1:] a sorted
draw from 1 .. qlen - 1 that holds every row once m >= qlen.  A random band on random data almost never has a complete map; a
planted one nearly always has.  Unplanted bands stay random: the rows whose map must be empty.  Two variants of the values:
quantised (integers(-6, 7) / 4: ties everywhere) and normal (plus noise of sd 0.05 on the planted columns).  Seeds are fixed;
build() is cached, so the CPU and the GPU file, and every test in them, see the same arrays.

The band-fill classes (sfa_plan.hpp, kClassShapes): a query of up to R * L events runs R rows per lane on L lanes, 64 / L rows
per wave, four waves per block; a wave runs max(m) + L - 1 steps, unrolled by 4 with a prefetch one group ahead."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from tests import maps_model as M

RNA, DTW, INV, REF = 0x001, 0x002, 0x004, 0x010  # opt.flag bits (src/sigfish.h:30-39)
MAX_QUERY = 2048
CLASSES = ((4, 16, 64), (8, 16, 128), (16, 16, 256), (32, 16, 512), (32, 32, 1024), (32, 64, 2048))  # (R, L, most events)
EDGE_QLENS = (1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2047, 2048)
SPIKE = 4194304.0  # 2^22: a float32 sum that has passed it counts in steps of 0.5
HUGE = 3e38         # ... and one that has passed this takes up nothing any more (it stays finite)

Band = namedtuple("Band", "read contig strand col_st m planted")
Case = namedtuple("Case", "name flag lens offs qlens bands strips spikes")  # spikes: [(contig, strand, column, level)]
Built = namedtuple("Built", "names seq_lengths ref_lengths st_offset forward reverse q q_off rows read_of_row")


def shape_of(qlen):
    """(R, L) of the class a query of qlen events runs in; beyond 2048 events the strips' 32 x 64"""
    return next(((R, L) for R, L, most in CLASSES if qlen <= most), (32, 64))


def per_block(L):
    return 4 * (64 // L)


def edge_widths(qlen):
    """the band widths every edge query length gets: around 1, around the lanes of the class, and around the query"""
    L = shape_of(qlen)[1]
    return sorted({1, 2, 3, 4, 5, 7, 8, L - 1, L, L + 1, max(qlen // 2, 1), qlen, min(2 * qlen, 2100)})


def row_bytes(qlen, m):
    """scratch a row takes (sfa_plan.hpp, map_row_bytes): (m + L - 1) steps x L lanes x words x 4"""
    R, L = shape_of(qlen)
    return (m + L - 1) * L * (2 if R == 32 else 1) * 4


class _Layout:
    """bands laid out one behind the other on the strands of the contigs, so that no planted band overwrites another"""

    def __init__(self, strands):
        self.strands, self.lens, self.offs, self.bands, self.cur = strands, [], [], [], None

    def contig(self, off=0):
        self.close()
        self.cur = {s: 0 for s in self.strands}
        self.off = off
        return len(self.lens)

    def put(self, read, m, strand="+", gap=2, planted=True):
        """a band of m columns `gap` columns behind the last one of its strand -> its first column"""
        assert gap >= 0 and m >= 1
        st = self.cur[strand] + gap
        self.bands.append(Band(read, len(self.lens), strand, st, m, planted))
        self.cur[strand] = st + m
        return st

    def put_ending(self, read, m, strand, end, planted=True):
        """a band of m columns whose last column is end - 1; it may not reach back into the bands its strand holds"""
        assert end - m >= self.cur[strand], (strand, end, m, self.cur[strand])
        return self.put(read, m, strand, gap=end - m - self.cur[strand], planted=planted)

    def level(self):
        """the next band of either strand begins behind everything laid out so far -> that column"""
        top = max(self.cur.values())
        self.cur = {s: top for s in self.cur}
        return top

    def close(self, tail=0):
        if self.cur is not None:
            self.lens.append(max(self.cur.values()) + tail)
            self.offs.append(self.off)
            self.cur = None


def _case(name, flag, lay, qlens, strips=False, spikes=()):
    lay.close()
    return Case(name, flag, tuple(lay.lens), tuple(lay.offs), tuple(qlens), tuple(lay.bands), strips, tuple(spikes))


def _edges(ci):
    """every query length of class ci at every width of edge_widths, one band behind the other on one contig"""
    lo = CLASSES[ci - 1][2] if ci else 0
    qlens = [q for q in EDGE_QLENS if lo < q <= CLASSES[ci][2]]
    lay = _Layout("+")
    lay.contig()
    for r, q in enumerate(qlens):
        for m in edge_widths(q):
            lay.put(r, m)
    lay.close(tail=3)
    return _case(f"edges_r{CLASSES[ci][0]}_l{CLASSES[ci][1]}", 0, lay, qlens)


MIXED_QLENS = (60, 300, 700, 1500)  # reads 0 .. 3: 4 x 16, 32 x 16, 32 x 32, 32 x 64
MIXED_WIDE = ((70, 64, 90), (330, 280, 401), (760, 650, 900), (1700, 1400, 1650))


def _mixed(name, counts):
    """rows of very different widths side by side in one wave: slots of m = 1, wide, 3, wide (L = 16), 1, wide (L = 32), and waves
    of one row each with widths 1, wide, 3, wide (L = 64); counts[L] rows per class -- 1, per_block - 1, per_block, per_block + 1"""
    lay = _Layout("+-")
    lay.contig()
    for r, q in enumerate(MIXED_QLENS):
        L = shape_of(q)[1]
        for k in range(counts[L]):
            narrow = 1 if L == 32 else (1, 3)[(k // 2) % 2]
            # (a class of one row: a wide one.  The widest row of a case, 1700 columns, is alone in its width: L = 64 has at most
            # five rows, two of them wide -- the two-budget test counts on it)
            m = narrow if k % 2 == 0 and counts[L] > 1 else MIXED_WIDE[r][(k // 2) % 3]
            lay.put(r, m, "+-"[k % 3 == 2])
    lay.close(tail=5)
    return _case(name, 0, lay, MIXED_QLENS)


def _array_edges():
    qlens = (50, 5, 25, 100, 300, 600)
    lay = _Layout("+-")
    lay.contig()            # contig 0: as short as its band, on both strands
    lay.put(0, 64, "+", gap=0), lay.put(0, 64, "-", gap=0)
    lay.contig()            # contig 1: seven columns
    lay.put(1, 7, "+", gap=0), lay.put(1, 7, "-", gap=0)
    lay.contig(off=3)       # contig 2, st_offset 3: a band at column 0 and one at the last column of either strand
    lay.put(2, 30, "+", gap=0), lay.put(3, 90, "-", gap=0), lay.put(4, 310, "+"), lay.put(2, 20, "-"), lay.put(5, 555, "-")
    lay.put(5, 640, "+", gap=7)                        # the contig ends with this band ...
    lay.put_ending(3, 101, "-", end=lay.cur["+"])      # ... and with this one on the other strand
    lay.contig(off=1)       # the last contig: both strands end with a band, the '-' one at the very end of the device's arrays
    lay.put(4, 1, "+", gap=0), lay.put(3, 3, "-", gap=0), lay.put(5, 700, "-", gap=1)
    lay.put(4, 250, "+"), lay.put(2, 16, "+", gap=0)
    lay.level()
    lay.put(3, 130, "+", gap=0), lay.put(4, 333, "-", gap=0)
    lay.put_ending(2, 2, "+", end=lay.cur["-"])
    return _case("array_edges_dna", 0, lay, qlens)


def _dtw_std():
    """--dtw-std: row 0 is the running sum from column 0 of the array.  col_st 0, 1, 2 and 300; and bands whose last column in
    front holds a spike, so that the prefix decides which moves tie: behind SPIKE every cost is rounded to steps of 0.5, behind
    HUGE every cost of the band is the prefix itself (the walk then goes diagonally wherever it can)"""
    qlens = (25, 100, 300)
    lay = _Layout("+")
    spikes = []
    for r, q in enumerate(qlens):
        for level in (None, SPIKE, HUGE):
            for col_st in (0, 1, 2, 300) if level is None else (1, 2, 300):
                c = lay.contig(off=(r + col_st) % 3)
                lay.put(r, q + (col_st % 7) - 3 if level is None else q - 2 - col_st % 3, gap=col_st)
                lay.close(tail=col_st % 4)
                if level is not None:
                    spikes.append((c, "+", col_st - 1, level))
    return _case("rna_dtw_std", RNA | DTW, lay, qlens, spikes=spikes)


def _orientation(name, flag):
    qlens = (30, 63, 100, 250, 500, 1000, 1500)  # none a multiple of its class's rows per lane but 500, 1000 (R = 32: 20, 8, 28 over)
    lay = _Layout("+")
    lay.contig(off=2)
    for r, q in enumerate(qlens):
        for m in (q - q // 5, q + q // 7 + 1, 3) if q < 600 else (q + 11,):
            lay.put(r, m)
    lay.close(tail=9)
    return _case(name, flag, lay, qlens)


def _forty_rows():
    """read 1 of three named by 40 rows with 40 bands (rows 7 and 39 identical), the other reads by one row each"""
    lay = _Layout("+-")
    lay.contig()
    for k in range(39):
        if k == 20:
            lay.contig(off=4)
        lay.put(1, 1 + (37 * k) % 260, "+-"[k % 2], gap=k % 3)
    lay.bands.append(lay.bands[7])
    lay.put(0, 40), lay.put(2, 600, "-")
    return _case("forty_rows_one_read", 0, lay, (33, 200, 555))


def _no_map():
    """unplanted bands at least as wide as the query between planted rows: their walks meet query row 0 behind the first column"""
    qlens = (25, 60, 200, 600)
    lay = _Layout("+-")
    lay.contig()
    for r, q in enumerate(qlens):
        lay.put(r, q + 5, "+")
        lay.put(r, q, "-", planted=False)
        lay.put(r, q - q // 4, "-")
        lay.put(r, 2 * q, "+", planted=False)
        lay.put(r, q + 10, "-", planted=False)
        lay.put(r, 2 * q, "-")
    return _case("no_map_between_maps", 0, lay, qlens)


def _strips(name, flag, qlens, col0):
    """rows beyond 2048 events (option map_strips): narrow planted bands, and one of m = qlen at 2049 events"""
    lay = _Layout("+")
    lay.contig()
    for r, q in enumerate(qlens):
        for k, m in enumerate((1, 2, 5, 63, 64, 65) + ((q,) if q == 2049 else ())):
            lay.put(r, m, gap=col0 if (r, k) == (0, 0) else 2)
    lay.close(tail=4)
    return _case(name, flag, lay, qlens, strips=True)


CASES = {c.name: c for c in (
    [_edges(ci) for ci in range(6)]
    + [_mixed("mixed_one_row", {16: 1, 32: 1, 64: 1}), _mixed("mixed_block_less_one", {16: 15, 32: 7, 64: 3}),
       _mixed("mixed_block", {16: 16, 32: 8, 64: 4}), _mixed("mixed_block_plus_one", {16: 17, 32: 9, 64: 5})]
    + [_array_edges(), _dtw_std(), _orientation("rna_reversed", RNA), _orientation("rna_invert", RNA | INV),
       _orientation("rna_full_ref", RNA | REF), _forty_rows(), _no_map(),
       _strips("strips_dna", 0, (2049, 4096, 4097, 6145), 0), _strips("strips_rna_dtw_std", RNA | DTW, (2049, 4097), 2),
       _strips("strips_rna_reversed", RNA, (2049, 6145), 0)])}
TABLE = [n for n, c in CASES.items() if not c.strips]
STRIPS = [n for n, c in CASES.items() if c.strips]
VARIANTS = ("quantised", "normal")
SEED_SALT = {"strips_rna_dtw_std": 1}  # (seed 0 left 5 of its 13 quantised planted rows without a complete map)


def _values(rng, n, quant):
    return (rng.integers(-6, 7, n) / 4).astype(np.float32) if quant else rng.normal(size=n).astype(np.float32)


def _plant_index(rng, qlen, m):
    if m == 1 or qlen == 1:
        return np.zeros(m, np.int64)
    if m >= qlen:
        rest = np.concatenate([np.arange(1, qlen), rng.integers(1, qlen, m - qlen)])
    else:
        rest = rng.choice(np.arange(1, qlen), m - 1, replace=False)
    return np.concatenate([[0], np.sort(rest)])


def rows_of(case, bands=None):
    """RESULT_DTYPE rows (valid = 1) that report the bands as the aligner would, and the read of each row"""
    import sigfish_amd as S
    bands = case.bands if bands is None else bands
    rows = np.zeros(len(bands), S.RESULT_DTYPE)
    for k, b in enumerate(bands):
        st, en = M.row_positions(b.col_st, b.col_st + b.m - 1, b.strand == "+", case.lens[b.contig], case.offs[b.contig])
        rows[k] = (b.contig, st, en, 0.0, 0.0, ord(b.strand), 0, 1, 0)
    return rows, np.array([b.read for b in bands], np.int32)


@functools.lru_cache(maxsize=None)
def build(name, variant):
    case, quant = CASES[name], variant == "quantised"
    rng = np.random.default_rng(zlib.crc32(name.encode()) * 2 + quant + 1000 * SEED_SALT.get(name, 0))
    rna = bool(case.flag & RNA)
    q_off = np.concatenate([[0], np.cumsum(case.qlens)]).astype(np.int64)
    q = _values(rng, int(q_off[-1]), quant)
    arrays = {"+": [_values(rng, n, quant) for n in case.lens]}
    if not rna:
        arrays["-"] = [_values(rng, n, quant) for n in case.lens]
    seen = set()
    for b in case.bands:
        assert 0 <= b.col_st and b.m >= 1 and b.col_st + b.m <= case.lens[b.contig], b
        if not b.planted or b in seen:
            continue
        seen.add(b)
        x = M.dp_query(q[q_off[b.read]:q_off[b.read + 1]], rna, bool(case.flag & INV))
        y = x[_plant_index(rng, len(x), b.m)]
        if not quant:
            y = y + rng.normal(0, 0.05, b.m).astype(np.float32)
        arrays[b.strand][b.contig][b.col_st:b.col_st + b.m] = y
    for contig, strand, col, level in case.spikes:
        arrays[strand][contig][col] = level
    for a in arrays.values():
        for y in a:
            y.setflags(write=False)
    q.setflags(write=False)
    rows, ror = rows_of(case)
    n = len(case.lens)
    return Built([f"c{i}" for i in range(n)], [x + 5 for x in case.lens], list(case.lens), list(case.offs), arrays["+"], arrays.get("-"),
                 q, q_off, rows, ror)


def ref_model(b):
    import sigfish_amd as S
    return S.RefModel(b.names, b.seq_lengths, b.ref_lengths, b.st_offset, b.forward, b.reverse)


@functools.lru_cache(maxsize=None)
def model_maps(name, variant):
    """the model's map of every row of the case (None: no complete map), computed once"""
    case, b = CASES[name], build(name, variant)
    memo, out = {}, []
    for k, band in enumerate(case.bands):
        if band not in memo:
            x = b.q[b.q_off[band.read]:b.q_off[band.read + 1]]
            memo[band] = M.row_map(b.rows[k], x, b.forward, b.reverse, b.st_offset, bool(case.flag & RNA), bool(case.flag & INV), bool(case.flag & DTW))
        out.append(memo[band])
    return out
