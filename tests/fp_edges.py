"""fp32 edge values for the DP, as data (tests/test_fp_edges_cpu.py shows from the oracle alone that each case reaches the range it
is named after, tests/test_fp_edges_gpu.py runs them through every alignment route).  Host-pure: numpy only.

DESIGN 3.4 says every cell is IEEE fp32 "with denormals" and the kernels lean on it: an unsigned min over bit patterns on query row
0, v_min3_f32 (whose result on denormals depends on the wave's FP mode) on the others, atomic minima and u64 keys over float bits,
hand-overs that are accepted only on bitwise equal costs.  The other inputs of the suite are of order 1 with sums of 10^2 .. 10^3.

A case is a flag, a reference of two contigs given as plain float32 arrays (LENS columns; RNA with non-zero ref_st_offset) and
ten reads of QLENS events: one of every base shape of the fill (64: 4 rows x 16 lanes, 250: 16 x 16, 257 and 600: 32 rows per lane,
1100: 32 x 64), two of 2100 events (two row strips; longer than either contig) and one of a single event.  A read follows a stretch
of one strand's array (about 0.6 columns per event, the strands in turn), so real alignments exist on '+' and on '-'.

Families (the same lengths in each):
  ordinary            the base: levels ~ N(0, 1), reads = their stretch + N(0, 0.3), z-normalised.  Not an edge; what the scaled
                      families are scaled from.
  pow2_scaled(k)      ordinary x 2^k, k = -120, -60, +60, +100: exact for +-60 and +100 (scores scale, everything else stays), NOT
                      for -120, where inputs below 2^-6 land under 2^-126 and lose bits (the read of one event, about 10^-4 in the
                      base, is one of them): the scores are no longer 2^k times the scores of the base.
  near_top            ordinary x s, s chosen so that the largest cell bound (below) is FLT_MAX / 3.
  denormal_all        levels are even integers of +-12, events their stretch with +-1 on a tenth of them (so no read costs 0), all
                      times 2^-149: every cell of every matrix is a denormal, the arithmetic is exact, ties are dense.
  denormal_crossing   ordinary x 2^-127 (rounded): values of 2^-130 .. 2^-124, early query rows denormal, later ones normal.
  absorbed            the first ABSORB_ROWS query rows are +-2^20 (x 0.9 .. 1.1) against levels ~ N(0, 1); the other events lie
                      10^-3 .. 10^-1 beside their column's level.  Behind those rows a sum is about 10^7, where fp32 counts in ones:
                      the small terms vanish, a term of a half and more counts as 1, and equal sums appear everywhere.  A stretch
                      of contig 0 is repeated in contig 1 with every level moved by 10^-3 .. 10^-2: to the reads drawn from it the
                      two cost the same in fp32 (score == score2, the later one wins) and not in float64.
  signed_zero         levels of {-0.0, +0.0, 1, -1}; reads are exact copies of their stretch with the signs of their zeros drawn
                      anew, a stretch of contig 0 is repeated in contig 1 (reads from it: score == score2 == +0, the 0 / 0 of
                      mapq_from_scores; the other exact reads: x / 0), two reads carry a few events no level equals.

Overflow is out of scope: a finite query whose costs overflow makes the reference abort.  Every cell of a subsequence
matrix is at most the cost of the straight path down its column, so bound() = max over reads and strands of
sum_rows max_cols |q_i - r|, in float64, bounds every cell; under --dtw-std row 0 is a running sum, so its last value is added.
build() asserts bound() < FLT_MAX / 2 for every case: no case here can produce an infinity.
"""
import functools
from collections import namedtuple

import numpy as np

RNA, DTW, INV = 0x001, 0x002, 0x004  # opt.flag bits (src/sigfish.h:30-39)
FLAGS = {"dna": 0, "rna": RNA, "rna_std": RNA | DTW, "rna_inv": RNA | INV}
FLT_MAX = float(np.finfo(np.float32).max)
MIN_NORMAL = float(np.finfo(np.float32).tiny)  # 2^-126
LENS = (701, 1503)
QLENS = (64, 250, 257, 600, 1100, 2100, 1, 250, 600, 2100)
ABSORB_ROWS = 10
POW2 = (-120, -60, 60, 100)
TWIN = (100, 400, 200)  # signed_zero, absorbed: columns [200, 500) of contig 1 '+' repeat columns [100, 400) of contig 0 '+'

Case = namedtuple("Case", "name family mode flag lens offs forward reverse q q_off origin")


def reverses(flag):
    """direct RNA without --invert is aligned with its events reversed (src/sigfish.c:857-866)"""
    return bool(flag & RNA) and not flag & INV


def jobs(case):
    """[(contig, strand, array)] in processing order: per contig '+', then '-' for DNA"""
    out = []
    for c, f in enumerate(case.forward):
        out.append((c, "+", f))
        if case.reverse is not None:
            out.append((c, "-", case.reverse[c]))
    return out


def events_of(case, i):
    return case.q[case.q_off[i]:case.q_off[i + 1]]


def dp_query(case, i):
    ev = events_of(case, i)
    return ev[::-1] if reverses(case.flag) else ev


def bound(case):
    """float64: the largest value a cell of any matrix of the case can take (module docstring)"""
    worst = 0.0
    for i in range(len(case.q_off) - 1):
        x = dp_query(case, i).astype(np.float64)
        for _, _, y in jobs(case):
            y = y.astype(np.float64)
            b = np.maximum(np.abs(x - y.min()), np.abs(x - y.max())).sum()
            if case.flag & DTW:
                b += np.abs(x[0] - y).sum()
            worst = max(worst, float(b))
    return worst


def windows(rlen, qlen):
    return -(-rlen // qlen)


# ---- the base: where the reads come from ----

def _sources(mode):
    """(contig, strand) of every read: the arrays long enough for its stretch, in turn"""
    strands = "+-" if mode == "dna" else "+"
    out, turn = [], {}
    for n in QLENS:
        span = max(1, (6 * n) // 10)
        ok = tuple((c, s) for c in range(len(LENS)) for s in strands if LENS[c] >= span + 2)
        out.append(ok[turn.get(ok, 0) % len(ok)])
        turn[ok] = turn.get(ok, 0) + 1
    return out


def _stretch(rng, rlen, n, lo=0, hi=None):
    """the columns the n events of a read follow: about 0.6 columns per event, inside [lo, hi)"""
    hi = rlen if hi is None else hi
    span = max(1, (6 * n) // 10)
    st = int(rng.integers(lo, hi - span + 1))
    return st + (np.arange(n) * span) // n


def _layout(mode, seed, twin=False):
    """-> rng, origin [(contig, strand, columns)] per read"""
    rng = np.random.default_rng(seed)
    origin = []
    for i, (c, s) in enumerate(_sources(mode)):
        if twin and i < 3:
            origin.append((0, "+", _stretch(rng, LENS[0], QLENS[i], TWIN[0], TWIN[1])))
        else:
            origin.append((c, s, _stretch(rng, LENS[c], QLENS[i])))
    return rng, origin


def _arrays(mode, draw):
    fw = [draw(n) for n in LENS]
    rv = [draw(n) for n in LENS] if mode == "dna" else None
    return fw, rv


def _finish(name, family, mode, fw, rv, reads_dp, origin):
    """reads_dp: the reads in DP order (query row 0 first)"""
    flag = FLAGS[mode]
    reads = [np.ascontiguousarray(x[::-1] if reverses(flag) else x, dtype=np.float32) for x in reads_dp]
    q_off = np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.int64)
    offs = [0, 0] if mode == "dna" else [1, 2]
    f32 = lambda arrs: None if arrs is None else [np.ascontiguousarray(a, dtype=np.float32) for a in arrs]
    case = Case(name, family, mode, flag, list(LENS), offs, f32(fw), f32(rv), np.concatenate(reads), q_off, origin)
    assert [len(x) for x in reads] == list(QLENS) and np.isfinite(case.q).all() and all(np.isfinite(y).all() for _, _, y in jobs(case))
    for a in [case.q] + [y for _, _, y in jobs(case)]:
        a.setflags(write=False)
    return case


def _source_array(fw, rv, c, s):
    return fw[c] if s == "+" else rv[c]


@functools.lru_cache(maxsize=None)
def _ordinary_f64(mode):
    """the base case in float64, before any rounding to float32: (fw, rv, reads in DP order, origin)"""
    rng, origin = _layout(mode, 4242 + len(mode))
    fw, rv = _arrays(mode, lambda n: rng.normal(size=n).astype(np.float32).astype(np.float64))
    reads = []
    for c, s, cols in origin:
        x = _source_array(fw, rv, c, s)[cols] + rng.normal(scale=0.3, size=len(cols))
        if len(x) > 1:
            x = (x - x.mean()) / x.std()
        else:
            x = rng.normal(scale=1e-4, size=1)  # one event has no z-score: a value in the middle of the levels, small enough to fall below 2^-126 at k = -120
        reads.append(x.astype(np.float32).astype(np.float64))
    return fw, rv, reads, origin


def _scaled(name, family, mode, s):
    fw, rv, reads, origin = _ordinary_f64(mode)
    mul = lambda arrs: None if arrs is None else [(a * s).astype(np.float32) for a in arrs]
    return _finish(name, family, mode, mul(fw), mul(rv), mul(reads), origin)


def ordinary(name, mode):
    return _scaled(name, "ordinary", mode, 1.0)


def pow2_scaled(name, mode, k):
    case = _scaled(name, f"pow2_scaled({k})", mode, 2.0 ** k)
    base = build(f"ordinary_{mode}")
    back = case.q.astype(np.float64) * 2.0 ** -k
    assert (k == -120) or np.array_equal(back, base.q.astype(np.float64)), "a power of two must scale the inputs exactly"
    return case


def near_top(name, mode):
    s = (FLT_MAX / 3) / bound(build(f"ordinary_{mode}"))
    case = _scaled(name, "near_top", mode, s)
    assert FLT_MAX / 8 < bound(case) < FLT_MAX / 2
    return case


def denormal_crossing(name, mode):
    case = _scaled(name, "denormal_crossing", mode, 2.0 ** -127)
    mags = np.abs(np.concatenate([case.q] + [y for _, _, y in jobs(case)]))
    assert np.median(mags) < MIN_NORMAL < mags.max() and 2.0 ** -124 > mags.max()
    return case


def denormal_all(name, mode):
    rng, origin = _layout(mode, 77 + len(mode))
    fw, rv = _arrays(mode, lambda n: 2 * rng.integers(-6, 7, n))
    reads = []
    for c, s, cols in origin:
        x = _source_array(fw, rv, c, s)[cols].copy()
        at = rng.choice(len(x), size=max(1, len(x) // 10), replace=False)
        x[at] += rng.integers(0, 2, len(at)) * 2 - 1  # odd: no (even) level equals it
        reads.append(x)
    unit = lambda arrs: None if arrs is None else [(a.astype(np.float64) * 2.0 ** -149).astype(np.float32) for a in arrs]
    case = _finish(name, "denormal_all", mode, unit(fw), unit(rv), unit(reads), origin)
    ints = np.concatenate([x[::-1] if reverses(case.flag) else x for x in reads])
    assert np.array_equal(case.q.view(np.int32) & 0x7fffffff, np.abs(ints)) and np.array_equal(case.q.view(np.uint32) >> 31, ints < 0)
    assert bound(case) < MIN_NORMAL  # no sum of any path leaves the denormals
    return case


def absorbed(name, mode):
    rng, origin = _layout(mode, 909 + len(mode), twin=True)
    fw, rv = _arrays(mode, lambda n: rng.normal(size=n).astype(np.float32))
    a, b, at = TWIN  # the repeat is a near twin: every level moved by 10^-3 .. 10^-2, which a sum of 10^7 does not see
    fw[1][at:at + b - a] = (fw[0][a:b] + 10.0 ** rng.uniform(-3, -2, b - a) * (rng.integers(0, 2, b - a) * 2 - 1)).astype(np.float32)
    reads = []
    for c, s, cols in origin:
        n = len(cols)
        x = _source_array(fw, rv, c, s)[cols].astype(np.float64)
        x += 10.0 ** rng.uniform(-3, -1, n) * (rng.integers(0, 2, n) * 2 - 1)
        big = min(n, ABSORB_ROWS)
        x[:big] = 2.0 ** 20 * rng.uniform(0.9, 1.1, big) * (rng.integers(0, 2, big) * 2 - 1)
        reads.append(x.astype(np.float32))
    return _finish(name, "absorbed", mode, fw, rv, reads, origin)


def signed_zero(name, mode):
    rng, origin = _layout(mode, 31 + len(mode), twin=True)
    values = np.array([-0.0, 0.0, 1.0, -1.0], np.float32)
    fw, rv = _arrays(mode, lambda n: values[rng.integers(0, 4, n)])
    a, b, at = TWIN
    fw[1][at:at + b - a] = fw[0][a:b]
    reads = []
    for i, (c, s, cols) in enumerate(origin):
        x = _source_array(fw, rv, c, s)[cols].copy()
        zero = x == 0
        x[zero] = np.where(rng.integers(0, 2, int(zero.sum())) == 1, np.float32(-0.0), np.float32(0.0))
        if i in (3, 7):  # two reads that no stretch answers exactly
            x[rng.choice(len(x), size=5, replace=False)] = np.float32(3.0)
        reads.append(x)
    case = _finish(name, "signed_zero", mode, fw, rv, reads, origin)
    assert (case.q.view(np.uint32) == 0x80000000).any() and (case.q.view(np.uint32) == 0).any()
    return case


# name -> (builder, mode, further arguments).  Every family on DNA (both strands); RNA (the query reversed), RNA --invert and
# --dtw-std on the families that leave fp32's middle furthest (--dtw-std not on near_top: its row 0 sums over the whole contig).
_TABLE = {}
for _mode in FLAGS:
    _TABLE[f"ordinary_{_mode}"] = (ordinary, _mode, ())


def _add(fn, mode, *args):
    name = fn.__name__ + "".join(f"_{'m' if a < 0 else 'p'}{abs(a)}" for a in args) + "_" + mode
    assert name not in _TABLE
    _TABLE[name] = (fn, mode, args)
    return name


NAMES = [_add(denormal_all, "dna"), _add(denormal_crossing, "dna")] + [_add(pow2_scaled, "dna", k) for k in POW2] + \
        [_add(near_top, "dna"), _add(absorbed, "dna"), _add(signed_zero, "dna"),
         _add(denormal_all, "rna"), _add(absorbed, "rna"), _add(pow2_scaled, "rna", -120),
         _add(denormal_crossing, "rna_inv"), _add(near_top, "rna_inv"), _add(signed_zero, "rna_inv"),
         _add(denormal_all, "rna_std"), _add(denormal_crossing, "rna_std"), _add(pow2_scaled, "rna_std", 100)]
FAMILIES = ["denormal_all", "denormal_crossing"] + [f"pow2_scaled({k})" for k in POW2] + ["near_top", "absorbed", "signed_zero"]


@functools.lru_cache(maxsize=None)
def build(name):
    """the case of that name; cached, so that the CPU and the GPU file, and every test in them, see the same arrays"""
    fn, mode, args = _TABLE[name]
    case = fn(name, mode, *args)
    assert bound(case) < FLT_MAX / 2, (name, bound(case))  # no cell of any matrix overflows
    return case


def family_of(name):
    fn, _, args = _TABLE[name]
    return fn.__name__ + (f"({args[0]})" if args else "")


def of_family(family, mode="dna"):
    return build([n for n in NAMES if _TABLE[n][1] == mode and family_of(n) == family][0])


def model(case):
    """the case's reference as the library takes it"""
    from sigfish_amd import api
    names = [f"c{i}" for i in range(len(case.lens))]
    return api.RefModel(names, [n + 5 for n in case.lens], case.lens, case.offs, case.forward, case.reverse)


def oracle_ref(O, case):
    names = [f"c{i}" for i in range(len(case.lens))]
    return O.RefSynth(names, [n + 5 for n in case.lens], case.lens, case.offs, case.forward, case.reverse)


def subset(case, reads):
    """(q, q_off) of the named reads alone"""
    parts = [events_of(case, i) for i in reads]
    return np.concatenate(parts), np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)


def last_row_of(x, y, dtype=np.float64):
    """The last row of subsequence(x, y) with every sum in `dtype`, by anti-diagonals (what the oracle computes in float32, here
    for asking what a wider accumulator would have answered)."""
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    n, m = len(x), len(y)
    inf = dtype(np.inf)
    prev2 = np.full(n, inf, dtype)  # diagonal d - 2, indexed by query row
    prev1 = np.full(n, inf, dtype)
    out = np.empty(m, dtype)
    for d in range(n + m - 1):
        lo, hi = max(0, d - m + 1), min(n - 1, d)
        i = np.arange(lo, hi + 1)
        dist = np.abs(x[i] - y[d - i])
        cur = np.full(n, inf, dtype)
        k = i >= 1
        up = np.where(k, prev1[np.maximum(i - 1, 0)], inf)
        diag = np.where(k, prev2[np.maximum(i - 1, 0)], inf)
        left = prev1[i]
        best = np.minimum(np.minimum(up, diag), left)
        best = np.where(i == 0, dtype(0), best)  # free start in query row 0
        cur[i] = dist + best
        if hi == n - 1:
            out[d - (n - 1)] = cur[n - 1]
        prev2, prev1 = prev1, cur
    return out
