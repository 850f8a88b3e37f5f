"""Exact ties on purpose, for the batch path (tests/test_tie_cases_cpu.py shows each from the oracle and the planner alone,
tests/test_tie_cases_gpu.py runs them through align_db).  Two rules decide who wins an exact tie (oracle/sdtw_oracle.c):
  * inside a window of qlen last-row columns the FIRST column wins (scan_windows: a strict <, src/sigfish.c:891-901);
  * between candidates -- the windows of a job, '+' then '-' of a contig, the contigs in order -- the LATER one ranks better
    (top_offer: !(score > t[l].score), src/sigfish.c:577-583), and score2 is simply the next entry of that list;
  * --dtw-std has one candidate per contig (its bottom-right cell): only the second rule applies.

A case is a flag, a reference model given as arrays, a handful of reads of ONE query length and, the same for every read, a
claim: tuples of (contig, strand, last-row column) that hold bitwise equal values, each the minimum of its window; the
candidate the reference reports; whether score == score2; for the cases with six and more tied candidates the five that stay,
best first.  Nothing here asks the oracle: the ties are structural and the seeds below were chosen until every claim held.

How a tie is made.  All levels are multiples of 1/4 of small magnitude, so every sum of the recurrence is exact in fp32 and two
cells tie whenever their cheapest paths cost the same.  A stretch S of distinct neighbouring levels is planted behind a
context C ("block" X = C | S, the context at least a query long where the contig has the room); a read is S stretched to qlen
events (`stretch` events per column) with +-1/4 on a tenth of its events -- never on its last ones -- so scores are not 0.
  * copies of X inside a contig, exact copies of a contig, and DNA whose reverse array equals its forward array: twins;
  * "dup": the column behind S repeats S's last level, which the read's last event equals -- the cell below-right of the
    winner then costs exactly as much (the step to it is free, and a repeated column is never cheaper than its original);
  * the column behind that is 1.5 away from S's last level, so the minimum does not run on.
A case's seed selects S, C, the filler and the noise.
"""
import functools
from collections import namedtuple

import numpy as np

RNA, DTW, INV = 0x001, 0x002, 0x004  # opt.flag bits (src/sigfish.h:30-39)
FLAGS = {"dna": 0, "rna": RNA, "rna_std": RNA | DTW, "rna_inv": RNA | INV}
REPS = (1, 5, 300)  # copies of a case's reads in one batch: other widenings, chunk counts and segments (sfa_plan.hpp)
N_SIMS = 1024       # SIMDs of an MI355X (256 CUs x 4): what the planner sizes chunks and widening by

Case = namedtuple("Case", "name mode flag qlen lens offs forward reverse q q_off ties winner top_tie top5 segments chunk_pairs real_split options zero")


def _levels(rng, n):
    return (rng.integers(-6, 7, n) / 4).astype(np.float32)


def _stretch_of_distinct_neighbours(rng, m):
    s = _levels(rng, m)
    for i in range(1, m):
        if s[i] == s[i - 1]:
            s[i] = s[i] + np.float32(0.75 if s[i] < 0.5 else -0.75)
    return s


def _stop(v):
    return np.float32(v - 1.5 if v > 0 else v + 1.5)


def _plant(arr, e, X, dup=False):
    """X ends in column e of arr (cut on the left where the contig begins); behind it the repeated last level, then the stop"""
    st = e - len(X) + 1
    cut = max(0, -st)
    arr[st + cut:e + 1] = X[cut:]
    nxt = e + 1
    if dup:
        assert nxt < len(arr)
        arr[nxt] = X[-1]
        nxt += 1
    if nxt < len(arr):
        arr[nxt] = _stop(X[-1])


def job_of(flag, contig, strand):
    """index into the job list: per contig '+', then '-' for DNA (src/sigfish.c:868-952)"""
    return contig if flag & RNA else 2 * contig + (strand == "-")


def windows(rlen, qlen):
    """[(first column, one past the last)] of the last-row windows of a job"""
    return [(w, min(w + qlen, rlen)) for w in range(0, rlen, qlen)]


def segment_range(rlen, qlen, n_seg, warm_windows, seg):
    """sdtw_kernels.hpp, segment_range: (col0, col_real, col_end, empty, last) of segment `seg` of a job"""
    nwin = (rlen + qlen - 1) // qlen
    nw = (nwin + n_seg - 1) // n_seg
    w_real = seg * nw
    return (max(0, w_real - warm_windows) * qlen, w_real * qlen, min(rlen, (w_real + nw) * qlen), w_real >= nwin, w_real + nw >= nwin)


class _Build:
    """what every builder below fills: contigs of filler, blocks planted into them, twins, then the reads"""

    def __init__(self, name, mode, qlen, seed, stretch=1, ctx=None, n_reads=4, noisy=True):
        self.name, self.mode, self.flag, self.qlen, self.stretch = name, mode, FLAGS[mode], qlen, stretch
        self.rng = np.random.default_rng(seed)
        self.m = -(-qlen // stretch)
        self.S = _stretch_of_distinct_neighbours(self.rng, self.m)
        self.C = _levels(self.rng, qlen if ctx is None else ctx)
        self.X = np.concatenate([self.C, self.S])
        self.n_reads, self.noisy = n_reads, noisy
        self.fw, self.rv, self.offs = [], [], []
        self.ties, self.winner, self.top_tie, self.top5 = [], None, False, None
        self.segments, self.chunk_pairs, self.real_split, self.options = [], [], (), {}

    @property
    def dna(self):
        return not self.flag & RNA

    def contig(self, n, off=0):
        self.fw.append(_levels(self.rng, n))
        self.rv.append(_levels(self.rng, n) if self.dna else None)
        self.offs.append(off if not self.dna else 0)
        return len(self.fw) - 1

    def copy_of(self, c):
        self.fw.append(self.fw[c].copy())
        self.rv.append(self.rv[c].copy() if self.dna else None)
        self.offs.append(self.offs[c])
        return len(self.fw) - 1

    def strand_twin(self, c):
        assert self.dna
        self.rv[c] = self.fw[c].copy()

    def plant(self, c, e, strand="+", dup=False, X=None):
        _plant(self.fw[c] if strand == "+" else self.rv[c], e, self.X if X is None else X, dup)
        return (c, strand, e)

    def degraded(self, d):
        """X with 3 * d columns of S raised or lowered by 1/2: a copy that matches the reads worse, the more the larger d"""
        X = self.X.copy()
        at = len(self.C) + (np.arange(3 * d) * 7 + 2) % max(self.m - 2 * self.stretch, 1)
        X[at] += np.where(X[at] > 0, -0.5, 0.5).astype(np.float32)
        return X

    def reads(self):
        base = self.S[(np.arange(self.qlen) * self.m) // self.qlen]
        out = []
        for _ in range(self.n_reads):
            x = base.copy()
            if self.noisy:
                free = max(self.qlen - 2 * self.stretch - 1, 1)  # the last events stay exact
                at = self.rng.choice(free, size=min(max(2, self.qlen // 10), free), replace=False)
                x[at] += (self.rng.integers(0, 2, len(at)) * 2 - 1).astype(np.float32) / 4
            out.append(x[::-1].copy() if (self.flag & RNA and not self.flag & INV) else x)  # query_rows (src/sigfish.c:857-866) turns it back
        return out

    def done(self):
        rd = self.reads()
        q_off = np.concatenate([[0], np.cumsum([len(x) for x in rd])]).astype(np.int64)
        lens = [len(a) for a in self.fw]
        assert sum(lens) <= 9100 and len(rd) <= 40
        return Case(self.name, self.mode, self.flag, self.qlen, lens, list(self.offs), self.fw, self.rv if self.dna else None, np.concatenate(rd).astype(np.float32),
                    q_off, self.ties, self.winner, self.top_tie, self.top5, self.segments, self.chunk_pairs, self.real_split, self.options, not self.noisy)


# ---- the situations ----

def in_window_adjacent(name, mode, qlen, seed, n_reads=4):
    """two tied minima next to each other in the middle of window 2 (dup): the first wins; the last window is partial"""
    b = _Build(name, mode, qlen, seed, n_reads=n_reads)
    c = b.contig(3 * qlen + qlen // 3 + 1)
    e = 2 * qlen + qlen // 2
    first = b.plant(c, e, dup=True)
    b.ties, b.winner = [(first, (c, "+", e + 1))], first
    return b.done()


def in_window_far(name, mode, qlen, seed):
    """two tied minima half a window apart inside window 2: blocks of qlen / 2 columns, four events per column.  The first wins;
    the block in front of the pair ends window 1 with the same value, which is score2."""
    half = qlen // 2
    b = _Build(name, mode, qlen, seed, stretch=4, ctx=half - -(-qlen // 4))
    assert len(b.X) == half
    c = b.contig(4 * qlen + 3)
    lead = b.plant(c, 2 * qlen - 1 - 3)  # (both of the pair then have a block's stretch and context behind them)
    first = b.plant(c, 2 * qlen + half - 1 - 3)
    second = b.plant(c, 3 * qlen - 1 - 3)
    b.ties, b.winner, b.top_tie = [(first, second), (lead, first)], first, True
    return b.done()


def edge_adjacent(name, mode, qlen, seed, n_reads=4):
    """tied minima in the last column of window 1 and the first column of window 2 (dup): the later wins, the earlier is score2.
    For a contig of fewer than three windows the pair sits on the edge of window 0, and window 1 is the last, partial one."""
    b = _Build(name, mode, qlen, seed, n_reads=n_reads)
    big = qlen > 2100
    c = b.contig(qlen + 3000 if big else 3 * qlen + qlen // 3)
    e = qlen - 1 if big else 2 * qlen - 1
    first = b.plant(c, e, dup=True)
    later = (c, "+", e + 1)
    b.ties, b.winner, b.top_tie = [(first,), (later,), (first, later)], later, True
    return b.done()


def windows_apart(name, mode, qlen, seed):
    """twins in windows 1 and 3, window 2 between them (two events per column): the later wins, score == score2"""
    b = _Build(name, mode, qlen, seed, stretch=2)
    c = b.contig(4 * qlen + 5, off=2)
    e = len(b.X) + 1
    assert e // qlen == 1
    first, later = b.plant(c, e), b.plant(c, e + 2 * qlen)
    b.ties, b.winner, b.top_tie = [(first, later)], later, True
    return b.done()


def last_partial(name, mode, qlen, seed, n_reads=4):
    """a twin in window 1 and one in the last, partial window (rlen % qlen = qlen / 2): the later wins, score == score2"""
    b = _Build(name, mode, qlen, seed, stretch=2, n_reads=n_reads)
    c = b.contig(3 * qlen + qlen // 2)
    first, later = b.plant(c, len(b.X) + 1), b.plant(c, 3 * qlen + qlen // 4)
    assert first[2] // qlen == 1 and later[2] - len(b.X) > first[2]
    b.ties, b.winner, b.top_tie = [(first, later)], later, True
    return b.done()


def short_contig_twins(name, mode, qlen, seed, n_reads=4):
    """contigs shorter than the query (one partial window each), one of filler between them: the later twin wins"""
    b = _Build(name, mode, qlen, seed, stretch=2, ctx=qlen // 5, n_reads=n_reads)
    n = len(b.X) + 4
    assert n < qlen
    a = b.contig(n)
    first = b.plant(a, n - 3)
    b.contig(qlen // 2 + 7)
    z = b.copy_of(a)
    later = (z, "+", n - 3)
    b.ties, b.winner, b.top_tie = [(first, later)], later, True
    return b.done()


def contig_twins(name, mode, qlen, seed, n_contigs, twins, n_reads=40):
    """many short contigs, so that the planner cuts the job list into chunks of one and two jobs once the batch is large; the
    twins are exact copies of each other on either side of such a cut.  The later twin wins, score == score2."""
    b = _Build(name, mode, qlen, seed, n_reads=n_reads)
    n = 160
    e = 140
    assert len(b.X) <= e
    for c in range(n_contigs):
        if c == twins[1]:
            b.copy_of(twins[0])
        else:
            b.contig(n)
            if c == twins[0]:
                b.plant(c, e)
    first, later = (twins[0], "+", e), (twins[1], "+", e)
    b.ties, b.winner, b.top_tie = [(first, later)], later, True
    b.chunk_pairs = [(job_of(b.flag, twins[0], "-" if b.dna else "+"), job_of(b.flag, twins[1], "+"))]
    b.real_split = (300,)
    return b.done()


def strand_twin(name, mode, qlen, seed, n_reads=4):
    """DNA whose reverse array equals its forward array: '-' comes later and wins, score == score2"""
    b = _Build(name, mode, qlen, seed, n_reads=n_reads)
    c = b.contig(qlen + qlen // 2)
    b.plant(c, qlen + qlen // 3)
    b.strand_twin(c)
    e = qlen + qlen // 3
    b.ties, b.winner, b.top_tie = [((c, "+", e), (c, "-", e))], (c, "-", e), True
    return b.done()


def segment_twins(name, mode, qlen, seed, n_seg, edge):
    """lane_widening 4 with column_segments 2 or 3: a contig of 50 windows, twins on either side of the last hand-over --
    edge: in its two neighbouring columns (dup); else: two windows in front of it and one behind, and for three segments a third
    twin in front of the first hand-over.  The later wins, score == score2."""
    b = _Build(name, mode, qlen, seed, stretch=1 if edge else 2)
    rlen = 50 * qlen
    c = b.contig(rlen)
    bounds = [segment_range(rlen, qlen, n_seg, 4, s)[1] for s in range(1, n_seg)]
    assert all(0 < x < rlen for x in bounds)
    h = bounds[-1]
    if edge:
        first = b.plant(c, h - 1, dup=True)
        cols = [first, (c, "+", h)]
        b.ties = [(first,), (cols[1],), tuple(cols)]
    else:
        cols = [b.plant(c, h - 2 * qlen + qlen // 2), b.plant(c, h + qlen + qlen // 2)]
        if n_seg == 3:
            cols.insert(0, b.plant(c, bounds[0] - 2 * qlen + qlen // 2))
        b.ties = [tuple(cols)]
    b.winner, b.top_tie = cols[-1], True
    j = job_of(b.flag, c, "+")
    b.segments = [(n_seg, j, x[2], y[2]) for x, y in zip(cols, cols[1:])]
    b.options = {"lane_widening": 4, "column_segments": n_seg}
    return b.done()


def many_windows(name, mode, qlen, seed):
    """seven tied candidates in every second window of one contig: the last five stay, the latest first; the fifth ties with the
    one that fell out"""
    b = _Build(name, mode, qlen, seed, stretch=2)
    c = b.contig(14 * qlen + qlen // 2)
    e0 = len(b.X) + 1
    cols = [b.plant(c, e0 + 2 * qlen * k) for k in range(7)]
    b.ties, b.winner, b.top_tie, b.top5 = [tuple(cols)], cols[-1], True, cols[:1:-1]
    return b.done()


def many_contigs(name, mode, qlen, seed, n_reads=4, stretch=2):
    """six exact copies of one contig shorter than the query (DNA: the strand twin too, twelve candidates): the last five stay"""
    b = _Build(name, mode, qlen, seed, stretch=stretch, ctx=qlen // 20, n_reads=n_reads)
    n = len(b.X) + 5
    a = b.contig(n)
    b.plant(a, n - 3)
    if b.dna:
        b.strand_twin(a)
    for _ in range(5):
        b.copy_of(a)
    cols = [(c, s, n - 3) for c in range(6) for s in ("+-" if b.dna else "+")]
    b.ties, b.winner, b.top_tie, b.top5 = [tuple(cols)], cols[-1], True, cols[:-6:-1]
    return b.done()


def rank5_tie(name, mode, qlen, seed, n_reads=4, stretch=1):
    """four candidates strictly better than each other, then two tied ones for the fifth place: the later of the two keeps it.
    Contigs in processing order: worst twin, third, worst twin again, best, fourth, second."""
    b = _Build(name, mode, qlen, seed, stretch=stretch, ctx=qlen // 8, n_reads=n_reads)
    n = len(b.X) + 6
    e = n - 3
    worst = b.degraded(5)
    for d in (5, 2, 5, 0, 3, 1):
        c = b.contig(n)
        b.fw[c][:] = b.fw[0]  # the same filler around every copy
        b.plant(c, e, X=worst if d == 5 else b.degraded(d) if d else b.X)
    col = lambda c: (c, "+", e)
    b.ties, b.winner, b.top5 = [(col(0), col(2))], col(3), [col(3), col(5), col(1), col(4), col(2)]
    return b.done()


def std_twins(name, mode, qlen, seed, n_reads=4):
    """--dtw-std: one candidate per contig, its last column.  Contigs 0, 2 and 4 are the stretch itself (two events per column),
    1 and 3 filler: the last twin wins, score == score2."""
    b = _Build(name, mode, qlen, seed, stretch=2, ctx=0, n_reads=n_reads)
    for c in range(5):
        k = b.contig(b.m)
        if c % 2 == 0:
            b.fw[k][:] = b.S
    cols = [(c, "+", b.m - 1) for c in (0, 2, 4)]
    b.ties, b.winner, b.top_tie = [tuple(cols)], cols[-1], True
    return b.done()


def zero_score(name, mode, qlen, seed):
    """THE zero-score case: reads that are the stretch itself against twin contigs.  score == score2 == 0, so mapq is the
    reference's 0 / 0 (orc_mapq: NaN saturates to INT_MIN, whose low byte is 0) -- whatever the oracle gives."""
    b = _Build(name, mode, qlen, seed, n_reads=2, noisy=False)
    a = b.contig(2 * qlen + 9)
    first = b.plant(a, qlen + qlen // 2)
    z = b.copy_of(a)
    later = (z, "+", first[2])
    b.ties, b.winner, b.top_tie = [(first, later)], later, True
    return b.done()


# name -> (builder, mode, query length, seed, further arguments).  Every query length class: 24, 64 (4 rows per lane), 130 (8 .. 16),
# 250 (16), 600 and 1024 (32 rows, 32 lanes), 1500 and 2048 (a wave per read), 2100 and 4500 (row strips: two and three strips).
_TABLE = {}


def _add(fn, mode, qlen, seed, **kw):
    name = f"{fn.__name__}_{mode}_q{qlen}" + "".join(f"_{k[0]}{'_'.join(str(x) for x in v) if isinstance(v, tuple) else v}" for k, v in kw.items() if k != "n_reads")
    assert name not in _TABLE
    _TABLE[name] = (fn, mode, qlen, seed, kw)


for _mode, _q in (("dna", 24), ("rna", 250), ("rna_inv", 1024), ("dna", 2100)):
    _add(in_window_adjacent, _mode, _q, 1, n_reads=2 if _q > 2048 else 4)
for _mode, _q in (("rna", 64), ("dna", 600), ("rna_inv", 1500)):
    _add(in_window_far, _mode, _q, 1)
for _mode, _q in (("rna", 24), ("dna", 64), ("rna_inv", 250), ("dna", 600), ("rna", 1024), ("dna", 1500), ("rna_inv", 2048), ("rna", 2100), ("dna", 4500)):
    _add(edge_adjacent, _mode, _q, 1, n_reads=2 if _q > 2048 else 4)
for _mode, _q in (("dna", 64), ("rna", 250), ("rna_inv", 1024), ("rna", 2048)):
    _add(windows_apart, _mode, _q, 1)
for _mode, _q in (("rna_inv", 24), ("dna", 600), ("rna", 2100)):
    _add(last_partial, _mode, _q, 1, n_reads=2 if _q > 2048 else 4)
for _mode, _q in (("dna", 64), ("rna", 1500), ("rna_inv", 4500)):
    _add(short_contig_twins, _mode, _q, 1, n_reads=2 if _q > 2048 else 4)
# 48 jobs; 40 reads x 300 are 3 000 waves, for which chunks_for() asks for 33 chunks: the cuts of split_jobs() fall behind jobs
# 0, 2, 3, 5, 6, ... (tests/test_tie_cases_cpu.py recomputes them)
_add(contig_twins, "rna", 24, 1, n_contigs=48, twins=(2, 3))
_add(contig_twins, "rna_inv", 64, 1, n_contigs=48, twins=(0, 47))
_add(contig_twins, "dna", 64, 1, n_contigs=24, twins=(1, 2))
_add(contig_twins, "dna", 24, 1, n_contigs=24, twins=(0, 23))
for _q in (250, 1500, 4500):
    _add(strand_twin, "dna", _q, 1, n_reads=2 if _q > 2048 else 4)
for _mode, _n, _edge in (("dna", 2, True), ("rna", 2, False), ("rna_inv", 3, True), ("dna", 3, False)):
    _add(segment_twins, _mode, 130, 1, n_seg=_n, edge=_edge)
for _mode, _q in (("rna", 64), ("dna", 250), ("rna_inv", 600)):
    _add(many_windows, _mode, _q, 1)
for _mode, _q, _s in (("dna", 250, 2), ("rna", 1024, 2), ("rna_inv", 2100, 2), ("dna", 4500, 4)):
    _add(many_contigs, _mode, _q, 1, n_reads=2 if _q > 2048 else 4, stretch=_s)
for _mode, _q, _s in (("rna", 64, 1), ("dna", 600, 1), ("rna_inv", 2048, 2), ("rna", 2100, 2)):
    _add(rank5_tie, _mode, _q, 1, n_reads=2 if _q > 2048 else 4, stretch=_s)
for _q in (24, 250, 1024, 2048, 2100):
    _add(std_twins, "rna_std", _q, 1, n_reads=2 if _q > 2048 else 4)
_add(zero_score, "rna", 250, 1)

NAMES = list(_TABLE)
MANY = [n for n in NAMES if _TABLE[n][0] in (many_windows, many_contigs, rank5_tie)]  # the cases with a claim about the top-5 list
SEGMENTED = [n for n in NAMES if _TABLE[n][0] is segment_twins]
SPLIT = [n for n in NAMES if _TABLE[n][0] is contig_twins]


@functools.lru_cache(maxsize=None)
def build(name):
    """the case of that name; cached, so that the CPU and the GPU file, and every test in them, see the same arrays"""
    fn, mode, qlen, seed, kw = _TABLE[name]
    return fn(name, mode, qlen, seed, **kw)


def repeated(case, reps):
    """the case's reads `reps` times in one batch -> (q, q_off)"""
    lens = np.diff(case.q_off)
    return np.tile(case.q, reps), np.concatenate([[0], np.cumsum(np.tile(lens, reps))]).astype(np.int64)


def job_lens(case):
    return [n for n in case.lens for _ in range(1 if case.flag & RNA else 2)]


def plan_request(case, reps, widening=0, segments=0, secondary=0):
    """the line tests/c/tie_plan.cpp answers for the case's reads `reps` times in one batch"""
    jl = job_lens(case)
    ql = list(np.tile(np.diff(case.q_off), reps))
    return (f"plan {N_SIMS} {widening} {segments} {secondary} {int(bool(case.flag & DTW))} {len(ql)} {len(jl)}\n" + " ".join(str(int(x)) for x in ql) + "\n" +
            " ".join(str(x) for x in jl) + "\n")
