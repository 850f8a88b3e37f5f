"""Deterministic inputs for the event detection's edges (tests/test_events_edges_cpu.py, tests/test_events_edges_gpu.py):
every length and content at which events_kernels.hpp takes another path, built once per chemistry.

A case is (name, raw int16, (digitisation, offset, range)).  What each case is FOR is only true while the signal behaves as
intended (the speculative picker accepts it, the certificate fails, ...): test_events_edges_cpu.py asserts those intentions
with the model of tests/events_model.py, so a signal that stops doing its job fails there, without a GPU."""
import functools
import zlib

import numpy as np

from sigfish_amd.synth import R9_DNA_META

SCALE = (R9_DNA_META["digitisation"], R9_DNA_META["offset"], R9_DNA_META["range"])
UNIT = np.float32(SCALE[2]) / np.float32(SCALE[0])   # pA per count
DWELL = {False: (6, 13), True: (10, 25)}             # samples per level: DNA, RNA (numpy's half-open ranges, 25 included below)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def to_raw(pa, scale=SCALE):
    unit = np.float32(scale[2]) / np.float32(scale[0])
    return np.clip(np.round(np.asarray(pa, np.float64) / float(unit) - scale[1]), -32768, 32767).astype(np.int16)


def step_pa(rng, n, dwell, noise=1.5, mu=90.0, sd=12.0):
    """An ordinary step signal in pA: levels ~ N(mu, sd), each held for dwell[0] .. dwell[1] samples, white noise on top."""
    if n == 0:
        return np.zeros(0)
    d = rng.integers(dwell[0], dwell[1] + 1, size=n // dwell[0] + 2)
    x = np.repeat(rng.normal(mu, sd, size=len(d)), d)[:n]
    return x + rng.normal(0.0, noise, size=n)


def ordinary(key, n, rna, dwell=None):
    return to_raw(step_pa(_rng("ordinary", key, n, rna), n, dwell or DWELL[rna]))


def chunk(n):
    return (n + 63) // 64   # samples per lane of the speculative peak picker


# lengths of the ordinary reads: around the long window (filled in per chemistry), around the tiles of 32 samples, and around
# the speculative picker's range of 24 .. 288 samples per lane
TILE_LENGTHS = (31, 32, 33, 63, 64, 65, 95, 96, 97)
SPEC_LENGTHS = (1472, 1473, 1536, 4096, 4097, 18432, 18433)
OUT_OF_RANGE = (1472, 18433)   # of SPEC_LENGTHS (every shorter length is out of range as well)

# The reads that have to be accepted by the speculative picker for their case to mean anything, but would rarely be with an
# arbitrary signal: at 24 or 25 samples per lane every lane has one or two events in which to meet its neighbour's walk.  They use
# the short end of the dwell range, and seeds found by trying 0, 1, 2, ... against events_model.spec_accepts;
# test_events_edges_cpu.py asserts that they still do their job.
SHORT_CHUNK_DWELL = {False: (6, 9), True: (10, 12)}
SEED = {False: {1473: 0, 1536: 0}, True: {1473: 5, 1536: 4}}
MANY_ORDINARY_SEEDS = {False: (0, 1, 2, 3, 4, 5, 6, 7, 8, 9), True: (0, 1, 4, 9, 10, 15, 18, 22, 26, 29)}   # batch (c)
FILLER_SEED = {False: {}, True: {8: 72, 9: 105, 10: 106}}   # filler k uses seed k unless named here
UNIT_SCALE = (8192.0, 0.0, 8192.0)   # pA == counts: sums of a noiseless signal are exact, flat stretches have t == 0


def _content_cases(rna, n):
    """The reads whose CONTENT is the edge, at n samples."""
    dw = DWELL[rna]
    C = chunk(n)
    out = []
    rng = _rng("content", rna, n)
    # exact ties in both statistics: every sample a multiple of 8 counts, little noise, so neighbouring windows repeat
    q = to_raw(step_pa(rng, n, dw, noise=0.6))
    out.append(("quantised", (np.round(q / 8.0) * 8).astype(np.int16), SCALE))
    out.append(("constant", np.full(n, 500, np.int16), SCALE))
    out.append(("zero_pa", np.full(n, -int(SCALE[1]), np.int16), SCALE))
    out.append(("ramp", np.round(np.linspace(200, 900, n)).astype(np.int16), SCALE))
    run = 2 * dw[1]
    out.append(("int16_extremes", np.where((np.arange(n) // run) % 2 == 0, 32767, -32768).astype(np.int16), SCALE))
    # level changes forced onto a tile boundary, onto a chunk boundary and onto the last sample of a chunk
    x = step_pa(rng, n, dw)
    for k, pos in enumerate((32 * (n // 96), C * 21, C * 42 - 1)):
        x[pos:] += (30.0 if k % 2 == 0 else -30.0) - (x[pos] - x[pos - 1])
    out.append(("changes_on_boundaries", to_raw(x), SCALE))
    # the suite's trick: a tiny offset turns raw == 0 into 1e-30 pA next to ordinary values, more than 52 bits apart
    r = to_raw(step_pa(rng, n, dw))
    r[::97] = 0
    out.append(("tiny_offset", r, (SCALE[0], 1e-30, SCALE[2])))
    out.append(("range_inf", to_raw(step_pa(rng, n, dw)), (SCALE[0], SCALE[1], float("inf"))))
    return [(f"{name}_{n}", raw, sc) for name, raw, sc in out]


def _few_events(n):
    """Four events in the whole read (pA == counts, no noise: nothing else fires): no lane ever meets its neighbour's walk."""
    x = np.full(n, 80.0)
    for k, c in enumerate((n // 5, 2 * n // 5 + 7, 3 * n // 5 + 3)):
        x[c:] += 25.0 if k % 2 == 0 else -25.0
    return x.astype(np.int16)


def _dense(n, key):
    """DNA: a level change every 3 to 5 samples, more firings of the short detector than a lane's lists hold."""
    rng = _rng("dense", False, n, key)
    d = rng.integers(3, 6, size=n // 3 + 2)
    lv = 90.0 + 40.0 * (np.arange(len(d)) % 2) + rng.normal(0.0, 3.0, size=len(d))
    return to_raw(np.repeat(lv, d)[:n] + rng.normal(0.0, 0.3, size=n))


PERIOD_11 = (1027, 330, 11, -39, -672, -765, -143, 0, 192, 226, 735)


def _period_11(n):
    """RNA: a noiseless pattern of 11 samples (pA == counts) on which the short detector (window 7) fires twice per period.
    Samples per lane decide what that does to the lists of the speculative picker, which hold 48 firings: 266 per lane
    (17000 samples) give the fullest lane exactly 48, 270 (17280) give it 49, 288 (18432) give it 52."""
    return np.tile(np.array(PERIOD_11, np.int16), n // 11 + 1)[:n]


def _noiseless_steps(n, rna):
    """An ordinary step signal without noise, pA == counts: events only where the level changes, few enough for the lists of the
    speculative picker even at 288 samples per lane (with noise the DNA detector fires every 5 samples or so and overflows them)."""
    rng = _rng("noiseless", n, rna)
    d = rng.integers(DWELL[rna][0], DWELL[rna][1] + 1, size=n // DWELL[rna][0] + 2)
    return np.repeat(np.round(rng.normal(500.0, 70.0, size=len(d))), d)[:n].astype(np.int16)


def _piecewise_linear(seed, n=1400):
    """A noiseless signal of straight pieces (pA == counts).  On a ramp both statistics are all but constant, so the short
    detector stays in its search and masks nothing; at the kinks the LONG detector is then the one that fires -- which ordinary
    signals never let it do.  Seeds chosen (RNA) so that the long detector's sample at the end of a 32-sample tile decides a
    peak: test_events_edges_cpu.py::test_long_detector_decides_across_tiles."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(np.repeat(rng.uniform(-60, 60, size=n // 25 + 1), 25)[:n])
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


PIECEWISE_SEEDS = (29, 15)


@functools.lru_cache(maxsize=None)
def cases(rna):
    """Every case of one chemistry, by name (batch (a) orders them)."""
    w2 = 14 if rna else 6
    c = {}
    for n in (1, 2 * w2 - 1, 2 * w2, 2 * w2 + 1) + TILE_LENGTHS + SPEC_LENGTHS:
        if n in SEED[rna]:
            c[f"len_{n}"] = (ordinary(SEED[rna][n], n, rna, SHORT_CHUNK_DWELL[rna]), SCALE)
        else:
            c[f"len_{n}"] = (ordinary(0, n, rna), SCALE)
    for n in (1600, 6000):
        for name, raw, sc in _content_cases(rna, n):
            c[name] = (raw, sc)
    if rna:
        c["dense_18432"] = (_period_11(18432), UNIT_SCALE)
        c["dense_17280"] = (_period_11(17280), UNIT_SCALE)
        c["full_lists_17000"] = (_period_11(17000), UNIT_SCALE)
    else:
        c["dense_18432"] = (_dense(18432, 0), SCALE)
        c["dense_16000"] = (_dense(16000, 1), SCALE)
    c["noiseless_18432"] = (_noiseless_steps(18432, rna), UNIT_SCALE)
    c["four_events_6000"] = (_few_events(6000), UNIT_SCALE)
    c["four_events_3000"] = (_few_events(3000), UNIT_SCALE)
    for seed in PIECEWISE_SEEDS:   # (22 samples per lane: always the sequential picker)
        c[f"piecewise_linear_1400_{seed}"] = (_piecewise_linear(seed), UNIT_SCALE)
    for k in range(32):   # ordinary reads of odd lengths, for a block of 32 reads that the speculative picker takes whole
        n = 4001 + 61 * k
        c[f"filler_{k}"] = (ordinary(FILLER_SEED[rna].get(k, k), n, rna), SCALE)
    return c


@functools.lru_cache(maxsize=None)
def batch_a(rna):
    """Everything in one call -> list of (name, raw, scale).  Reads 0, 31 and the last one are empty; the longest read sits in
    the first block with the shortest; reads 32 .. 63 -- one block of the two-lanes-per-read picker, half a block of the
    read-per-lane prefix sums -- are all taken by the speculative picker; every other block mixes accepted and declined
    reads; 78 reads (DNA) or 79 (RNA), no multiple of 32."""
    c = cases(rna)
    empty = (np.zeros(0, np.int16), SCALE)
    names = [n for n in c if not n.startswith("filler_")]
    first = ["len_18433", "len_1", "len_4097", "dense_18432", "len_1473", "constant_1600", "len_33", "quantised_6000", "len_1472",
             "tiny_offset_1600", "len_18432", "range_inf_6000", "len_64", "four_events_6000", "len_1536", "zero_pa_6000"]
    rest = [n for n in names if n not in first]
    order = [("empty_first", empty)] + [(n, c[n]) for n in first + rest[:14]] + [("empty_middle", empty)]
    assert len(order) == 32
    order += [(f"filler_{k}", c[f"filler_{k}"]) for k in range(32)]
    order += [(n, c[n]) for n in rest[14:]] + [("empty_last", empty)]
    assert len(order) % 32 != 0
    return [(n, r, s) for n, (r, s) in order]


def batch_b(rna):
    """One read alone."""
    raw, sc = cases(rna)["len_4097"]
    return [("len_4097", raw, sc)]


@functools.lru_cache(maxsize=None)
def batch_c(rna, n_reads):
    """8192 or 8193 reads of 40 .. 1600 samples, most of them 40, ten ordinary 1600-sample reads among them (at 8192 reads
    the speculative picker still runs and takes those; one read more and the batch is not offered to it)."""
    out = []
    short = ordinary("c", 40, rna)
    ten = {137 + 811 * k: k for k in range(10)}
    for i in range(n_reads):
        if i in ten:
            out.append((f"ordinary_1600_{ten[i]}", ordinary(("c", MANY_ORDINARY_SEEDS[rna][ten[i]]), 1600, rna, SHORT_CHUNK_DWELL[rna]), SCALE))
        elif i % 97 == 5:
            n = 40 + (i * 37) % 1560
            out.append((f"len_{n}", ordinary(("c", i), n, rna), SCALE))
        else:
            out.append(("len_40", short, SCALE))
    return out


def pack(batch):
    """-> raw (concatenated), raw_off int64[n + 1], scaling float64[n, 3]"""
    raws = [r for _, r, _ in batch]
    off = np.concatenate([[0], np.cumsum([len(r) for r in raws])]).astype(np.int64)
    raw = np.concatenate(raws) if off[-1] else np.zeros(0, np.int16)
    return raw, off, np.array([s for _, _, s in batch], np.float64)


@functools.lru_cache(maxsize=None)
def model_a(rna):
    """The model's account of every read of batch (a), computed once: events_model.detect() plus spec = (accepted, reason),
    spec_start (what the speculative picker would write, None where it declines), spec_stats (events_model.spec_walk's) and
    cert = (exact, margin)."""
    from tests import events_model as M
    p = M.params(rna)
    out = []
    for name, raw, sc in batch_a(rna):
        d = M.detect(raw, sc, rna)
        d["spec_stats"] = {}
        ok, why, d["spec_start"] = M.spec_walk(d["t1"], d["t2"], len(raw), p, d["spec_stats"])
        d["spec"] = (ok, why)
        d["cert"] = M.certificate(raw, sc)
        out.append(d)
    return out


def same_bits(a, b):
    """float32 arrays equal as bits, NaN equal to NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def host_events(raw, sc, rna):
    """The host twin's event table of one read."""
    import sigfish_amd as S
    if len(raw) == 0:
        return np.zeros(0, S.EVENT_DTYPE)
    return S.detect_events(raw, dict(digitisation=sc[0], offset=sc[1], range=sc[2]), rna)


@functools.lru_cache(maxsize=None)
def host_a(rna):
    return [host_events(raw, sc, rna) for _, raw, sc in batch_a(rna)]
