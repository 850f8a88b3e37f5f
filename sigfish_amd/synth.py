"""Synthetic workloads at the alignment-stage boundary: seeded k-mer models, random references,
and reads drawn from the reference event arrays with over-segmentation and noise.  numpy only; used by bench.py
and the tests to produce inputs of the BASELINE.json shapes (there is no network for real datasets)."""
import numpy as np

from . import api


def kmer_levels(k, seed, mu=90.0, sd=12.0):
    """Seeded synthetic k-mer model: level_mean ~ N(mu, sd), lexicographic ACGT order."""
    rng = np.random.default_rng(seed)
    return rng.normal(mu, sd, size=4 ** k).astype(np.float32)


def random_sequence(n, seed):
    rng = np.random.default_rng(seed)
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, size=n)])


def _znorm_rows(q):
    """Row-wise z-normalisation with the reference's sequential fp32 recipe (src/sigfish.c:483-502)."""
    q = np.ascontiguousarray(q, np.float32)
    n = np.float32(q.shape[1])
    mean = (np.cumsum(q, axis=1, dtype=np.float32)[:, -1] / n).astype(np.float32)
    d = (q - mean[:, None]).astype(np.float32)
    var = (np.cumsum(d * d, axis=1, dtype=np.float32)[:, -1] / n).astype(np.float32)
    sd = np.sqrt(var).astype(np.float32)
    return ((q - mean[:, None]) / sd[:, None]).astype(np.float32)


def make_reads(ref: "api.RefModel", n_reads, qlen=250, seed=0, short_frac=0.05, noise=0.35, min_len=25):
    """Returns (queries float32[sum qlen], q_off int64[n+1], truth dict).

    Each read follows consecutive reference levels from a random (contig ∝ length, strand, start), every level
    repeated 1+Poisson(0.5) times (over-segmentation), plus N(0, noise²) in z-units, then z-normalised.
    `short_frac` of the reads are truncated to a length in [min_len, qlen) to exercise the ragged path.
    For RNA models (single strand) the event order is reversed, as the sequencer reads 3'->5'."""
    rng = np.random.default_rng(seed)
    rna = ref.reverse is None
    lens = ref.ref_lengths.astype(np.int64)
    contig = rng.choice(ref.num_ref, size=n_reads, p=lens / lens.sum())
    strand = np.zeros(n_reads, np.int8) if rna else rng.integers(0, 2, size=n_reads).astype(np.int8)
    # dwell -> k-mer index of each of the qlen events
    dwell = 1 + rng.poisson(0.5, size=(n_reads, qlen))
    cum = np.cumsum(dwell, axis=1)
    flags = np.zeros((n_reads, qlen + 1), np.int32)
    rows = np.repeat(np.arange(n_reads), qlen)
    cols = np.minimum(cum, qlen).ravel()
    flags[rows, cols] = 1  # cum is strictly increasing, so only the unused column qlen can repeat
    kidx = np.cumsum(flags[:, :qlen], axis=1)  # 0-based k-mer step of each event
    span = kidx[:, -1] + 1
    room = np.maximum(lens[contig] - span, 1)
    start = (rng.random(n_reads) * room).astype(np.int64)
    pos = np.minimum(start[:, None] + kidx, (lens[contig] - 1)[:, None])
    # gather levels from a flat copy of the arrays
    offs = np.concatenate([[0], np.cumsum(lens)])[:-1]
    flat_f = np.concatenate(ref.forward)
    flat = flat_f if rna else np.stack([flat_f, np.concatenate(ref.reverse)])
    base = offs[contig][:, None] + pos
    lv = flat[base] if rna else flat[strand[:, None].astype(np.int64), base]
    q = lv + rng.normal(0.0, noise, size=lv.shape).astype(np.float32)
    if rna:
        q = q[:, ::-1]
    q = _znorm_rows(q)
    # ragged tail: a fraction of reads keeps only their first L events (re-normalised)
    qlens = np.full(n_reads, qlen, np.int64)
    n_short = int(round(short_frac * n_reads)) if qlen > min_len else 0
    if n_short:
        which = rng.choice(n_reads, size=n_short, replace=False)
        qlens[which] = rng.integers(min_len, qlen, size=n_short)
    q_off = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int64)
    out = np.empty(int(q_off[-1]), np.float32)
    full = qlens == qlen
    # fast path: full-length rows are contiguous copies
    idx_full = np.nonzero(full)[0]
    if len(idx_full):
        dst = (q_off[idx_full][:, None] + np.arange(qlen)[None, :]).ravel()
        out[dst] = q[idx_full].ravel()
    for i in np.nonzero(~full)[0]:
        out[q_off[i]:q_off[i + 1]] = api.znormalise(q[i, :qlens[i]])
    truth = dict(contig=contig.astype(np.int32), strand=strand, start=start.astype(np.int64), span=span.astype(np.int64))
    return out, q_off, truth


def workload(name, n_reads=None, seed=0, golden_dir=None):
    """The BASELINE.json configurations as (RefModel, flag, queries, q_off, meta)."""
    import os
    gd = golden_dir or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    import re
    m = re.fullmatch(r"ncov_r9_dna_q(\d+)", name)
    if m:  # q250 = configs[2]: synthetic R9 DNA reads x 30 kb nCoV reference, -q 250; other -q values for the long classes
        lv = kmer_levels(6, 1)
        qlen = int(m.group(1))
        ref = api.RefModel.from_fasta(os.path.join(gd, "data", "nCoV-2019.reference.fasta"), lv, 6, 0, qlen)
        flag, n = 0, n_reads or 100_000 * 250 // qlen
    elif name == "r10_dna_1mb_q250":  # configs[3]: synthetic R10 DNA reads x 1 Mb reference (k=9)
        lv = kmer_levels(9, 3)
        ref = api.RefModel.from_records([("synthetic_1Mb", random_sequence(1_000_000, 4))], lv, 9, 0, 250)
        flag, qlen, n = 0, 250, n_reads or 2_000
    elif name == "rna004_fullref_dtwstd_q250":  # configs[4]: RNA004 --full-ref --dtw-std x sequin transcriptome
        lv = kmer_levels(9, 3)
        flag = api.RNA | api.REF | api.DTW
        ref = api.RefModel.from_fasta(os.path.join(gd, "data", "rnasequin_sequences_2.4.fa"), lv, 9, flag, 250)
        qlen, n = 250, n_reads or 50_000
    elif name == "sequin_r9_rna_q250":  # configs[1] shape: R9 RNA x sequin 3'-slices
        lv = kmer_levels(5, 2, 100.0, 14.0)
        flag = api.RNA
        ref = api.RefModel.from_fasta(os.path.join(gd, "data", "rnasequin_sequences_2.4.fa"), lv, 5, flag, 250)
        qlen, n = 250, n_reads or 100_000
    else:
        raise ValueError(f"unknown workload {name}")
    q, q_off, truth = make_reads(ref, n, qlen=qlen, seed=seed)
    strands = 1 if ref.reverse is None else 2
    cells = int((q_off[1:] - q_off[:-1]).sum()) * int(ref.ref_lengths.sum()) * strands
    alg_bytes = int((4 * (q_off[1:] - q_off[:-1]) + 4 * strands * int(ref.ref_lengths.sum()) + 32).sum())
    meta = dict(name=name, n_reads=n, qlen=qlen, cells=cells, algorithmic_bytes=alg_bytes, truth=truth)
    return ref, flag, q, q_off, meta


# ---- raw RNA reads for the automatic query start (-p -1: adaptor, then poly-A tail, src/jnn.c) ----------------------------
# Calibrated on the 8 reads of tests/golden/data/sequin_rna.blow5: digitisation 2048, range 548.79 (0.268 pA per count),
# offset -227 .. -253, transcript levels around 90 pA (raw 500 .. 730), 25 k .. 90 k samples, the start found 7 k .. 20 k
# samples in.
RNA_POLYA_KINDS = ("normal", "adaptor_edge", "two_low", "polya_edge", "no_adaptor", "no_polya", "polya_at_end", "n2000",
                   "n2001", "constant", "outside", "nonfinite", "adaptor_hi")


def make_rna_polya_reads(n_reads, seed=0, pore=0, kinds=None, body=(5_000, 40_000)):
    """Seeded raw RNA reads [(read_id, digitisation, offset, range, sampling_rate, int16 samples)] in four parts: a leader
    near the open level, an adaptor stretch low in raw counts, a poly-A plateau about 30 pA above the adaptor mean (noise
    and a controlled number of out-of-band excursions), a transcript body of k-mer levels.  `kinds` (default: every kind
    of RNA_POLYA_KINDS, "normal" weighted up) picks what each read exercises: adaptor lengths around the segmenter's
    limits for `pore` (lo = 500 for RNA004, else 2000; hi = 200000), two low stretches closer and farther apart than
    seg_dist, poly-A lengths around 250 with excursions around 30, no adaptor / no poly-A, a tail ending behind the last
    event, reads of 2000 and 2001 samples, constant reads, samples outside [0, 1200], non-finite scaling."""
    rng = np.random.default_rng(seed)
    if kinds is None:
        kinds = RNA_POLYA_KINDS
        w = np.array([12.0 if k == "normal" else (0.3 if k == "adaptor_hi" else 1.0) for k in kinds])
    else:
        w = np.ones(len(kinds))
    lo = 500 if pore == 2 else 2000
    levels = kmer_levels(5, 11, 90.0, 12.0)
    dig, rng_ = 2048.0, 548.7882690429688
    unit = np.float32(rng_) / np.float32(dig)
    out = []

    def steps(n, mu, sd, dwell_lo=5, dwell_hi=40, noise=2.0):  # piecewise-constant pA with noise
        d = rng.integers(dwell_lo, dwell_hi, size=n // dwell_lo + 2)
        x = np.repeat(rng.normal(mu, sd, size=len(d)) if sd > 0 else np.full(len(d), mu), d)[:n]
        return x + rng.normal(0, noise, size=n)

    def kmer_body(n):
        d = rng.integers(5, 40, size=n // 5 + 2)
        return np.repeat(levels[rng.integers(0, len(levels), size=len(d))], d)[:n] + rng.normal(0, 2.0, size=n)

    def polya(n, level, n_exc):
        x = level + rng.normal(0, rng.uniform(1.0, 3.5), size=n)
        if n_exc > 0 and n > 0:  # excursions out of the +-20 pA band, in short clusters
            at = rng.choice(n, size=min(n_exc, n), replace=False)
            x[at] = level + rng.choice([-1, 1], size=len(at)) * rng.uniform(22, 40, size=len(at))
        return x

    for r in range(n_reads):
        kind = kinds[rng.choice(len(kinds), p=w / w.sum())]
        off = float(rng.integers(-253, -226))
        scale_rng = rng_
        ad_lvl = rng.uniform(52, 75)
        leader = steps(int(rng.integers(0, 3000)), rng.uniform(105, 120), 3.0)
        ad_len = int(rng.integers(lo + 1500, lo + 9000))
        pa_len = int(rng.integers(300, 2500))
        n_exc = int(rng.integers(0, 25))
        bl = int(rng.integers(*body))
        pa = None
        if kind == "adaptor_edge":  # the rolling mean stays low for about (adaptor - 2000 + a few hundred) samples
            ad_len = int(rng.integers(max(lo - 500, 100), lo + 3000))
        elif kind == "adaptor_hi":
            ad_len = int(rng.integers(201_000, 203_500))
            bl = int(rng.integers(3000, 8000))
        elif kind == "polya_edge":
            pa_len = int(rng.integers(180, 330))
            n_exc = int(rng.integers(15, 50))
        if kind == "two_low":  # a gap at transcript level between two adaptor-like stretches
            gap = int(rng.integers(200, 4500))
            a1 = steps(int(rng.integers(lo // 2, lo + 4000)), ad_lvl, 2.0)
            pa = np.concatenate([leader, a1, kmer_body(gap), steps(ad_len, ad_lvl, 2.0), polya(pa_len, ad_lvl + 30, n_exc), kmer_body(bl)])
        elif kind == "no_adaptor":
            pa = np.concatenate([leader, kmer_body(bl + 8000)])
        elif kind == "no_polya":
            pa = np.concatenate([leader, steps(ad_len, ad_lvl, 2.0), kmer_body(bl)])
        elif kind == "polya_at_end":
            pa = np.concatenate([leader, steps(ad_len, ad_lvl, 2.0), polya(pa_len, ad_lvl + 30, n_exc), kmer_body(int(rng.integers(0, 40)))])
        elif kind in ("n2000", "n2001"):
            n = 2000 if kind == "n2000" else 2001
            pa = np.concatenate([steps(600, ad_lvl, 2.0), polya(400, ad_lvl + 30, 0), kmer_body(n - 1000)])
        elif kind == "constant":
            pa = np.full(int(rng.integers(3000, 30000)), rng.uniform(60, 110))
        else:
            pa = np.concatenate([leader, steps(ad_len, ad_lvl, 2.0), polya(pa_len, ad_lvl + 30, n_exc), kmer_body(bl)])
        raw = np.round(pa / unit - off)
        if kind == "outside":  # clamp_outlier territory: spikes below 0 and above 1200 raw counts
            at = rng.choice(len(raw), size=max(1, len(raw) // 200), replace=False)
            raw[at] = rng.choice([-400.0, -5.0, 1250.0, 3000.0], size=len(at))
        raw = np.clip(raw, -32768, 32767).astype(np.int16)
        if kind == "nonfinite":  # range beyond fp32: raw_unit = inf, pA = +-inf or NaN
            scale_rng = 1e39
        out.append((f"polya_{seed}_{r}_{kind}", dig, off, scale_rng, 3000.0, raw))
    return out


# ---- raw DNA reads and a BLOW5 file of them (the replay of `sigfish-amd realtime`, tools/realtime_replay.py) ---------------
R9_DNA_META = dict(digitisation=8192.0, offset=6.0, range=1467.61, sampling_rate=4000.0)
RAW_DNA_KINDS = ("mapped", "random", "stalled", "flat")


def make_dna_raw_reads(records, level_mean, k, n_reads, seed=0, samples=(2000, 9000), dwell=(6, 13), noise=1.5, kinds=("mapped",), meta=R9_DNA_META, rna=False):
    """Seeded raw DNA reads [(read_id, digitisation, offset, range, sampling_rate, int16 samples)] over [(name, sequence)] and a
    4^k table of level means (pA).  Read r is of kind kinds[r % len(kinds)]:
      mapped  the levels of consecutive k-mers from a random (contig, strand, start), each held for dwell[0] .. dwell[1] - 1
              samples, plus N(0, noise); behind the contig's end the read goes on with random k-mers
      random  random k-mers all the way: a signal that belongs nowhere
      stalled random k-mers for 200 .. 330 samples, then one level without noise: the events stop long before the read does
      flat    one level, no noise: the detector finds no event
    rna: direct RNA instead -- a mapped read follows the forward strand only, from its start k-mer BACKWARDS (the molecule passes
    the pore 3' to 5', which is why the reference takes the query reversed, src/sigfish.c:860-863)."""
    return _dna_raw_reads(records, level_mean, k, n_reads, seed, samples, dwell, noise, kinds, meta, rna)[0]


def make_dna_raw_reads_truth(records, level_mean, k, n_reads, seed=0, samples=(2000, 9000), dwell=(6, 13), noise=1.5, kinds=("mapped",), meta=R9_DNA_META, rna=False):
    """make_dna_raw_reads that knows where its reads came from -> (reads, truth): the same reads for the same arguments, and per read
    (contig index, begin, end, strand) or None for the kinds that belong nowhere (random, stalled, flat).  [begin, end) are the bases
    the k-mers the read was built from cover ON THE FORWARD STRAND, also for a '-' read: the k-mers whose level reached at least one
    sample, so the interval ends where the read's samples do; a read that runs off its contig's end (and goes on with random
    k-mers) is clipped to the contig."""
    return _dna_raw_reads(records, level_mean, k, n_reads, seed, samples, dwell, noise, kinds, meta, rna)


def _dna_raw_reads(records, level_mean, k, n_reads, seed, samples, dwell, noise, kinds, meta, rna):
    rng = np.random.default_rng(seed)
    lv = np.asarray(level_mean, np.float32)
    code = np.full(256, 0, np.int64)
    for i, c in enumerate("ACGT"):
        code[ord(c)] = i
    comp = str.maketrans("ACGT", "TGCA")
    w = 4 ** np.arange(k - 1, -1, -1)

    def kmers(seq):
        b = code[np.frombuffer(seq.encode(), np.uint8)]
        return np.lib.stride_tricks.sliding_window_view(b, k) @ w

    fwd = [kmers(s.upper()) for _, s in records]
    rev = [kmers(s.upper().translate(comp)[::-1]) for _, s in records]
    lens = np.array([len(x) for x in fwd], np.float64)
    out, truth = [], []
    for r in range(n_reads):
        kind = kinds[r % len(kinds)]
        n = int(rng.integers(samples[0], samples[1] + 1))
        d = rng.integers(dwell[0], dwell[1], n // dwell[0] + 2)
        idx = rng.integers(0, len(lv), len(d))
        where = None
        if kind == "mapped":
            c = int(rng.choice(len(fwd), p=lens / lens.sum()))
            minus = False if rna else bool(rng.integers(0, 2))
            along = fwd[c][::-1] if rna else (rev if minus else fwd)[c]
            at = int(rng.integers(0, max(len(along) - 100, 1)))
            m = min(len(along) - at, len(d))
            idx[:m] = along[at:at + m]
            # k-mers at .. last of `along` reach a sample; k-mer i of fwd covers bases [i, i + k), k-mer i of rev and of the RNA
            # order is k-mer len - 1 - i of fwd
            last = at + min(m, int(np.searchsorted(np.cumsum(d), n)) + 1) - 1
            nk = len(along)
            where = (c, nk - 1 - last, nk - 1 - at + k, "-" if minus else "+") if (rna or minus) else (c, at, last + k, "+")
        truth.append(where)
        pa = np.full(n, lv[idx[0]], np.float64) if kind == "flat" else np.repeat(lv[idx].astype(np.float64), d)[:n]
        if kind != "flat":
            pa = pa + rng.normal(0, noise, n)
        if kind == "stalled":
            pa[int(rng.integers(200, 331)):] = lv[idx[-1]]
        raw = np.clip(np.round(pa * meta["digitisation"] / meta["range"] - meta["offset"]), -32768, 32767).astype(np.int16)
        out.append((f"raw_{seed}_{r}_{kind}", meta["digitisation"], meta["offset"], meta["range"], meta["sampling_rate"], raw))
    return out, truth


def write_truth_paf(path, reads, truth, names, lengths):
    """The truth of make_dna_raw_reads_truth as the PAF file `sigfish-amd realtime --truth` and api.read_truth take: one line per
    read -- read id, samples, 0, samples, strand, contig name, contig length, begin, end, end - begin, end - begin, 60 -- and
    `*` for the contig of a read that belongs nowhere (its coordinates 0).  names / lengths: the contigs' names and base counts."""
    with open(path, "w") as f:
        for (rid, _, _, _, _, raw), where in zip(reads, truth):
            if where is None:
                f.write(f"{rid}\t{len(raw)}\t0\t{len(raw)}\t*\t*\t0\t0\t0\t0\t0\t0\n")
            else:
                c, b, e, strand = where
                f.write(f"{rid}\t{len(raw)}\t0\t{len(raw)}\t{strand}\t{names[c]}\t{int(lengths[c])}\t{b}\t{e}\t{e - b}\t{e - b}\t60\n")


def write_blow5(path, reads, attrs=(("experiment_type", "genomic_dna"), ("sequencing_kit", "unknown"))):
    """An uncompressed BLOW5 file (layout: csrc/host/blow5.hpp) of reads = [(read_id, digitisation, offset, range, sampling_rate,
    int16 samples)], as make_dna_raw_reads and make_rna_polya_reads return them."""
    import struct
    text = "".join(f"@{k}\t{v}\n" for k, v in attrs)
    text += "#char*\tuint32_t\tdouble\tdouble\tdouble\tdouble\tuint64_t\tint16_t*\n"
    text += "#read_id\tread_group\tdigitisation\toffset\trange\tsampling_rate\tlen_raw_signal\traw_signal\n"
    hdr = b"BLOW5\x01" + bytes([0, 2, 0, 0]) + struct.pack("<I", 1) + bytes([0])
    hdr += b"\0" * (64 - len(hdr)) + struct.pack("<I", len(text)) + text.encode()
    with open(path, "wb") as out:
        out.write(hdr)
        for rid, dig, off, rng_, rate, raw in reads:
            name = rid.encode()
            raw = np.ascontiguousarray(raw, np.int16)
            payload = struct.pack("<H", len(name)) + name + struct.pack("<I4dQ", 0, dig, off, rng_, rate, len(raw)) + raw.tobytes()
            out.write(struct.pack("<Q", len(payload)) + payload)
        out.write(b"5WOLB")
