"""synth.make_dna_raw_reads_truth: the reads of make_dna_raw_reads bit for bit for the same seed, and a truth whose interval is what
the read was built from -- without noise, the read's runs of equal samples are the quantised levels of the interval's k-mers in
order ('-': of its reverse complement), on both strands, for reads clipped at a contig's end and for direct RNA; write_truth_paf
against api.read_truth."""
import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import synth

K = 6
LEVELS = synth.kmer_levels(K, 21)
RECORDS = [("c0", synth.random_sequence(905, 1)), ("c1", synth.random_sequence(405, 2)), ("c2", synth.random_sequence(3000, 3))]
KINDS = ("mapped", "mapped", "random", "mapped", "stalled", "flat")


@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna"])
@pytest.mark.parametrize("kw", [dict(), dict(kinds=KINDS, samples=(500, 4000)), dict(noise=0.0, dwell=(3, 5), kinds=("mapped", "random"))], ids=["defaults", "kinds", "no_noise"])
def test_the_reads_are_make_dna_raw_reads_bit_for_bit(kw, rna):
    plain = synth.make_dna_raw_reads(RECORDS, LEVELS, K, 60, seed=11, rna=rna, **kw)
    reads, truth = synth.make_dna_raw_reads_truth(RECORDS, LEVELS, K, 60, seed=11, rna=rna, **kw)
    assert len(reads) == len(truth) == len(plain) == 60
    for a, b in zip(plain, reads):
        assert a[:5] == b[:5] and a[5].dtype == b[5].dtype == np.int16 and np.array_equal(a[5], b[5])
    kinds = kw.get("kinds", ("mapped",))
    for r, where in enumerate(truth):
        assert (where is None) == (kinds[r % len(kinds)] != "mapped"), (r, where)


def collapse(x):
    x = np.asarray(x)
    return x[np.concatenate([[True], x[1:] != x[:-1]])]


def quantised(levels):
    m = synth.R9_DNA_META
    return np.clip(np.round(levels.astype(np.float64) * m["digitisation"] / m["range"] - m["offset"]), -32768, 32767).astype(np.int16)


def levels_of(seq):
    code = {c: i for i, c in enumerate("ACGT")}
    return np.array([LEVELS[sum(code[c] * 4 ** (K - 1 - j) for j, c in enumerate(seq[i:i + K]))] for i in range(len(seq) - K + 1)], np.float32)


@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna"])
def test_the_interval_holds_the_levels_the_read_was_built_from(rna):
    comp = str.maketrans("ACGT", "TGCA")
    reads, truth = synth.make_dna_raw_reads_truth(RECORDS, LEVELS, K, 120, seed=5, samples=(300, 6000), noise=0.0, rna=rna)
    strands, clipped, whole = set(), 0, 0
    for (rid, _, _, _, _, raw), (c, b, e, strand) in zip(reads, truth):
        seq = RECORDS[c][1]
        assert 0 <= b < e <= len(seq) and e - b >= K, (rid, b, e)
        part = seq[b:e]
        lv = levels_of(part.translate(comp)[::-1]) if strand == "-" else levels_of(part)
        if rna:  # the molecule passes 3' to 5': the forward k-mers backwards
            assert strand == "+"
            lv = lv[::-1]
        want, got = collapse(quantised(lv)), collapse(raw)
        assert len(want) <= len(got) and np.array_equal(got[:len(want)], want), (rid, c, b, e, strand)
        # the interval is no shorter than the read: a read inside its contig is its interval's levels and nothing else; one that ran
        # off the contig's end goes on with random k-mers, and its interval ends where the contig does in the read's direction
        ran_off = (b == 0) if (strand == "-" or rna) else (e == len(seq))
        if len(got) > len(want):
            assert ran_off, (rid, c, b, e, strand, len(got), len(want))
            clipped += 1
        else:
            whole += 1
        strands.add(strand)
    assert strands == ({"+"} if rna else {"+", "-"}) and clipped >= 5 and whole >= 40


def test_write_truth_paf_and_read_truth(tmp_path):
    reads, truth = synth.make_dna_raw_reads_truth(RECORDS, LEVELS, K, 24, seed=2, kinds=KINDS)
    names, lengths = [n for n, _ in RECORDS], [len(s) for _, s in RECORDS]
    path = str(tmp_path / "truth.paf")
    synth.write_truth_paf(path, reads, truth, names, lengths)
    got = S.read_truth(path, names)
    assert len(got) == 24
    for (rid, *_), where in zip(reads, truth):
        assert got[rid] == ((-1, 0, 0) if where is None else where[:3])
    lines = open(path).read().splitlines()
    assert all(len(ln.split("\t")) == 12 for ln in lines)
    first = lines[0].split("\t")
    assert first[0] == reads[0][0] and first[4] == truth[0][3] and first[5] == names[truth[0][0]] and int(first[6]) == lengths[truth[0][0]]
