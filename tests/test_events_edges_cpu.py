"""The inputs of tests/test_events_edges_gpu.py are what they claim to be -- without a GPU.

tests/events_model.py restates the event detection kernels in numpy; here it is held against the host twin
(S.detect_events, itself pinned to the compiled reference) on every read of batch (a), and asked which route the kernels have to
take for every read, so that the GPU test cannot pass vacuously: enough reads accepted by the speculative peak picker, reads
declined for each reason, both verdicts of the prefix sums' exactness certificate, all far from the verdict's edge."""
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from oracle import oracle as O
from tests import events_edge_cases as E
from tests import events_model as M
from tests.util import GOLD, write_blow5

CHEM = [pytest.param(False, id="dna"), pytest.param(True, id="rna")]
# reads outside the compiled reference's domain (see test_host_twin_equals_compiled_reference_on_the_edge_reads)
REF_ABORTS = {False: ("constant", "zero_pa", "four_events", "int16_extremes"),
              True: ("constant", "zero_pa", "four_events", "int16_extremes", "dense", "full_lists")}


@pytest.mark.parametrize("rna", CHEM)
def test_model_equals_host_twin(rna):
    for (name, raw, sc), m, ev in zip(E.batch_a(rna), E.model_a(rna), E.host_a(rna)):
        assert np.array_equal(m["start"], ev["start"].astype(np.int64)), name
        for f in ("length", "mean", "stdv"):
            assert E.same_bits(m[f], ev[f]), (name, f)


@pytest.mark.parametrize("rna", CHEM)
def test_speculative_walk_of_the_model_is_the_sequential_one(rna):
    """Where the model of ev_peaks_spec_kernel accepts a read, what it assembles from the 64 lanes is the sequential walk's
    result (the kernel's own claim, checked on the model before it is checked on the GPU)."""
    n_acc = 0
    for (name, raw, sc), m in zip(E.batch_a(rna), E.model_a(rna)):
        assert (m["spec_start"] is not None) == m["spec"][0]
        if m["spec"][0]:
            n_acc += 1
            assert np.array_equal(m["spec_start"], m["start"]), name
    assert n_acc >= 20


@pytest.mark.parametrize("rna", CHEM)
def test_batch_a_takes_every_route(rna):
    batch, model = E.batch_a(rna), E.model_a(rna)
    names = [b[0] for b in batch]
    assert len(batch) % 32 != 0
    assert [i for i, b in enumerate(batch) if len(b[1]) == 0] == [0, 31, len(batch) - 1]
    lens = [len(b[1]) for b in batch]
    assert lens.index(max(lens)) < 32 and max(lens) == 18433   # the longest read in one block with the shortest
    acc = np.array([m["spec"][0] for m in model])
    why = [m["spec"][1] for m in model]
    assert acc.sum() >= 20
    assert acc[32:64].all(), [names[i] for i in range(32, 64) if not acc[i]]   # one block of ev_peaks_kernel with nothing live
    for b0 in (0, 64):   # every other block of 32 (and so of 64) mixes accepted and declined reads
        assert acc[b0:b0 + 32].any() and not acc[b0:b0 + 32].all()
    assert why.count("list") >= 2
    assert why.count("nosync") >= 2
    C = [E.chunk(n) for n in lens]
    assert [w == "range" for w in why] == [c < 24 or c > 288 for c in C]
    for n in (1473, 1536):   # 24 samples per lane, the shortest that is offered; 1473 leaves lanes 62 and 63 empty
        assert model[names.index(f"len_{n}")]["spec"] == (True, ""), n
    assert 62 * E.chunk(1473) >= 1473
    for n in (1472, 18433):
        assert model[names.index(f"len_{n}")]["spec"] == (False, "range"), n
    assert model[names.index("len_4097")]["spec"] == (False, "nosync")   # (lane 63 holds 2 samples: nothing to meet there)
    # 288 samples per lane, the longest chunk offered: the noiseless read is accepted in both chemistries.  The ordinary
    # len_18432 read is accepted for RNA only: with noise the DNA detector fires more often than a lane's lists hold.
    assert model[names.index("noiseless_18432")]["spec"] == (True, "")
    assert model[names.index("len_18432")]["spec"] == ((True, "") if rna else (False, "list"))
    # the lists hold 48 firings of the short detector per lane: more than that declines the read ...
    fires = {nm: m["spec_stats"].get("max_fires") for nm, m in zip(names, model)}
    assert model[names.index("dense_18432")]["spec"] == (False, "list") and fires["dense_18432"] > 48
    if rna:   # ... 49 do, and exactly 48 are accepted
        assert model[names.index("dense_17280")]["spec"] == (False, "list") and fires["dense_17280"] == 49
        assert model[names.index("full_lists_17000")]["spec"] == (True, "") and fires["full_lists_17000"] == 48
    else:
        assert model[names.index("dense_16000")]["spec"] == (False, "list") and fires["dense_16000"] > 48
    for k in ("four_events_6000", "four_events_3000"):
        assert len(model[names.index(k)]["start"]) == 4 and model[names.index(k)]["spec"] == (False, "nosync")
    # the certificate: both verdicts, none near the edge (the kernel sums in another order: rounding, never a factor)
    exact = np.array([m["cert"][0] for m in model])
    margin = np.array([m["cert"][1] for m in model])
    assert np.all((margin < 0.25) | (margin > 4.0))
    assert exact.any() and not exact.all()
    assert np.array_equal(exact, margin < 1.0)
    for i, nm in enumerate(names):
        if nm.startswith(("tiny_offset", "range_inf")):
            assert not exact[i], nm
    # the t-statistics tie exactly where the samples are quantised
    q = model[names.index("quantised_6000")]
    assert np.sum(q["t1"][1:] == q["t1"][:-1]) > 100


def test_long_detector_decides_across_tiles():
    """ev_peaks_kernel runs the long detector one sample behind the short one, so at the first position of a 32-sample tile it
    looks at the last sample of the previous tile, carried over in a register.  The piecewise-linear RNA reads are the ones
    where that matters: with the long statistic of those samples lost (0 instead), the model's walk gives other events."""
    p = M.RNA
    batch, model = E.batch_a(True), E.model_a(True)
    for seed in E.PIECEWISE_SEEDS:
        i = [b[0] for b in batch].index(f"piecewise_linear_1400_{seed}")
        m, n = model[i], len(batch[i][1])
        assert m["spec"] == (False, "range")
        t2 = m["t2"].copy()
        t2[31::32] = 0
        assert not np.array_equal(M.walk(m["t1"], t2, n, p), m["start"]), seed


@pytest.mark.parametrize("rna", CHEM)
def test_batch_c_ordinary_reads_are_accepted(rna):
    p = M.params(rna)
    for n_reads in (8192, 8193):
        batch = E.batch_c(rna, n_reads)
        assert len(batch) == n_reads and sum(len(b[1]) for b in batch) < 1_000_000
        ten = [b for b in batch if b[0].startswith("ordinary_1600")]
        assert len(ten) == 10 and sum(len(b[1]) == 40 for b in batch) > n_reads * 0.9
    for name, raw, sc in ten:
        t1, t2 = M.tstats(raw, sc, p)
        assert M.spec_accepts(t1, t2, len(raw), p) == (True, ""), name


@pytest.mark.skipif(not os.path.exists(O.REF_DRIVER), reason="oracle/_ref not built (no /root/reference)")
@pytest.mark.parametrize("rna", CHEM)
def test_host_twin_equals_compiled_reference_on_the_edge_reads(rna, tmp_path):
    """The reads of batch (a) with at least 1000 samples and finite scaling, through the compiled reference: event counts and
    query windows as in tests/test_host_vs_reference_random.py.  Left out are the reads the reference cannot take at all: on a
    signal whose windows have no spread (constant, all-zero, the noiseless four-event reads, runs of int16 extremes, RNA's
    periodic pattern) it aborts in trim_raw_by_mad (src/events.c:246, `rt.end > rt.start`) before it detects anything, or, for
    the extremes, in create_event (src/events.c:463, `start < nsample`) depending on what else is in the file."""
    reads = [(name, sc[0], sc[1], sc[2], 4000.0, raw) for name, raw, sc in E.batch_a(rna)
             if len(raw) >= 1000 and np.isfinite(sc).all() and not name.startswith(REF_ABORTS[rna])]
    assert len(reads) >= 45
    blow5 = str(tmp_path / "edges.blow5")
    write_blow5(blow5, reads, attrs=(("experiment_type", "rna" if rna else "genomic_dna"), ("sequencing_kit", "unknown")))
    k = 5 if rna else 6
    fasta = os.path.join(GOLD, "data", "rnasequin_sequences_2.4.fa" if rna else "nCoV-2019.reference.fasta")
    dump = str(tmp_path / "dump.bin")
    subprocess.run([O.REF_DRIVER, "--model", os.path.join(GOLD, "models", f"syn{k}.f32"), "--kmer", str(k), "--dump", dump,
                    *(["--rna"] if rna else []), fasta, blow5], check=True, capture_output=True)
    d = O.parse_dump(dump)
    assert len(d["reads"]) == len(reads)
    checked = 0
    for want, (rid, dig, off, rng_, rate, raw) in zip(d["reads"], reads):
        meta = dict(digitisation=dig, offset=off, range=rng_)
        ev = S.detect_events(raw, meta, rna)
        if want["valid"]:
            assert want["n_events"] == len(ev), rid
        keep, a, b = (False, 0, 0)
        if len(ev):
            keep, a, b = S.select_query(ev, raw, meta, 50, 250, S.RNA if rna else 0, 0)
        assert keep == want["valid"], rid
        if keep:
            assert (a, b) == (want["qstart"], want["qend"]), rid
            assert np.array_equal(ev["mean"][a:b].view(np.uint32), want["query"].view(np.uint32)), rid
            assert int(ev["start"][a]) == want["ev_start_first"] and int(ev["start"][b - 1]) == want["ev_start_last"]
            assert np.float32(ev["length"][b - 1]) == want["ev_len_last"]
            checked += 1
    assert checked > 40
