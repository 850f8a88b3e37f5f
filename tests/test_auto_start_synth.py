"""The RNA poly-A read generator (synth.make_rna_polya_reads) and the host route of the automatic query start (-p -1:
detect_events -> detect_query_start / select_query) against the COMPILED REFERENCE: same windows, same normalised
queries, same PAF.  The device route is compared with this host route on the GPU (tests/test_auto_start_gpu.py).
The reference's driver never sets pore_flag, so this covers pore 0 only."""
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from oracle import oracle as O
from sigfish_amd import synth
from tests.util import GOLD, write_blow5


def test_generator_is_seeded_and_covers_every_kind():
    a = synth.make_rna_polya_reads(200, seed=3)
    b = synth.make_rna_polya_reads(200, seed=3)
    assert [r[0] for r in a] == [r[0] for r in b] and all(np.array_equal(x[5], y[5]) for x, y in zip(a, b))
    kinds = {r[0].split("_", 3)[3] for r in synth.make_rna_polya_reads(600, seed=4)}
    assert kinds == set(synth.RNA_POLYA_KINDS)
    for kind, n in (("n2000", 2000), ("n2001", 2001)):
        assert {len(r[5]) for r in synth.make_rna_polya_reads(5, seed=1, kinds=(kind,))} == {n}


@pytest.mark.parametrize("pore", [0, 2])
def test_host_query_start_finds_and_misses(pore):
    """detect_query_start on the generator's reads: most find a start behind the tail, the fallback kinds do not"""
    reads = synth.make_rna_polya_reads(400, seed=9, pore=pore)
    found = miss = 0
    for rid, dig, off, rng_, rate, raw in reads:
        meta = dict(digitisation=dig, offset=off, range=rng_)
        ev = S.detect_events(raw, meta, True)
        if len(ev) == 0:
            continue
        st = S.detect_query_start(raw, meta, ev, pore)
        kind = rid.split("_", 3)[3]
        if kind in ("n2000", "n2001"):  # (a body can hold an adaptor-like dip, so "no_adaptor" may still find one)
            assert st == -1, rid
        found += st >= 0
        miss += st < 0
        if st >= 0:  # the start is the reference's: the window select_query picks begins there
            keep, a, b = S.select_query(ev.copy(), raw, meta, -1, 500, S.RNA, pore)
            assert a == st or not keep
    assert found >= len(reads) // 2 and miss >= len(reads) // 10, (found, miss)


@pytest.mark.skipif(not os.path.exists(O.REF_DRIVER), reason="oracle/_ref not built (reference tree absent)")
def test_host_route_matches_reference_on_synthetic_reads(tmp_path):
    # (constant reads and non-finite scaling are outside the reference's domain: trim_raw_by_mad asserts, src/events.c:246)
    reads = [r for r in synth.make_rna_polya_reads(330, seed=21, pore=0) if r[0].split("_", 3)[3] not in ("constant", "nonfinite")]
    blow5 = str(tmp_path / "polya.blow5")
    write_blow5(blow5, reads, attrs=(("experiment_type", "rna"), ("sequencing_kit", "unknown")), compress=True)
    dump = str(tmp_path / "dump.bin")
    paf = subprocess.run([O.REF_DRIVER, "--model", os.path.join(GOLD, "models", "syn5.f32"), "--kmer", "5", "--dump", dump, "--rna",
                          "-p", "-1", "-q", "500", os.path.join(GOLD, "data", "rnasequin_sequences_2.4.fa"), blow5],
                         check=True, capture_output=True).stdout.decode()
    d = O.parse_dump(dump)
    assert len(d["reads"]) == len(reads)
    checked = fell_back = 0
    for want, (rid, dig, off, rng_, rate, raw) in zip(d["reads"], reads):
        meta = dict(digitisation=dig, offset=off, range=rng_)
        ev = S.detect_events(raw, meta, True)
        if want["valid"]:
            assert want["n_events"] == len(ev), rid
        keep, a, b = (False, 0, 0)
        if len(ev):
            fell_back += S.detect_query_start(raw, meta, ev, 0) < 0
            keep, a, b = S.select_query(ev, raw, meta, -1, 500, S.RNA, 0)
        assert keep == want["valid"], rid
        if keep:
            assert (a, b) == (want["qstart"], want["qend"]), rid
            assert np.array_equal(ev["mean"][a:b].view(np.uint32), want["query"].view(np.uint32)), rid
            checked += 1
    assert checked > 150 and fell_back > 20, (checked, fell_back)
    # the PAF of the host route's windows (alignment by the oracle's restatement) is the reference's
    valid = [(w, r) for w, r in zip(d["reads"], reads) if w["valid"]]
    q = np.concatenate([w["query"] for w, _ in valid])
    q_off = np.concatenate([[0], np.cumsum([len(w["query"]) for w, _ in valid])]).astype(np.int64)
    rows = O.align_batch(q, q_off, d["ref"], d["flag"], threads=8)
    lines = []
    for (w, (rid, dig, off, rng_, rate, raw)), r in zip(valid, rows):
        end_raw = int(np.float32(np.float32(w["ev_start_last"]) + w["ev_len_last"]))
        lines.append(S.paf_row(r, rid, d["ref"].names[int(r["rid"])], w["ev_start_first"], end_raw, (w["qend"] - 1) - w["qstart"], len(raw),
                               int(d["ref"].seq_lengths[int(r["rid"])])))
    assert "".join(lines) == paf
