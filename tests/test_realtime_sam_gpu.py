"""realtime.replay(sam=True) on the GPU: a decided channel's SAM record, from the maps of Session.event_maps.
  * with the defaults of `realtime` (normalisation over the whole query, never early) the records without their three tags are
    the records `sigfish-amd dtw --sam` prints, i.e. the compiled reference's golden output (header lines are not compared);
  * on the synthetic three-contig workload every record of an early, full or end-of-read decision equals a per-read
    restatement: api.r2qevent_map on the events the slot had at its decision (the host twin fed the same chunks).
Text and integers: no tolerance anywhere."""
import os
import re
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime
from tests.realtime_util import BIN, strip_tags, tags, write_model
from tests.test_realtime_gpu import synthetic  # noqa: F401  (the fixture: three contigs, 60 raw reads of every kind)
from tests.test_session_raw_gpu import Twin
from tests.util import load_case

pytestmark = pytest.mark.gpu

# reads of the fixtures with fewer than p + q events.  Every read of both fixtures has at least 830 events (the note in
# tests/test_realtime_gpu.py) and both cases run with the defaults p = 50, q = 250, so none is
EXEMPT = {"dna_sam": [], "rna_sam": []}


def dtw_unprintable(c, model):
    """the mapped rows `dtw --sam` reports as having no SAM record for the case (its warning on stderr; none: 0)"""
    r = subprocess.run([BIN, "dtw", "--kmer-model", model, "--verbose", "1", *[str(a) for a in c["args"]], c["fasta"], c["blow5"]], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    m = re.search(r"WARNING: (\d+) mapped row\(s\) have no SAM record", r.stderr.decode())
    return int(m.group(1)) if m else 0


@pytest.mark.parametrize("name", ["dna_sam", "rna_sam"])
def test_defaults_equal_dtw_sam(name, tmp_path):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    c = load_case(name)
    args = [str(a) for a in c["args"]]
    p, q = c["prefix_size"], c["query_size"]
    assert p + q < 830 and EXEMPT[name] == []  # no read is too short to be calibrated: none is exempt
    resweep = bool(c["flag"] & S.RNA) and "--invert" not in args  # the query is the events reversed: swept again, not extended
    ref = S.RefModel.from_fasta(c["fasta"], c["levels"], c["k"], c["flag"], q)
    reads = list(S.Blow5File(c["blow5"]))
    want = sorted((ln + "\n" for ln in c["out_text"].splitlines() if ln and not ln.startswith("@")), key=lambda ln: ln.split("\t")[0])
    with S.Aligner(ref, c["flag"]) as al:
        for channels, chunk in ((2, 1600), (8, 333)):
            lines, refused, n_mapped = [], 0, 0
            for item in realtime.replay(al, reads, channels, chunk, p, q, q, q, 61, resweep=resweep, sam=True):
                tick, ch, index, row, info, span, why, sam = item
                rid, _, raw = reads[index]
                text, ref_n = realtime.format_sam(rid, ref.names, row, info, why, sam, c["flag"])
                n_mapped += realtime.mapped(row)
                refused += ref_n
                if text:
                    assert tags(text) == (q, int(info["n_samples"]), "F")
                    lines.append(text)
            assert strip_tags("".join(lines)) == want, (channels, chunk)
            assert len(lines) + refused == n_mapped
            counts = (refused, n_mapped)
        model = write_model(tmp_path / "syn.model", c["k"])
        assert counts[0] == dtw_unprintable(c, model)  # records sam_row_from_map refuses are absent from the golden too


def test_synthetic_records_equal_the_per_read_restatement(synthetic):  # noqa: F811
    skip, norm, query, min_events, min_mapq, channels, chunk = 3, 25, 70, 30, 5, 7, 800
    reads = list(S.Blow5File(synthetic["blow5"]))
    ref = synthetic["ref"]
    reasons, n_records, n_cand_records = set(), 0, 0
    with S.Aligner(ref, 0) as al:
        plain = [realtime.format_line(reads[it[2]][0], len(reads[it[2]][2]), ref.names, ref.seq_lengths, it[3], it[4], it[5], it[6])
                 for it in realtime.replay(al, reads, channels, chunk, skip, norm, query, min_events, min_mapq)]
        items = list(realtime.replay(al, reads, channels, chunk, skip, norm, query, min_events, min_mapq, sam=True))
        assert len(items) == len(plain) == 60
        for it, paf in zip(items, plain):
            tick, ch, index, row, info, span, why, sam = it
            rid, _, raw = reads[index]
            text, refused = realtime.format_sam(rid, ref.names, row, info, why, sam, 0)
            assert refused == 0 and bool(text) == bool(paf)  # schedule and decision rule are those of the PAF replay
            if not text:
                continue
            assert tags(text) == tags(paf) == (int(info["q_events"]), int(info["n_samples"]), why)
            # the host twin of the slot, fed the same chunks up to the decision
            sent = int(info["n_samples"])
            tw = Twin(False, (skip, norm, query))
            for a in range(0, sent, chunk):
                tw.feed(raw[a:a + chunk], a + chunk > len(raw))
            qn = tw.query_so_far()
            n_q = int(info["q_events"])
            assert qn is not None and len(qn) == n_q
            ev = tw.final().copy()
            ev["mean"][skip:skip + n_q] = qn
            j, plus = int(row["rid"]), row["strand"] == ord("+")
            host = S.r2qevent_map(row, ev, skip, skip + n_q, ref.forward[j] if plus else ref.reverse[j], int(ref.st_offset[j]), 0)
            assert np.array_equal(sam["map"], host), (rid, why)
            assert text == realtime.format_sam_line(rid, ref.names, row, info, why, ev, skip, skip + n_q, host, 0), (rid, why)
            reasons.add(why)
            n_records += 1
        assert reasons == {"E", "F", "R"} and n_records >= 30, (reasons, n_records)  # (about this test's own inputs)
        # with candidates: the valid candidates' records follow as secondaries, from the same call's maps
        for it in realtime.replay(al, reads[:14], channels, chunk, skip, norm, query, min_events, min_mapq, candidates=2, sam=True):
            tick, ch, index, row, info, span, why, cand, sam = it
            rid, _, raw = reads[index]
            text, refused = realtime.format_sam(rid, ref.names, row, info, why, sam, 0, cand=cand)
            if not text:
                continue
            recs = text.splitlines()
            n_valid = sum(realtime.mapped(r) for r in cand)
            assert refused == 0 and len(recs) == 1 + n_valid and n_valid <= 2
            ev, qs, qe = sam["events"], sam["qstart"], sam["qend"]
            stats = (info["norm_mean"], info["norm_sd"])
            evn = ev.copy()
            evn["mean"][qs:qe] = ((ev["mean"][qs:qe] - np.float32(stats[0])) / np.float32(stats[1])).astype(np.float32)
            for k, r in enumerate(c for c in cand if realtime.mapped(c)):
                j, plus = int(r["rid"]), r["strand"] == ord("+")
                host = S.r2qevent_map(r, evn, qs, qe, ref.forward[j] if plus else ref.reverse[j], int(ref.st_offset[j]), 0)
                assert recs[1 + k] + "\n" == realtime.format_sam_line(rid, ref.names, r, info, why, ev, qs, qe, host, 0, True)
                assert int(recs[1 + k].split("\t")[1]) & 256
                n_cand_records += 1
        assert n_cand_records >= 4, n_cand_records  # (about this test's own inputs)
