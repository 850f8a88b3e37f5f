"""The Python replay with the automatic query start (realtime.replay(skip=-1, resweep=True)) on the GPU.
  * With one final point only (auto_start_every = 0), caps above the longest fixture read, normalisation over the whole query
    and recalibration at the end, the lines are those of the compiled reference's `dtw --rna -q 500 -p -1` (golden
    rna_q500_pauto.out) once the five tags are removed.
  * With a point every 1600 samples, a window that doubles from 25 events and early decisions, a small synthetic file gives the
    lines a per-read restatement predicts (tests/autostart_oracle.py, the window rule, align_db, realtime.decide); at least one
    read found at a mid-read point (as:A:P) is decided early (dc:A:E).
The `sigfish-amd realtime` binary still refuses -p -1, so there is no binary to compare bytes with.  No tolerance anywhere."""
import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime, synth
from tests.autostart_oracle import cut
from tests.realtime_util import write_model
from tests.test_session_autostart_gpu import SlotTwin
from tests.test_session_raw_gpu import Rows
from tests.util import load_case

pytestmark = pytest.mark.gpu


def _ref(tmp_path, query):
    c = load_case("rna_q500_pauto")
    levels, k = S.read_kmer_model(write_model(tmp_path / "syn.model", c["k"]))
    return c, S.RefModel.from_fasta(c["fasta"], levels, k, S.RNA, query)


def _lines(al, ref, reads, **kw):
    out = []
    for item in realtime.replay(al, reads, **kw):
        tick, ch, index, row, info, span, why, auto = item
        out.append((realtime.format_line(reads[index][0], len(reads[index][2]), ref.names, ref.seq_lengths, row, info, span, why, auto), why, auto))
    return out


def test_final_point_only_prints_the_golden_lines(tmp_path):
    c, ref = _ref(tmp_path, 500)
    assert c["prefix_size"] == -1 and c["query_size"] == 500
    reads = list(S.Blow5File(c["blow5"]))
    longest = max(len(r[2]) for r in reads)
    with S.Aligner(ref, S.RNA) as al:
        got = _lines(al, ref, reads, channels=3, chunk_samples=1600, skip=-1, norm=500, query=500, min_events=500, min_mapq=61, at_end=True, resweep=True,
                     auto_start_every=0, auto_start_max_samples=longest + 1, max_skip_events=longest // 2)
    lines = [ln for ln, _, _ in got if ln]
    for ln in lines:
        f = ln.rstrip("\n").split("\t")
        assert f[-2].startswith("qs:i:") and f[-1] in ("as:A:E", "as:A:F") and f[-3][:5] == "dc:A:" and f[-3][5] in "FR", ln
    strip = sorted("\t".join(ln.rstrip("\n").split("\t")[:-5]) + "\n" for ln in lines)
    want = sorted(ln + "\n" for ln in c["out_text"].splitlines())
    assert strip == want and len(want) >= 5


def predict(al_rows, ref, rid, meta, raw, chunk, every, max_samples, max_skip, norm, query, at, min_events, min_mapq):
    """the line of one read: its slot's state after every tick, restated, until realtime.decide decides"""
    import tests.test_session_autostart_gpu as T
    assert (T.NORM, T.QUERY, T.AT) == (norm, query, at)  # (SlotTwin's window rule is the module's)
    t, pos = SlotTwin(meta, 0, every, max_samples, max_skip, query), 0
    while True:
        n = min(chunk, len(raw) - pos)
        t.feed(raw[pos:pos + n], n < chunk)
        pos += n
        fin = t.final()
        status = (S.RAW_CALIBRATED if t.window else 0) | (S.RAW_FULL if t.skip >= 0 and len(fin) >= t.skip + query else 0) | (S.RAW_ENDED if t.ended else 0)
        info = dict(status=status, q_events=t.window, n_samples=t.n)
        row = al_rows.rows([t.query_so_far()])[0]
        why = realtime.decide(row, info, min_events, min_mapq)
        if why:
            span = (0, 0)
            if t.window:
                last = fin[t.skip + t.window - 1]
                span = (int(fin["start"][t.skip]), int(last["start"]) + int(last["length"]))
            auto = dict(skip=t.skip, status=t.status)
            return realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why, auto)
        assert n == chunk


def test_points_every_chunk_print_the_predicted_lines(tmp_path):
    norm, query, chunk, max_samples, max_skip, min_events, min_mapq = 25, 100, 1600, 1 << 17, 4000, 50, 0
    at = tuple(S.recal_double(norm, query))
    c, ref = _ref(tmp_path, query)
    reads = [(r[0], dict(digitisation=r[1], offset=r[2], range=r[3]), r[5])
             for r in synth.make_rna_polya_reads(14, seed=2, kinds=["normal", "normal", "no_polya", "polya_edge", "n2001"], body=(3000, 6000))]
    with S.Aligner(ref, S.RNA) as al:
        got = _lines(al, ref, reads, channels=4, chunk_samples=chunk, skip=-1, norm=norm, query=query, min_events=min_events, min_mapq=min_mapq, recalibrate="double",
                     at_end=True, resweep=True, auto_start_max_samples=max_samples, max_skip_events=max_skip)
        rows = Rows(al)
        want = [predict(rows, ref, rid, meta, raw, chunk, chunk, max_samples, max_skip, norm, query, at, min_events, min_mapq) for rid, meta, raw in reads]
    assert sorted(ln for ln, _, _ in got) == sorted(want)
    assert any(ln.rstrip("\n").endswith("as:A:P") and "\tdc:A:E\t" in ln for ln in want) and any(ln.rstrip("\n").endswith("as:A:F") for ln in want)


def test_needs_resweep():
    with pytest.raises(S.SfaError, match="needs resweep"):
        next(realtime.replay(None, [], 2, 1600, -1, 25, 100, 50, 0))
