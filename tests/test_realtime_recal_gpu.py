"""`sigfish-amd realtime --recalibrate / --recalibrate-at-end` on the GPU:
  * calibrated on 25 events and recalibrated on the doubling list, a read that is not decided early prints `sigfish-amd dtw`'s
    line (the compiled reference's golden output), whatever the channels and the chunk size, and is decided full;
  * with --recalibrate-at-end a read that ends short of the query prints dtw's line too: the whole synthetic file against
    `sigfish-amd dtw` on the same file, no read exempt;
  * with early decisions the command line prints what the Python replay prints, and every early / full row is Aligner.align_db
    of the host twin's query under the window rule.
No tolerance anywhere."""
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime
from tests.realtime_util import BIN, strip_tags, tags, write_model
from tests.test_realtime_gpu import run_realtime, synthetic  # noqa: F401  (the fixture)
from tests.test_session_gpu import assert_rows
from tests.test_session_recal_gpu import RecalTwin
from tests.util import load_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["dna_default", "rna_invert"])
def test_goldens_with_a_short_calibration(name, tmp_path):
    c = load_case(name)
    model = write_model(tmp_path / "syn.model", c["k"])
    want = sorted((ln + "\n" for ln in c["out_text"].splitlines()), key=lambda ln: ln.split("\t")[0])
    for channels, chunk in ((2, 1600), (2, 333)):
        out = run_realtime(model, c["fasta"], c["blow5"], *[str(a) for a in c["args"]], "--channels", str(channels), "--chunk-samples", str(chunk), "--norm-events", "25",
                           "--min-mapq", "61", "--recalibrate", "double", "--recalibrate-at-end")
        assert strip_tags(out) == want, ((channels, chunk), out)
        for ln in out.splitlines():
            assert tags(ln)[2] == "F", ln


def test_short_reads_equal_dtw(synthetic):  # noqa: F811
    """stalled reads end with 40 .. 65 events: at their end they are normalised over all events behind -p, as dtw normalises a
    read that is too short.

    --norm-events 64 and --recalibrate-at-end alone: the command line adds q = 70 as the one point, so a full read is normalised
    over the 70 events dtw uses, and a read that ends with 25 <= events - 3 < 70 over all of them.  No read is exempt."""
    skip, query = 3, 70
    reads = list(S.Blow5File(synthetic["blow5"]))
    n_ev = [len(S.detect_events(raw, meta, False)) for _, meta, raw in reads]
    assert any(25 <= n - skip < 64 for n in n_ev)  # (about this test's own inputs)
    dtw = subprocess.run([BIN, "dtw", "--kmer-model", synthetic["model"], "--verbose", "0", "-p", str(skip), "-q", str(query), synthetic["fasta"], synthetic["blow5"]],
                         capture_output=True, timeout=300)
    assert dtw.returncode == 0, dtw.stderr.decode()
    want = sorted(dtw.stdout.decode().splitlines(keepends=True), key=lambda ln: ln.split("\t")[0])
    out = run_realtime(synthetic["model"], synthetic["fasta"], synthetic["blow5"], "--channels", "7", "--chunk-samples", "800", "-p", str(skip), "-q", str(query),
                       "--norm-events", "64", "--min-mapq", "61", "--recalibrate-at-end")
    got = strip_tags(out)
    short = {rid for (rid, _, _), n in zip(reads, n_ev) if n - skip < query}
    assert any(ln.split("\t")[0] in short for ln in want)  # (about this test's own inputs: dtw prints lines of reads that end short)
    assert got == want
    assert {tags(ln)[2] for ln in out.splitlines()} == {"F", "R"}


def test_early_decisions_cli_equals_python_replay(synthetic):  # noqa: F811
    skip, norm, query, min_events, min_mapq, channels, chunk, at = 3, 25, 70, 30, 5, 7, 800, (35, 50, 70)
    out = run_realtime(synthetic["model"], synthetic["fasta"], synthetic["blow5"], "--channels", str(channels), "--chunk-samples", str(chunk), "-p", str(skip), "-q", str(query),
                       "--norm-events", str(norm), "--min-events", str(min_events), "--min-mapq", str(min_mapq), "--recalibrate", ",".join(map(str, at)), "--recalibrate-at-end")
    reads = list(S.Blow5File(synthetic["blow5"]))
    ref = synthetic["ref"]
    lines, reasons, checks = [], set(), []
    with S.Aligner(ref, 0) as al:
        for tick, ch, index, row, info, span, why in realtime.replay(al, reads, channels, chunk, skip, norm, query, min_events, min_mapq, recalibrate=at, at_end=True):
            rid, _, raw = reads[index]
            line = realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why)
            lines.append(line)
            if line:
                reasons.add(why)
            if line and why in "EF":  # the host twin of the slot, fed the same chunks
                tw = RecalTwin(False, (skip, norm, query), at, True)
                for a in range(0, int(info["n_samples"]), chunk):  # (no read's length is a multiple of the chunk)
                    tw.feed(raw[a:a + chunk], a + chunk > len(raw))
                q = tw.query_so_far()
                assert q is not None and len(q) == int(info["q_events"]) and tw.window == int(info["norm_window"]), (rid, why)
                checks.append((q, row))
        assert out == "".join(lines)
        assert reasons == {"E", "F", "R"}, reasons  # (about this test's own inputs)
        qs = [q for q, _ in checks]
        want = al.align_db(np.concatenate(qs), np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.int64))
        assert_rows(np.array([row for _, row in checks], S.RESULT_DTYPE), want, True, "early and full rows against align_db")
