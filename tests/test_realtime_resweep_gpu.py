"""`sigfish-amd realtime --rna --resweep` on the GPU: direct RNA in the reference's own orientation (the query is the events
reversed) replayed through a resweep session
  * with its defaults (normalisation over the whole query, never early) a read with at least p + q events prints the line
    `sigfish-amd dtw --rna` prints for it, i.e. the compiled reference's golden output (rna_default), once the three tags are
    removed, whatever the channels and the chunk size;
  * calibrated on 25 events, recalibrated on the doubling list and at the end of the read, every F and R line is dtw's;
  * the command line and the Python replay(resweep=True) print the same bytes.
No tolerance anywhere."""
import pytest

import sigfish_amd as S
from sigfish_amd import realtime
from tests.realtime_util import strip_tags, tags, write_model
from tests.test_realtime_gpu import run_realtime
from tests.util import load_case

pytestmark = pytest.mark.gpu

# reads of the fixture with fewer than p + q = 300 events (exempt from the comparison with dtw under the defaults: never
# calibrated here, a shortened window there).  The eight reads of sequin_rna.blow5 have 1117 .. 4233 events, so none is
EXEMPT = []


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    c = load_case("rna_default")
    assert c["flag"] == S.RNA and [str(a) for a in c["args"]] == ["--rna"]  # (the reference's own orientation: no --invert)
    c["model"] = write_model(tmp_path_factory.mktemp("rna") / "syn.model", c["k"])
    c["want"] = sorted((ln + "\n" for ln in c["out_text"].splitlines()), key=lambda ln: ln.split("\t")[0])
    assert len(c["want"]) == 8
    return c


def test_defaults_equal_dtw(case):
    assert len(EXEMPT) <= 1
    want = [ln for ln in case["want"] if ln.split("\t")[0] not in EXEMPT]
    for extra in (["--channels", "2", "--chunk-samples", "1600"], ["--channels", "8", "--chunk-samples", "1600"], ["--channels", "3", "--chunk-samples", "333"]):
        out = run_realtime(case["model"], case["fasta"], case["blow5"], "--rna", "--resweep", *extra)
        got = [ln for ln in strip_tags(out) if ln.split("\t")[0] not in EXEMPT]
        assert got == want, (extra, out)
        for ln in out.splitlines():
            ne, ns, why = tags(ln)
            assert ne == case["query_size"] and why == "F" and 0 < ns <= int(ln.split("\t")[1]), ln


def test_short_calibration_equals_dtw(case):
    """a window that starts at 25 events and doubles: 50, 100, 200, then q = 250; every line a read ends with is dtw's, no read
    exempt"""
    for channels, chunk in ((2, 1600), (8, 333)):
        out = run_realtime(case["model"], case["fasta"], case["blow5"], "--rna", "--resweep", "--channels", str(channels), "--chunk-samples", str(chunk),
                           "--norm-events", "25", "--recalibrate", "double", "--recalibrate-at-end")
        assert strip_tags(out) == case["want"], ((channels, chunk), out)
        for ln in out.splitlines():
            assert tags(ln)[2] in "FR", ln


def test_cli_equals_python_replay(case):
    """with early decisions: --min-events 50 --min-mapq 20 on a window that doubles from 25 events"""
    skip, norm, query, min_events, min_mapq, channels, chunk = case["prefix_size"], 25, case["query_size"], 50, 20, 3, 800
    out = run_realtime(case["model"], case["fasta"], case["blow5"], "--rna", "--resweep", "--channels", str(channels), "--chunk-samples", str(chunk),
                       "--norm-events", str(norm), "--min-events", str(min_events), "--min-mapq", str(min_mapq), "--recalibrate", "double", "--recalibrate-at-end")
    levels, k = S.read_kmer_model(case["model"])
    ref = S.RefModel.from_fasta(case["fasta"], levels, k, S.RNA, query)
    reads = list(S.Blow5File(case["blow5"]))
    lines = []
    with S.Aligner(ref, S.RNA) as al:
        for tick, ch, index, row, info, span, why in realtime.replay(al, reads, channels, chunk, skip, norm, query, min_events, min_mapq, recalibrate="double",
                                                                     at_end=True, resweep=True):
            rid, _, raw = reads[index]
            line = realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why)
            lines.append(line)
            if line:  # q_events is the window: a point of the list, or all the read had at its end
                assert tags(line) == (int(info["q_events"]), int(info["n_samples"]), why) and int(info["q_events"]) == int(info["norm_window"])
    assert out == "".join(lines) and len(out.splitlines()) >= 1
