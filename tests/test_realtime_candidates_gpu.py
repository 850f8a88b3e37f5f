"""`sigfish-amd realtime --candidates` on the GPU: with the defaults a read's lines without the three tags are the lines
`sigfish-amd dtw --secondary yes` prints -- the reference's primary line and, behind it, the candidates of tests/golden/secondary/
--, the Python replay prints the same bytes as the binary, and without the option no byte of the output moves."""
import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime
from tests.realtime_util import strip_tags, tags, write_model
from tests.test_cli_secondary_gpu import _expected
from tests.test_realtime_gpu import run_realtime, synthetic  # noqa: F401 (synthetic: the module's fixture of mixed decisions)
from tests.util import load_case

pytestmark = pytest.mark.gpu
EXTRA = (["--channels", "2", "--chunk-samples", "1600"], ["--channels", "8", "--chunk-samples", "333"])


def _by_read(lines):
    """lines grouped by read id, in the order they were printed (a read's primary first, its candidates best first)"""
    out = {}
    for ln in lines:
        out.setdefault(ln.split("\t")[0], []).append(ln)
    return out


def test_defaults_equal_dtw_secondary(tmp_path):
    c = load_case("dna_default")
    model = write_model(tmp_path / "syn.model", c["k"])
    want = _by_read(_expected(c).splitlines(keepends=True))  # what `dtw --secondary yes` prints (tests/test_cli_secondary_gpu.py)
    assert any(len(v) > 1 for v in want.values()) and all("tp:A:P" in v[0] and all("tp:A:S" in x for x in v[1:]) for v in want.values())
    plain = sorted(c["out_text"].splitlines(keepends=True), key=lambda ln: ln.split("\t")[0])
    for extra in EXTRA:
        args = [str(a) for a in c["args"]] + list(extra)
        out = run_realtime(model, c["fasta"], c["blow5"], *args, "--candidates", "4")
        got = _by_read(["\t".join(ln.split("\t")[:-3]) + "\n" for ln in out.splitlines()])
        assert got == want, (extra, out)  # every read of the fixture has p + q events: realtime prints them all
        for ln in out.splitlines():
            ne, ns, why = tags(ln)
            assert ne == c["query_size"] and why == "F", ln
        # without the option: the parent's output, the lines the existing golden test expects
        assert strip_tags(run_realtime(model, c["fasta"], c["blow5"], *args)) == plain, extra


def test_cli_equals_python_replay_with_candidates(synthetic):
    skip, norm, query, min_events, min_mapq, channels, chunk = 3, 25, 70, 30, 5, 7, 800
    common = ["--channels", str(channels), "--chunk-samples", str(chunk), "-p", str(skip), "-q", str(query), "--norm-events", str(norm), "--min-events", str(min_events),
              "--min-mapq", str(min_mapq)]
    out = run_realtime(synthetic["model"], synthetic["fasta"], synthetic["blow5"], *common, "--candidates", "4")
    reads = list(S.Blow5File(synthetic["blow5"]))
    ref = synthetic["ref"]
    text, prim_only, n_cand = [], [], 0
    with S.Aligner(ref, 0) as al:
        for tick, ch, index, row, info, span, why, cand in realtime.replay(al, reads, channels, chunk, skip, norm, query, min_events, min_mapq, candidates=4):
            rid, _, raw = reads[index]
            line = realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why)
            more = realtime.format_candidates(rid, len(raw), ref.names, ref.seq_lengths, row, cand, info, span, why)
            text += [line, more]
            prim_only.append(line)
            n_cand += more.count("\n")
            if line and cand["valid"][0]:
                assert row["score2"].tobytes() == cand["score"][0].tobytes()
    assert out == "".join(text)
    assert n_cand > 0 and out.count("tp:A:S") == n_cand  # (about this test's own inputs)
    # the schedule and the decisions do not change with the option: its output without the candidate lines is the output without it
    assert run_realtime(synthetic["model"], synthetic["fasta"], synthetic["blow5"], *common) == "".join(prim_only)
