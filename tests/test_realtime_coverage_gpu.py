"""`sigfish-amd realtime --depth-cap` and replay(depth_cap=) on a handful of synthetic reads drawn from one short contig that is
one target: the two print the same stdout bytes and the same trace, `cover` lines included.  The rule is restated per read from
the printed lines alone, with the numpy model of tests/coverage_model.py: the accepted reads of a tick add the target interval of
their line, the mask that follows holds from the next tick on, so the best on-target column a later read reports must be a
coordinate the model still has open, a read decided when the model has no open column is unblocked with an empty on-target class,
and every `cover` line carries the model's count.  Without depth_cap the output is what it was."""
import os
import subprocess

import pytest

import sigfish_amd as S
from sigfish_amd import realtime, synth
from tests import coverage_model as M
from tests.realtime_util import BIN, write_model
from tests.test_session_raw_gpu import META

pytestmark = pytest.mark.gpu

SKIP, NORM, QUERY, MIN_EVENTS, CHANNELS, CHUNK, MARGIN, N_READS, K, CAP = 3, 25, 70, 30, 4, 800, 0.05, 16, 6, 1


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("realtime_coverage")
    model = write_model(tmp / "syn.model", K, synth.kmer_levels(K, 21))
    levels, _ = S.read_kmer_model(model)
    recs = [("c0", synth.random_sequence(405, 1)), ("c1", synth.random_sequence(905, 2))]
    fasta, blow5, bed = (str(tmp / n) for n in ("ref.fa", "reads.blow5", "t.bed"))
    with open(fasta, "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in recs))
    # every read comes from c0, the target: the reads of the later ticks find it covered
    reads = synth.make_dna_raw_reads(recs[:1], levels, K, N_READS, seed=9, samples=(2500, 6000), kinds=("mapped",), meta={**META, "sampling_rate": 4000.0})
    synth.write_blow5(blow5, reads)
    with open(bed, "w") as f:
        f.write("c0\t0\t401\n")
    return dict(tmp=tmp, model=model, levels=levels, fasta=fasta, blow5=blow5, bed=bed)


def python_run(al, ref, reads, targets, depth_cap):
    trace, summary, out = [], {}, []
    kw = {} if depth_cap is None else dict(depth_cap=depth_cap)
    for tick, ch, index, row, info, span, why, cls, action in realtime.replay(al, reads, CHANNELS, CHUNK, SKIP, NORM, QUERY, MIN_EVENTS, 61, trace=trace, targets=targets,
                                                                              mode=S.ENRICH, margin=MARGIN, summary=summary, **kw):
        rid, _, raw = reads[index]
        out.append((tick, ch, realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why, target=(cls, S.ENRICH, MIN_EVENTS, MARGIN)), cls.copy(), action, why))
    return out, trace, summary


def test_depth_cap_in_replay_and_in_the_binary(files):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    ref = S.RefModel.from_fasta(files["fasta"], files["levels"], K, 0, QUERY)
    reads = list(S.Blow5File(files["blow5"]))
    targets = S.read_targets(files["bed"], ref.names)
    t = [tuple(int(v) for v in x) for x in targets]
    with S.Aligner(ref, 0) as al:
        got, trace, summary = python_run(al, ref, reads, targets, CAP)
        base, base_trace, base_summary = python_run(al, ref, reads, targets, None)
    assert len(got) == len(base) == N_READS and "cover" in summary and "cover" not in base_summary and not any(" cover " in ln for ln in base_trace)

    # ---- the rule, read by read, from the printed lines ----
    model = M.Coverage([int(x) for x in ref.ref_lengths], [int(x) for x in ref.st_offset], 2, CAP)
    covers = {int(ln.split()[1]): ln for ln in trace if " cover " in ln}
    ticks = sorted({g[0] for g in got})
    n_iv = n_bases = 0
    for tick in ticks:
        added = []
        for _, ch, line, cls, action, why in (g for g in got if g[0] == tick):  # ascending channels
            assert action == (S.target_decide(cls, S.ENRICH, MIN_EVENTS, MARGIN) if why == "E" else "P")
            rid, x = int(cls["on_rid"]), int(cls["on_pos_end"])
            if model.open_columns(t) == 0:  # nothing is wanted any more: the class is empty, an early decision unblocks
                assert rid == -1 and x == -1 and (why != "E" or action == "U"), (tick, ch, cls)
            elif rid >= 0:  # the best on-target column is one the mask of this tick has open: the model BEFORE this tick's intervals
                assert model.depth[rid][x - model.off[rid]] < CAP, (tick, ch, cls)
            if action == "A" and line:
                f = line.split("\t")
                assert f[5] == ref.names[0] and "\tac:A:A" in line
                if int(f[7]) < int(f[8]):
                    added.append((ref.names.index(f[5]), int(f[7]), int(f[8])))
        model.add(added)  # ... which hold from the next tick on
        if added:
            n_iv, n_bases = n_iv + len(added), n_bases + sum(e - b for _, b, e in added)
            assert covers.pop(tick) == f"tick {tick} cover n={len(added)} open={model.open_columns(t)}", tick
    assert not covers  # no `cover` line without an accepted read
    assert summary["cover"] == dict(cap=CAP, intervals=n_iv, bases=n_bases, base=2 * int(ref.ref_lengths[0]), open=model.open_columns(t))
    # up to and including the tick of the first `cover` line the run is the run without a cap
    first = min(int(ln.split()[1]) for ln in trace if " cover " in ln)
    assert [g[2] for g in got if g[0] <= first] == [g[2] for g in base if g[0] <= first]
    assert [ln for ln in trace if int(ln.split()[1]) <= first and " cover " not in ln] == [ln for ln in base_trace if int(ln.split()[1]) <= first]
    # (about this test's own inputs: the cap changes decisions -- reads the plain run accepts are unblocked here)
    acts, base_acts = [g[4] for g in got], [g[4] for g in base]
    assert n_iv >= 2 and acts.count("A") < base_acts.count("A") and acts.count("U") > base_acts.count("U"), (acts, base_acts)

    # ---- the binary prints the same bytes and the same trace; without --depth-cap what it printed before ----
    common = [BIN, "realtime", "--kmer-model", files["model"], "--verbose", "0", "--channels", str(CHANNELS), "--chunk-samples", str(CHUNK), "-p", str(SKIP), "-q", str(QUERY),
              "--norm-events", str(NORM), "--min-events", str(MIN_EVENTS), "--targets", files["bed"], "--enrich", "--margin", str(MARGIN)]
    for more, want, want_trace, want_summary in ((["--depth-cap", str(CAP)], got, trace, realtime.format_summary(summary) + realtime.format_cover_summary(summary)),
                                                 ([], base, base_trace, realtime.format_summary(base_summary))):
        path = str(files["tmp"] / f"trace_{len(more)}.txt")
        run = subprocess.run(common + more + ["--trace", path, files["fasta"], files["blow5"]], capture_output=True, timeout=300)
        assert run.returncode == 0, run.stderr.decode()
        assert run.stdout.decode() == "".join(g[2] for g in want), more
        assert open(path).read() == "".join(ln + "\n" for ln in want_trace), more
        assert run.stderr.decode().endswith(want_summary) and ("coverage:" in run.stderr.decode()) == bool(more), run.stderr.decode()
