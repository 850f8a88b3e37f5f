"""`sigfish-amd realtime --group-cap` and replay(group_cap=) on a handful of synthetic reads drawn from one short contig that is
tiled by named groups of ten coordinates: the two print the same stdout bytes, the same trace (`cover` and `full` lines
included) and the same summary, with and without --quota.  At a cap nobody reaches every line is the --by-name line plus og.  The
rule is restated per read from the printed lines alone, with the numpy model of tests/group_cover_model.py: the accepted reads of a
tick add the interval of their line, the live labels that follow hold from the next tick on, so no read is accepted for a column
that was capped at the start of its tick; and a `full` line appears for every group the input fills, at the tick that filled it."""
import os
import subprocess

import pytest

import sigfish_amd as S
from sigfish_amd import realtime, synth
from tests import group_cover_model as M
from tests.realtime_util import BIN, write_model
from tests.test_session_raw_gpu import META

pytestmark = pytest.mark.gpu

SKIP, NORM, QUERY, MIN_EVENTS, CHANNELS, CHUNK, MARGIN, N_READS, K, CAP, TILE = 3, 25, 70, 30, 4, 800, 0.05, 16, 6, 1, 10


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("realtime_group_cap")
    model = write_model(tmp / "syn.model", K, synth.kmer_levels(K, 21))
    levels, _ = S.read_kmer_model(model)
    recs = [("c0", synth.random_sequence(405, 1)), ("c1", synth.random_sequence(905, 2))]
    fasta, blow5, bed = (str(tmp / n) for n in ("ref.fa", "reads.blow5", "t.bed"))
    with open(fasta, "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in recs))
    # every read comes from c0, which the groups tile: the reads of the later ticks find parts of it covered
    reads = synth.make_dna_raw_reads(recs[:1], levels, K, N_READS, seed=9, samples=(2500, 6000), kinds=("mapped",), meta={**META, "sampling_rate": 4000.0})
    synth.write_blow5(blow5, reads)
    with open(bed, "w") as f:
        f.write("".join(f"c0\t{a}\t{min(a + TILE, 401)}\tamp{a // TILE:02d}\n" for a in range(0, 401, TILE)))
    return dict(tmp=tmp, model=model, levels=levels, fasta=fasta, blow5=blow5, bed=bed)


def python_run(al, ref, reads, groups, group_cap, quota=None):
    """-> ([(tick, channel, line, cls, action, reason, on_group or None)], trace, summary)"""
    gt, names = groups
    trace, summary, out = [], {}, []
    kw = {}
    if group_cap is not None:
        kw["group_cap"] = group_cap
    if quota is not None:
        kw["quota"] = quota
    for item in realtime.replay(al, reads, CHANNELS, CHUNK, SKIP, NORM, QUERY, MIN_EVENTS, 61, trace=trace, targets=(gt, names), by_name=True, mode=S.ENRICH, margin=MARGIN,
                                summary=summary, **kw):
        tick, ch, index, row, info, span, why, cls, action, head = item[:10]
        og = item[10] if kw else None
        rid, _, raw = reads[index]
        line = realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why, target=(cls, S.ENRICH, MIN_EVENTS, MARGIN),
                                    group=None if head is None else (head, names), quota=None if og is None else (og, names))
        out.append((tick, ch, line, cls.copy(), action, why, og))
    return out, trace, summary


def binary_run(files, more, tag):
    path = str(files["tmp"] / f"trace_{tag}.txt")
    cmd = [BIN, "realtime", "--kmer-model", files["model"], "--verbose", "0", "--channels", str(CHANNELS), "--chunk-samples", str(CHUNK), "-p", str(SKIP), "-q", str(QUERY),
           "--norm-events", str(NORM), "--min-events", str(MIN_EVENTS), "--targets", files["bed"], "--enrich", "--margin", str(MARGIN), "--by-name"]
    run = subprocess.run(cmd + more + ["--trace", path, files["fasta"], files["blow5"]], capture_output=True, timeout=300)
    assert run.returncode == 0, run.stderr.decode()
    return run.stdout.decode(), open(path).read(), run.stderr.decode()


def test_group_cap_in_replay_and_in_the_binary(files):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    ref = S.RefModel.from_fasta(files["fasta"], files["levels"], K, 0, QUERY)
    reads = list(S.Blow5File(files["blow5"]))
    groups = S.read_target_groups(files["bed"], ref.names)
    gt, names = groups
    n_groups = len(names)
    assert n_groups == 41
    with S.Aligner(ref, 0) as al:
        got, trace, summary = python_run(al, ref, reads, groups, CAP)
        both, both_trace, both_summary = python_run(al, ref, reads, groups, CAP, quota=2)
        far, far_trace, far_summary = python_run(al, ref, reads, groups, 1 << 30)
        base, base_trace, base_summary = python_run(al, ref, reads, groups, None)
    assert len(got) == len(far) == len(base) == N_READS and "group_cover" in summary and "group_cover" not in base_summary
    assert not any(" cover " in ln or " full " in ln for ln in base_trace)

    # ---- a cap nobody reaches: every line is the --by-name line plus og, the trace is the same but for the cover lines ----
    for f, b in zip(far, base):
        assert f[:2] == b[:2] and f[4:6] == b[4:6]
        if b[2]:
            assert f[2].startswith(b[2][:-1] + "\tog:Z:") and f[2].count("\t") == b[2].count("\t") + 1, (f[2], b[2])
        else:
            assert f[2] == ""
    assert [ln for ln in far_trace if " cover " not in ln] == base_trace and not any(" full " in ln for ln in far_trace)

    # ---- the rule, read by read, from the printed lines ----
    targets = [tuple(int(x[f]) for f in ("contig", "begin", "end", "group")) for x in gt]
    model = M.GroupCover([int(x) for x in ref.ref_lengths], [int(x) for x in ref.st_offset], 2, n_groups, targets, CAP)
    marks = {}
    for ln in trace:
        if " cover " in ln or " full " in ln:
            marks.setdefault(int(ln.split()[1]), []).append(ln)
    full, n_iv, n_bases = set(), 0, 0
    for tick in sorted({g[0] for g in got}):
        added = []
        for _, ch, line, cls, action, why, og in (g for g in got if g[0] == tick):  # ascending channels
            assert action == (S.target_decide(cls, S.ENRICH, MIN_EVENTS, MARGIN) if why == "E" else "P")
            rid, x = int(cls["on_rid"]), int(cls["on_pos_end"])
            if rid >= 0:  # the best ON column is one the labels of this tick have live: the model BEFORE this tick's intervals
                e = x - model.off[rid]
                assert model.depth[rid][e] < CAP and og == int(model.by_coord[rid][e]) < n_groups, (tick, ch, cls, og)
            else:
                assert og == -1
            if action == "A" and line:  # no read is accepted for a column that was capped at the start of its tick
                assert rid >= 0 and f"\tog:Z:{names[og]}\n" in line and "\tac:A:A" in line
                f = line.split("\t")
                if int(f[7]) < int(f[8]):
                    added.append((ref.names.index(f[5]), int(f[7]), int(f[8])))
        model.add(added)  # ... which hold from the next tick on
        want = []
        if added:
            n_iv, n_bases = n_iv + len(added), n_bases + sum(e - b for _, b, e in added)
            want.append(f"tick {tick} cover n={len(added)} open={2 * int(ref.ref_lengths[0])}")  # (no mask cap: the mask's own columns, every column of c0)
            rec = model.records()
            for g in range(n_groups):
                if g not in full and rec[g]["columns"] > 0 and rec[g]["capped"] == rec[g]["columns"]:
                    full.add(g)
                    want.append(f"tick {tick} full group={names[g]}")
        assert marks.pop(tick, []) == want, tick
    assert not marks
    assert full, "the input fills no group: the test's reads do not reach what it is about"
    rec = model.records().astype(S.GROUP_COVER_DTYPE)
    assert summary["group_cover"]["records"].tobytes() == rec.tobytes() and summary["group_cover"]["intervals"] == n_iv and summary["group_cover"]["bases"] == n_bases
    assert summary["group_cover"]["full"] == full
    # (about this test's own inputs: the cap changes decisions)
    assert [g[4] for g in got] != [g[4] for g in base]

    # ---- the binary prints the same bytes, the same trace and the same summary; without --group-cap what it printed before ----
    tail = lambda s, n: realtime.format_summary(s) + realtime.format_group_summary(s, n)
    for more, want, want_trace, want_summary, tag in ((["--group-cap", str(CAP)], got, trace, tail(summary, names) + realtime.format_group_cover_summary(summary, names), "cap"),
                                                      (["--group-cap", str(CAP), "--quota", "2"], both, both_trace, tail(both_summary, names) + realtime.format_group_cover_summary(both_summary, names), "both"),
                                                      ([], base, base_trace, tail(base_summary, names), "base")):
        out, tr, err = binary_run(files, more, tag)
        assert out == "".join(g[2] for g in want), more
        assert tr == "".join(ln + "\n" for ln in want_trace), more
        assert err.endswith(want_summary) and ("group cap" in err) == bool(more), err
    assert any(" close group=" in ln for ln in both_trace) or both_summary.get("quota") == 2
