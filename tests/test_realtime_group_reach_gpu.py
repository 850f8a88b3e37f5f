"""`sigfish-amd realtime --by-name --group-lead N [--group-stranded]` and replay(by_name=True, group_lead=, group_stranded=) on a small
synthetic file whose reads know where they came from: the two print the same stdout bytes, the same trace and the same summary --
alone, stranded, with --quota, with --group-cap 1 and with --truth.  Per read the labels are restated with the numpy model of
tests/reach_group_model.py: the best ON column of a decided read carries a group's label under the model, the line's og names it,
and tg names it when that column beats the best OFF column.  The summary gains one line with the labelled columns, the model's
count.  --group-lead 0 without --group-stranded prints --by-name's bytes."""
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime, synth
from tests import reach_group_model as M
from tests.realtime_util import BIN, write_model
from tests.test_session_raw_gpu import META

pytestmark = pytest.mark.gpu

SKIP, NORM, QUERY, MIN_EVENTS, CHANNELS, CHUNK, MARGIN, N_READS, K, LEAD = 3, 25, 70, 30, 8, 800, 0.05, 32, 6, 400
BED = "c0\t400\t1100\tleft\t0\t+\nc0\t900\t1500\tmid\t0\t-\nc1\t0\t700\tright\t0\t.\nc1\t2300\t3100\tlast\t0\t+\nc0\t2500\t2600\tleft\t0\t-\n"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("realtime_group_reach")
    model = write_model(tmp / "syn.model", K, synth.kmer_levels(K, 21))
    levels, _ = S.read_kmer_model(model)
    recs = [("c0", synth.random_sequence(3005, 1)), ("c1", synth.random_sequence(3105, 2))]
    fasta, blow5, bed, paf = (str(tmp / n) for n in ("ref.fa", "reads.blow5", "t.bed", "truth.paf"))
    with open(fasta, "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in recs))
    reads, where = synth.make_dna_raw_reads_truth(recs, levels, K, N_READS, seed=7, samples=(2000, 9000), kinds=("mapped",), meta={**META, "sampling_rate": 4000.0})
    synth.write_blow5(blow5, reads)
    synth.write_truth_paf(paf, reads, where, [n for n, _ in recs], [len(s) for _, s in recs])
    with open(bed, "w") as f:
        f.write(BED)
    return dict(tmp=tmp, model=model, levels=levels, fasta=fasta, blow5=blow5, bed=bed, paf=paf)


def python_run(al, ref, reads, files, group_lead=None, group_stranded=False, quota=None, group_cap=None, truth=None):
    """-> ([(line, cls, action, head, on_group or None)] per decided read, trace, summary, names)"""
    if group_stranded:
        targets = S.read_reach_target_groups(files["bed"], ref.names, group_lead, stranded=True)
    else:
        targets = S.read_target_groups(files["bed"], ref.names)
    names = targets[1]
    kw = {}
    if group_lead is not None:
        kw.update(group_lead=group_lead, group_stranded=group_stranded)
    if quota is not None:
        kw["quota"] = quota
    if group_cap is not None:
        kw["group_cap"] = group_cap
    if truth is not None:
        kw["truth"] = truth
    use_open = quota is not None or group_cap is not None
    trace, summary, out = [], {}, []
    for item in realtime.replay(al, reads, CHANNELS, CHUNK, SKIP, NORM, QUERY, MIN_EVENTS, 61, targets=targets, by_name=True, mode=S.ENRICH, margin=MARGIN, summary=summary, trace=trace,
                                **kw):
        tick, ch, index, row, info, span, why, cls, action, head = item[:10]
        og = item[10] if use_open else None
        marks = item[10 + use_open] if truth is not None else None
        rid, _, raw = reads[index]
        line = realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why, target=(cls, S.ENRICH, MIN_EVENTS, MARGIN),
                                    group=None if head is None else (head, names), quota=None if og is None else (og, names), truth=None if marks is None else (marks, names))
        out.append((line, cls.copy(), action, None if head is None else head.copy(), og))
    return out, trace, summary, names


def want_summary(summary, names):
    text = realtime.format_summary(summary)
    if "reach_groups" in summary:
        text += realtime.format_reach_group_summary(summary)
    text += realtime.format_group_summary(summary, names)
    if "group_cover" in summary:
        text += realtime.format_group_cover_summary(summary, names)
    if "truth" in summary:
        text += realtime.format_truth_summary(summary["truth"])
    return text


CASES = {"group_lead": (dict(group_lead=LEAD), ["--group-lead", str(LEAD)]),
         "group_stranded": (dict(group_lead=LEAD, group_stranded=True), ["--group-lead", str(LEAD), "--group-stranded"]),
         "quota": (dict(group_lead=LEAD, group_stranded=True, quota=2), ["--group-lead", str(LEAD), "--group-stranded", "--quota", "2"]),
         "group_cap": (dict(group_lead=LEAD, group_cap=1), ["--group-lead", str(LEAD), "--group-cap", "1"]),
         "truth": (dict(group_lead=LEAD, group_stranded=True, truth=True), ["--group-lead", str(LEAD), "--group-stranded", "--truth", None]),
         "group_lead_0": (dict(group_lead=0), ["--group-lead", "0"])}


def binary_run(files, extra, tag):
    path = str(files["tmp"] / f"trace_{tag}.txt")
    cmd = [BIN, "realtime", "--kmer-model", files["model"], "--verbose", "0", "--channels", str(CHANNELS), "--chunk-samples", str(CHUNK), "-p", str(SKIP), "-q", str(QUERY),
           "--norm-events", str(NORM), "--min-events", str(MIN_EVENTS), "--targets", files["bed"], "--enrich", "--margin", str(MARGIN), "--by-name"]
    run = subprocess.run(cmd + extra + ["--trace", path, files["fasta"], files["blow5"]], capture_output=True, timeout=300)
    assert run.returncode == 0, run.stderr.decode()
    return run.stdout.decode(), open(path).read(), run.stderr.decode()


@pytest.mark.parametrize("case", list(CASES))
def test_the_binary_prints_what_replay_prints(files, case):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    kw, extra = CASES[case]
    kw = dict(kw)
    extra = [files["paf"] if x is None else x for x in extra]
    ref = S.RefModel.from_fasta(files["fasta"], files["levels"], K, 0, QUERY)
    reads = list(S.Blow5File(files["blow5"]))
    if kw.get("truth"):
        kw["truth"] = S.read_truth(files["paf"], ref.names)
    with S.Aligner(ref, 0) as al:
        got, trace, summary, names = python_run(al, ref, reads, files, **kw)
    assert len(got) == N_READS
    # ---- the labels, restated: the model's list from the BED file alone ----
    contigs, groups, tl = list(ref.names), [], []
    for ln in BED.splitlines():
        f = ln.split("\t")
        if f[3] not in groups:
            groups.append(f[3])
        tl.append((contigs.index(f[0]), int(f[1]), int(f[2]), kw["group_lead"], groups.index(f[3]), (None if f[5] == "." else f[5]) if kw.get("group_stranded") else None))
    assert groups == names
    ng = len(names)
    lens, offs = [int(x) for x in ref.ref_lengths], [int(x) for x in ref.st_offset]
    label, _ = M.tables(tl, ng, lens, offs, 2)
    assert summary["reach_groups"] == dict(lead=kw["group_lead"], stranded=bool(kw.get("group_stranded")), columns=int((label != ng).sum())) and summary["reach_groups"]["columns"] > 0
    named = 0
    for line, cls, action, head, og in got:
        if cls["valid"] != 1 or cls["on_rid"] < 0:
            continue
        want, _ = M.label_of(tl, ng, int(cls["on_rid"]), chr(int(cls["on_strand"])), int(cls["on_pos_end"]))
        assert want < ng, (cls, want)  # the best ON column is one the model labels
        if og is not None:
            assert og == want, (cls, og, want)
        if head is not None and cls["on_score"] < cls["off_score"]:  # the row's best column overall: the head's best entry is its label
            assert head["best"] == want and f"\ttg:Z:{names[want]}\t" in line, (line, want)
            named += 1
    assert named > 0, "no read's best column is labelled: the test's reads do not reach what it is about"
    # ---- the binary: the same bytes, the same trace, the same summary ----
    out, btrace, err = binary_run(files, extra, case)
    assert out == "".join(g[0] for g in got), case
    assert btrace == "".join(ln + "\n" for ln in trace), case
    assert err.endswith(want_summary(summary, names)) and "reach groups: lead" in err, (err, want_summary(summary, names))
    if case == "group_lead_0":  # lead 0, both strands: --by-name's bytes
        base_out, base_trace, base_err = binary_run(files, [], "by_name")
        assert out == base_out and btrace == base_trace and "reach groups" not in base_err
        assert base_err.endswith(want_summary(summary, names).replace(realtime.format_reach_group_summary(summary), ""))


def test_group_stranded_bed_errors(files, tmp_path):
    common = [BIN, "realtime", "--kmer-model", files["model"], "--targets", None, "--enrich", "--margin", "0.1", "--by-name", "--group-lead", "5", "--group-stranded", files["fasta"],
              files["blow5"]]
    for text, word in (("c0\t10\t20\tg\n", "--group-stranded needs a sixth column"), ("c0\t10\t20\tn\t0\tx\n", "none of")):
        bed = tmp_path / "bad.bed"
        bed.write_text(text)
        run = subprocess.run([str(bed) if x is None else x for x in common], capture_output=True, timeout=300)
        assert run.returncode > 0 and word in run.stderr.decode() and run.stdout == b"", run.stderr.decode()
