"""`sigfish-amd realtime --truth` and replay(truth=) on a small synthetic file whose reads know where they came from
(synth.make_dna_raw_reads_truth): the two print the same stdout, trace and `truth:` summary; without the four truth tags the lines
are those of the run without truth, and without its `verdict` lines the trace is that run's; every tt / tn is the class / group this
file computes in numpy from the truth file and the BED file, every tv / gv follows from the line's own tc / tg; the summary is a
recount from the printed lines and the trace.  With --targets alone, with --by-name --quota 2 and with --candidates 2.  Nothing is
asserted about how many decisions are correct."""
import os
import re
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime, synth
from tests.realtime_util import BIN, write_model
from tests.test_session_raw_gpu import META

pytestmark = pytest.mark.gpu

SKIP, NORM, QUERY, MIN_EVENTS, CHANNELS, CHUNK, MARGIN, N_READS, K = 3, 25, 70, 30, 8, 800, 0.05, 48, 6
KINDS = ("mapped", "mapped", "mapped", "random", "mapped", "mapped", "stalled", "mapped")
BED = "c0\t400\t1100\tleft\nc0\t900\t1500\tmid\nc1\t0\t700\tright\nc1\t2300\t3100\tlast\nc0\t2500\t2600\tleft\n"
ABSENT = (5, 17)  # reads left out of the truth file: they have no truth
TRUTH_TAGS = re.compile(r"\ttt:A:.\ttv:A:.(\ttn:Z:[^\t\n]*\tgv:A:.)?")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("realtime_truth")
    model = write_model(tmp / "syn.model", K, synth.kmer_levels(K, 21))
    levels, _ = S.read_kmer_model(model)
    recs = [("c0", synth.random_sequence(3005, 1)), ("c1", synth.random_sequence(3105, 2))]
    fasta, blow5, bed, paf = (str(tmp / n) for n in ("ref.fa", "reads.blow5", "t.bed", "truth.paf"))
    with open(fasta, "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in recs))
    reads, where = synth.make_dna_raw_reads_truth(recs, levels, K, N_READS, seed=7, samples=(2000, 9000), kinds=KINDS, meta={**META, "sampling_rate": 4000.0})
    synth.write_blow5(blow5, reads)
    synth.write_truth_paf(paf, reads, where, [n for n, _ in recs], [len(s) for _, s in recs])
    lines = open(paf).read().splitlines(True)
    with open(paf, "w") as f:
        f.write("".join(ln for k, ln in enumerate(lines) if k not in ABSENT))
    with open(bed, "w") as f:
        f.write(BED)
    return dict(tmp=tmp, model=model, levels=levels, fasta=fasta, blow5=blow5, bed=bed, paf=paf)


def numpy_truth(files):
    """{read id: (class, edge, group name)} from the two files, nothing of the package: shared bases counted one by one"""
    targets, names = [], []
    for ln in BED.splitlines():
        c, b, e, name = ln.split("\t")
        if name not in names:
            names.append(name)
        targets.append((c, int(b), int(e), names.index(name)))
    out = {}
    for ln in open(files["paf"]).read().splitlines():
        f = ln.split("\t")
        if f[5] == "*":
            out[f[0]] = ("O", False, "*")
            continue
        bases = np.arange(int(f[7]), int(f[8]))
        shared = [int(((bases >= b) & (bases < e)).sum()) if c == f[5] else 0 for c, b, e, _ in targets]
        groups = [g for (_, _, _, g), s in zip(targets, shared) if s]
        out[f[0]] = ("T" if groups else "O", bool(groups) and not any(s == len(bases) for s in shared), names[min(groups)] if groups else "*")
    return out, names


CASES = {"targets": (dict(), []), "by_name_quota": (dict(by_name=True, quota=2), ["--by-name", "--quota", "2"]), "candidates": (dict(candidates=2), ["--candidates", "2"])}


def python_run(al, ref, reads, files, kw, truth):
    """-> (lines: one string per decided read, primary and candidate lines together; trace; summary; actions by read index)"""
    by_name, quota, candidates = kw.get("by_name", False), kw.get("quota"), kw.get("candidates", 0)
    gt, names = S.read_target_groups(files["bed"], ref.names)
    targets = (gt, names) if by_name else S.read_targets(files["bed"], ref.names)
    trace, summary, lines, actions = [], {}, [], {}
    more = dict(truth=truth) if truth is not None else {}
    for item in realtime.replay(al, reads, CHANNELS, CHUNK, SKIP, NORM, QUERY, MIN_EVENTS, 61, targets=targets, mode=S.ENRICH, margin=MARGIN, summary=summary, trace=trace, **kw, **more):
        tick, ch, index, row, info, span, why = item[:7]
        at = 7
        cand = None
        if candidates:
            cand, at = item[at], at + 1
        cls, action, at = item[at], item[at + 1], at + 2
        head = on_group = marks = None
        if by_name:
            head, at = item[at], at + 1
        if quota is not None:
            on_group, at = item[at], at + 1
        if truth is not None:
            marks = item[at]
        rid, _, raw = reads[index]
        tags = dict(target=(cls, S.ENRICH, MIN_EVENTS, MARGIN), group=None if head is None else (head, names), quota=None if quota is None else (on_group, names),
                    truth=None if marks is None else (marks, names if by_name else None))
        text = realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why, **tags)
        if candidates:
            text += realtime.format_candidates(rid, len(raw), ref.names, ref.seq_lengths, row, cand, info, span, why, **tags)
        lines.append(text)
        actions[index] = action
    return lines, trace, summary, actions


def tag(line, name):
    m = re.search(r"\t" + name + r":[AZif]:([^\t\n]*)", line)
    return m.group(1) if m else None


@pytest.mark.parametrize("case", list(CASES))
def test_truth_in_the_binary_and_in_replay(files, case):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    kw, extra = CASES[case]
    by_name = kw.get("by_name", False)
    ref = S.RefModel.from_fasta(files["fasta"], files["levels"], K, 0, QUERY)
    reads = list(S.Blow5File(files["blow5"]))
    truth = S.read_truth(files["paf"], ref.names)
    want_of, names = numpy_truth(files)
    assert len(truth) == N_READS - len(ABSENT)
    kinds = [v[0] for v in want_of.values()]
    assert kinds.count("T") >= 8 and kinds.count("O") >= 12 and sum(v[1] for v in want_of.values()) >= 3 and sum(f"_{k}" in r for r in want_of for k in ("random", "stalled")) >= 6

    with S.Aligner(ref, 0) as al:
        lines, trace, summary, actions = python_run(al, ref, reads, files, kw, truth)
        base_lines, base_trace, base_summary, base_actions = python_run(al, ref, reads, files, kw, None)

    # ---- truth changes no decision: the lines without the four tags, the trace without its verdict lines ----
    assert len(lines) == len(base_lines) == N_READS and sum(bool(ln) for ln in lines) >= N_READS // 2
    assert [TRUTH_TAGS.sub("", ln) for ln in lines] == base_lines and "".join(lines) != "".join(base_lines)
    assert [ln for ln in trace if " verdict " not in ln] == base_trace and actions == base_actions
    assert "truth" in summary and "truth" not in base_summary and {k: v for k, v in summary.items() if k != "truth"} == base_summary
    every = [ln for text in lines for ln in text.splitlines()]
    assert all(ln.count("\ttt:A:") == 1 and ln.count("\ttv:A:") == 1 and ln.count("\ttn:Z:") == ln.count("\tgv:A:") == int(by_name) for ln in every)
    assert all(re.search(r"\ttt:A:.\ttv:A:." + (r"\ttn:Z:[^\t]*\tgv:A:.$" if by_name else "$"), ln) for ln in every)  # behind all other tags
    if kw.get("candidates"):
        assert any("\ttp:A:S\t" in ln for ln in every)
        for text in lines:  # candidate lines repeat their primary's truth tags
            per = text.splitlines()
            assert all(TRUTH_TAGS.search(ln).group(0) == TRUTH_TAGS.search(per[0]).group(0) for ln in per[1:])

    # ---- every tt / tn is this file's class / group; every tv / gv follows from the line's own tc / tg ----
    for ln in every:
        rid = ln.split("\t")[0]
        cls, _, group = want_of.get(rid, ("N", False, None))
        tc, tt, tv = tag(ln, "tc"), tag(ln, "tt"), tag(ln, "tv")
        assert tt == cls, (ln, want_of.get(rid))
        assert tv == ("N" if "N" in (tc, tt) else "C" if tc == tt else "W"), ln
        if by_name:
            tg, tn, gv = tag(ln, "tg"), tag(ln, "tn"), tag(ln, "gv")
            assert tn == ("." if group is None else group), (ln, want_of.get(rid))
            assert gv == ("N" if tn == "." else "C" if tg == tn else "W"), ln
    seen = {tag(ln, "tt") for ln in every}
    assert {"T", "O"} <= seen  # (N too where an absent read prints a line)

    # ---- the summary is a recount from the printed lines and the trace ----
    length, recount = {}, realtime.new_truth_account(by_name)
    primary = {ln.split("\t")[0]: ln for ln in every if "\ttp:A:S\t" not in ln}
    index_of = {rid: k for k, (rid, _, _) in enumerate(reads)}
    verdicts = 0
    for k, ln in enumerate(trace):
        f = ln.split()
        if f[2] == "take":
            length[int(f[4].split("=")[1])] = int(f[5].split("=")[1])
        if f[2] != "verdict":
            continue
        verdicts += 1
        assert " decide " in trace[k - 1] and trace[k - 1].split()[3:5] == f[3:5] and trace[k - 1].split()[-1] == f[-1], (trace[k - 1], ln)
        read, tt, tv, sent = int(f[4].split("=")[1]), f[5][3:], f[6][3:], int(f[7].split("=")[1])
        rid = reads[read][0]
        assert tt == want_of.get(rid, ("N",))[0]
        line = primary.get(rid)
        action = tag(line, "ac") if line else actions[read]
        assert action == actions[read] and (line is None or tv == tag(line, "tv"))
        realtime.note_truth(recount, tt, want_of.get(rid, ("N", False))[1], action, tv, sent, 0 if action == "U" else length[read] - sent, length[read])
        if by_name and line:
            recount["groups"][tag(line, "gv")] += 1
    assert verdicts == N_READS == sum(" decide " in ln for ln in trace) and sorted(index_of[r] for r in primary) == sorted(i for i, ln in enumerate(lines) if ln)
    assert summary["truth"] == recount, (summary["truth"], recount)
    assert recount["N"]["reads"] == len(ABSENT) and recount["T"]["reads"] + recount["O"]["reads"] == N_READS - len(ABSENT)
    want_summary = realtime.format_truth_summary(recount)

    # ---- the binary prints what replay() prints: stdout, trace, summary; and without --truth what it printed before ----
    common = [BIN, "realtime", "--kmer-model", files["model"], "--verbose", "0", "--channels", str(CHANNELS), "--chunk-samples", str(CHUNK), "-p", str(SKIP), "-q", str(QUERY),
              "--norm-events", str(NORM), "--min-events", str(MIN_EVENTS), "--targets", files["bed"], "--enrich", "--margin", str(MARGIN)] + extra
    for more, want_lines, want_trace in ((["--truth", files["paf"]], lines, trace), ([], base_lines, base_trace)):
        path = str(files["tmp"] / f"trace_{case}_{len(more)}.txt")
        run = subprocess.run(common + more + ["--trace", path, files["fasta"], files["blow5"]], capture_output=True, timeout=300)
        assert run.returncode == 0, run.stderr.decode()
        err = run.stderr.decode()
        assert run.stdout.decode() == "".join(want_lines) and open(path).read() == "".join(ln + "\n" for ln in want_trace), (case, more)
        head = realtime.format_summary(base_summary) + (realtime.format_group_summary(base_summary, names) if by_name else "")
        assert err.endswith(head + (want_summary if more else "")) and ("truth:" in err) == bool(more), (err, head, want_summary)
