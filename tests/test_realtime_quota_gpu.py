"""`sigfish-amd realtime --quota` and replay(quota=) on a small synthetic file over a reference of a few named targets: the two print
the same stdout, trace and summary; with a quota nobody reaches every line minus its og tag is the --by-name line; after a group's
`close` line no later line carries ac:A:A with that group's og; and the input is no vacuous one -- the Python run alone shows a
closure and a read whose action differs from the run without a quota."""
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime, synth
from tests.realtime_util import BIN, write_model
from tests.test_session_raw_gpu import META

pytestmark = pytest.mark.gpu

SKIP, NORM, QUERY, MIN_EVENTS, CHANNELS, CHUNK, MARGIN, N_READS = 3, 25, 70, 30, 4, 800, 0.05, 28


def python_run(al, ref, reads, gt, names, quota):
    """replay(by_name=True, quota=) -> (lines, trace, summary, [(tick, name of on_group or None, action, line)])"""
    trace, summary, lines, seen = [], {}, [], []
    kw = dict(quota=quota) if quota is not None else {}
    for item in realtime.replay(al, reads, CHANNELS, CHUNK, SKIP, NORM, QUERY, MIN_EVENTS, 61, targets=(gt, names), by_name=True, mode=S.ENRICH, margin=MARGIN, summary=summary,
                                trace=trace, **kw):
        tick, ch, index, row, info, span, why, cls, action, head = item[:10]
        on_group = item[10] if quota is not None else None
        rid, _, raw = reads[index]
        line = realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why, target=(cls, S.ENRICH, MIN_EVENTS, MARGIN),
                                    group=None if head is None else (head, names), quota=None if quota is None else (on_group, names))
        lines.append(line)
        seen.append((tick, index, on_group, action, line))
    return lines, trace, summary, seen


def test_quota_in_the_binary_and_in_replay(tmp_path):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    k = 6
    model = write_model(tmp_path / "syn.model", k, synth.kmer_levels(k, 21))
    levels, _ = S.read_kmer_model(model)
    recs = [("c0", synth.random_sequence(905, 1)), ("c1", synth.random_sequence(405, 2)), ("c2", synth.random_sequence(62, 3))]
    fasta, blow5, bed = (str(tmp_path / n) for n in ("ref.fa", "reads.blow5", "t.bed"))
    with open(fasta, "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in recs))
    synth.write_blow5(blow5, synth.make_dna_raw_reads(recs, levels, k, N_READS, seed=7, samples=(2000, 9000), kinds=("mapped", "mapped", "mapped", "random", "mapped", "mapped", "stalled"),
                                                      meta={**META, "sampling_rate": 4000.0}))
    with open(bed, "w") as f:
        f.write("c0\t0\t450\tleft\nc1\t0\t400\tother\nc0\t450\t900\tright\n")
    ref = S.RefModel.from_fasta(fasta, levels, k, 0, QUERY)
    reads = list(S.Blow5File(blow5))
    gt, names = S.read_target_groups(bed, ref.names)
    assert names == ["left", "other", "right"]
    common = [BIN, "realtime", "--kmer-model", model, "--verbose", "0", "--channels", str(CHANNELS), "--chunk-samples", str(CHUNK), "-p", str(SKIP), "-q", str(QUERY),
              "--norm-events", str(NORM), "--min-events", str(MIN_EVENTS), "--targets", bed, "--enrich", "--margin", str(MARGIN), "--by-name"]

    def binary(extra, name):
        run = subprocess.run(common + extra + ["--trace", str(tmp_path / name), fasta, blow5], capture_output=True, timeout=300)
        assert run.returncode == 0, run.stderr.decode()
        return run.stdout.decode(), open(tmp_path / name).read(), run.stderr.decode().splitlines()

    with S.Aligner(ref, 0) as al:
        base_lines, base_trace, base_summary, base_seen = python_run(al, ref, reads, gt, names, None)
        lines, trace, summary, seen = python_run(al, ref, reads, gt, names, 2)
        far_lines, far_trace, far_summary, _ = python_run(al, ref, reads, gt, names, 1000)

    # ---- the restatement alone, first: this input closes a group and changes what happens to a read ----
    closes = [ln for ln in trace if " close " in ln]
    assert len(closes) >= 1, trace
    action_of_read = {index: action for _, index, _, action, _ in seen}
    base_action = {index: action for _, index, _, action, _ in base_seen}
    changed = [i for i in action_of_read if base_action.get(i) == "A" and action_of_read[i] == "U"]
    assert len(changed) >= 1, (action_of_read, base_action)
    assert not any(" close " in ln for ln in base_trace + far_trace)

    # ---- after a group's close line no later line carries ac:A:A with that group's og; within the closing tick it may ----
    closed_at = {ln.split("group=")[1].split()[0]: int(ln.split()[1]) for ln in closes}
    accepted = dict.fromkeys(names, 0)
    for tick, index, on_group, action, line in seen:
        if not line:
            continue
        og = line.rstrip("\n").split("\t")[-1]
        assert og == "og:Z:" + (names[on_group] if 0 <= on_group < len(names) else "*")
        if "\tac:A:A\t" in line:
            assert og != "og:Z:*" and (og[5:] not in closed_at or tick <= closed_at[og[5:]]), (tick, line, closed_at)
            accepted[og[5:]] += 1
    for name, tick in closed_at.items():
        assert accepted[name] >= 2 and f"tick {tick} close group={name} accepted=2" in closes  # closed by the read that filled the quota
        assert summary[("closed_at", names.index(name))] == tick
    assert all(accepted[n] < 2 for n in names if n not in closed_at)

    # ---- a quota nobody reaches: every line minus its og tag is the --by-name line, the trace is the same ----
    assert len(far_lines) == len(base_lines) == N_READS and far_trace == base_trace
    for far, base in zip(far_lines, base_lines):
        assert (far == "" and base == "") or (far.rsplit("\tog:Z:", 1)[0] + "\n" == base and far.count("\tog:Z:") == 1), (far, base)

    # ---- the binary prints what replay() prints: stdout, trace, summary ----
    for quota, want_lines, want_trace, want_summary in ((2, lines, trace, summary), (1000, far_lines, far_trace, far_summary)):
        out, tr, err = binary(["--quota", str(quota)], f"trace_{quota}.txt")
        assert out == "".join(want_lines) and tr == "".join(ln + "\n" for ln in want_trace), quota
        want = realtime.format_summary(want_summary) + realtime.format_group_summary(want_summary, names)
        assert "".join(ln + "\n" for ln in err[-len(names) - 2:]) == want, (err, want)
        assert f"quota={quota} closed_at=" in want
    # without --quota: stdout, trace and stderr are what --by-name printed (the lines of the Python run without a quota)
    out, tr, err = binary([], "trace_none.txt")
    assert out == "".join(base_lines) and tr == "".join(ln + "\n" for ln in base_trace) and "og:Z:" not in out
    assert "".join(ln + "\n" for ln in err[-len(names) - 2:]) == realtime.format_summary(base_summary) + realtime.format_group_summary(base_summary, names)
    assert "quota" not in "\n".join(err)
