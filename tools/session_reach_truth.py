#!/usr/bin/env python3
"""Reach targets against truth, measured: what a lead buys and costs under --enrich, on the synthetic reads and the truth of
tools/session_truth_bench.py (same reference, targets, read kinds and observation: every read is fed to its end, one
Session.classes call per tick, decisions simulated offline with that tool's numpy statement of target_decide).

Per setting -- a lead of 0, of about half and of about one synthetic read length, on targets for both strands (the lead lies in
front of the target in each strand's own direction), and the margins below at --min-events 50 -- the table gives, for --enrich:
  accepted       reads decided on target (they are sequenced to their end)
  wrong unblocks reads decided off target whose whole true span shares a base with a target (truth_class 'T')
  wrong accepts  reads decided on target whose truth is 'O' (mapped elsewhere, or belonging nowhere)
  samples/read   samples sent up to the decision, mean over the decided reads
Lead 0 is Session.set_reach_targets with lead 0, which is the plain mask.  No threshold follows from this table.

    python tools/session_reach_truth.py [--reads 4000] [--channels 512] [--chunk 1600] [--query 250] [--out DIR]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import session_truth_bench as TB  # noqa: E402
import sigfish_amd as S  # noqa: E402
from sigfish_amd import synth  # noqa: E402

MARGINS = (0.02, 0.05, 0.1)
MIN_EVENTS = 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4000)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=1600)
    ap.add_argument("--query", type=int, default=250)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out_dir = a.out or os.path.join(ROOT, "profiles", f"session_reach_{S.build_id()}")
    os.makedirs(out_dir, exist_ok=True)
    log = open(os.path.join(out_dir, "session_reach_truth.log"), "w")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    levels = synth.kmer_levels(TB.K, 1)
    fasta = os.path.join(ROOT, "tests", "golden", "data", "nCoV-2019.reference.fasta")
    recs = [(n, s) for n, s in S.read_fasta(fasta)]
    ref = S.RefModel.from_fasta(fasta, levels, TB.K, 0, a.query)
    targets = [(0, 2000, 3000), (0, 14000, 15200), (0, 25500, 26300)]
    reads, where = synth.make_dna_raw_reads_truth(recs, levels, TB.K, a.reads, seed=a.seed, kinds=TB.KINDS)
    spans = [w[2] - w[1] for w in where if w is not None]
    read_len = int(np.median(spans))
    leads = (0, read_len // 2, read_len)
    true_t = np.array([w is not None and S.truth_class(targets, *w[:3]) == "T" for w in where])
    say(f"build {S.build_id()}  targets {targets}  reads {a.reads} kinds {TB.KINDS}  channels {a.channels} chunk {a.chunk} query {a.query} seed {a.seed}")
    say(f"median true span of a mapped read {read_len} bases: leads {leads}; {int(true_t.sum())} reads truly on target, {int((~true_t).sum())} off")
    say("")
    say("| lead | margin | decided | accepted reads | wrong unblocks | wrong accepts | samples sent per decided read |")
    say("|---|---|---|---|---|---|---|")
    table = []
    with S.Aligner(ref, 0) as al:
        for lead in leads:
            t0 = time.time()
            rt = [(c, b, e, lead, None) for c, b, e in targets]
            records, ticks = TB.observe(al, reads, a.channels, a.chunk, a.query, targets, lambda text: None, apply=lambda se: se.set_reach_targets(rt))
            width = max(len(r) for r in records)
            n = np.zeros((len(records), width), np.int64)
            on = np.full((len(records), width), np.inf, np.float32)
            off = np.full((len(records), width), np.inf, np.float32)
            ok = np.zeros((len(records), width), bool)
            sent = np.zeros((len(records), width), np.int64)
            for i, r in enumerate(records):
                for k, (ne, a_on, a_off, cal, s) in enumerate(r):
                    n[i, k], on[i, k], off[i, k], ok[i, k], sent[i, k] = ne, a_on, a_off, cal, s
            rows = np.arange(len(records))
            for mg in MARGINS:
                d = TB.decide(n, on, off, ok, MIN_EVENTS, mg)
                has = (d != 0).any(axis=1)
                first = np.where(has, (d != 0).argmax(axis=1), 0)
                cls = np.where(has, d[rows, first], 0)
                table.append(f"| {lead} | {mg} | {int(has.sum())} | {int((cls == 1).sum())} | {int(((cls == -1) & true_t).sum())} | {int(((cls == 1) & ~true_t).sum())} | "
                             f"{sent[rows, first][has].mean() if has.any() else float('nan'):.0f} |")
                say(table[-1])
            print(f"  (lead {lead}: {ticks} ticks, {time.time() - t0:.1f} s)", flush=True)
    log.close()


if __name__ == "__main__":
    main()
