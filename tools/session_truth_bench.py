#!/usr/bin/env python3
"""Target decisions against truth, measured: how early a class decision becomes possible, how often it is right, and what --enrich
buys in sequenced signal, over a grid of --margin and --min-events.

Observe, do not decide: a raw session is driven directly (not replay()); every read is fed tick by tick TO ITS END, whatever a
decision rule would have said, and after every tick ONE Session.classes call over the live slots records (n_events, on_score,
off_score) per read and tick.  Then target_decide is simulated offline over those records for every grid point: a read is decided at
its first tick whose record decides (the slot calibrated, n_events >= min_events, |off - on| >= margin * n_events); under --enrich a
read decided off target is unblocked there (what was sent so far is what the pore sequenced of it), every other read is sequenced to
its end.  The offline rule is a numpy statement of target_rules.hpp's; the tool checks it against the library's sfa_target_decide
on a sample of the records before it reports anything.

Workload: the nCoV reference (tests/golden/data), synthetic k-mer levels, targets covering about a tenth of it, reads from
synth.make_dna_raw_reads_truth -- half mapped, a quarter random, the rest stalled and flat --, 512 channels, 1600 samples per tick.
A read's truth is api.truth_class of its interval (an overlap rule); reads that straddle a target's edge are counted apart (edge).

    python tools/session_truth_bench.py [--reads 20000] [--channels 512] [--chunk 1600] [--query 250] [--out DIR]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sigfish_amd as S  # noqa: E402
from sigfish_amd import synth  # noqa: E402

K, SKIP, NORM = 6, 3, 25
KINDS = ("mapped", "random", "mapped", "stalled", "mapped", "random", "mapped", "flat")  # half mapped, a quarter random, the rest
MARGINS = (0.0, 0.01, 0.02, 0.05, 0.1, 0.2, 0.4)
MIN_EVENTS = (30, 50, 100, 200)


def observe(al, reads, channels, chunk, query, targets, say, apply=None):
    """-> per read a list of (n_events, on, off, calibrated, samples sent) per tick, to the read's end (or until its query is full).
    apply(session): sets the session's targets in place of Session.set_targets(targets) (tools/session_reach_truth.py)"""
    records = [[] for _ in reads]
    nxt, on, sent = 0, [-1] * channels, [0] * channels
    ticks = 0
    with al.session(channels) as se:
        se.configure_raw(SKIP, NORM, query)
        if apply is None:
            se.set_targets(targets)
        else:
            apply(se)
        while True:
            for c in range(channels):
                if on[c] < 0 and nxt < len(reads):
                    on[c], sent[c], nxt = nxt, 0, nxt + 1
            slots = [c for c in range(channels) if on[c] >= 0]
            if not slots:
                break
            chunks, ends = [], []
            for c in slots:
                raw = reads[on[c]][5]
                chunks.append(raw[sent[c]:sent[c] + chunk])
                sent[c] += len(chunks[-1])
                ends.append(len(chunks[-1]) < chunk)
            off = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
            scaling = [(reads[on[c]][1], reads[on[c]][2], reads[on[c]][3]) for c in slots]
            _, info = se.extend_raw(slots, np.concatenate(chunks) if off[-1] else np.zeros(0, np.int16), off, scaling, ends)
            cls = se.classes(slots)
            done = []
            for i, c in enumerate(slots):
                st = int(info[i]["status"])
                records[on[c]].append((int(cls[i]["n_events"]) if cls[i]["valid"] else 0, float(cls[i]["on_score"]), float(cls[i]["off_score"]), bool(st & S.RAW_CALIBRATED) and bool(cls[i]["valid"]),
                                       sent[c]))
                if ends[i] or st & (S.RAW_FULL | S.RAW_POISONED):
                    done.append(c)
            if done:
                se.reset(done)
                for c in done:
                    on[c] = -1
            ticks += 1
            if ticks % 50 == 0:
                say(f"  tick {ticks}: {nxt} of {len(reads)} reads taken")
    return records, ticks


def decide(n, on, off, ok, min_events, margin):
    """target_class_of over arrays: 1 on target, -1 off target, 0 undecided (float32 arithmetic, as target_rules.hpp)"""
    n32, m = n.astype(np.float32), np.float32(margin)
    with np.errstate(invalid="ignore"):
        need = m * n32
        both_inf = np.isinf(on) & np.isinf(off)
        t = (off - on >= need) & ~both_inf
        o = (on - off >= need) & ~both_inf & ~t
    live = ok & (n >= min_events)
    return np.where(live & t, 1, np.where(live & o, -1, 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=1600)
    ap.add_argument("--query", type=int, default=250, help="query events at which a read is full (-q)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None, help="directory for the log [profiles/session_truth_<build id> of the repository]")
    a = ap.parse_args()
    out_dir = a.out or os.path.join(ROOT, "profiles", f"session_truth_{S.build_id()}")
    os.makedirs(out_dir, exist_ok=True)
    log = open(os.path.join(out_dir, "session_truth_bench.log"), "w")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    levels = synth.kmer_levels(K, 1)
    fasta = os.path.join(ROOT, "tests", "golden", "data", "nCoV-2019.reference.fasta")
    recs = [(n, s) for n, s in S.read_fasta(fasta)]
    ref = S.RefModel.from_fasta(fasta, levels, K, 0, a.query)
    length = len(recs[0][1])
    # three intervals, about a tenth of the contig
    targets = [(0, 2000, 3000), (0, 14000, 15200), (0, 25500, 26300)]
    covered = sum(e - b for _, b, e in targets)
    say(f"build {S.build_id()}  reference {recs[0][0]} {length} bases  targets {targets} = {covered} bases ({100.0 * covered / length:.1f}%)")
    say(f"reads {a.reads} kinds {KINDS}  channels {a.channels}  chunk {a.chunk}  skip {SKIP} norm {NORM} query {a.query}  seed {a.seed}")
    reads, where = synth.make_dna_raw_reads_truth(recs, levels, K, a.reads, seed=a.seed, kinds=KINDS)
    true_t = np.array([w is not None and S.truth_class(targets, *w[:3]) == "T" for w in where])
    edge = np.array([w is not None and S.truth_edge(targets, *w[:3]) for w in where])
    mapped = np.array([w is not None for w in where])
    size = np.array([len(r[5]) for r in reads], np.int64)
    say(f"truth: {int(true_t.sum())} reads on target (T), of them {int(edge.sum())} edge reads; {int((~true_t).sum())} off target (O), of them {int((~mapped).sum())} that belong nowhere; "
        f"samples in the file {int(size.sum())}, on target {int(size[true_t].sum())} ({100.0 * size[true_t].sum() / size.sum():.2f}%)")

    t0 = time.time()
    with S.Aligner(ref, 0) as al:
        records, ticks = observe(al, reads, a.channels, a.chunk, a.query, targets, say)
    say(f"observed {sum(len(r) for r in records)} records in {ticks} ticks, {time.time() - t0:.1f} s wall (one extend_raw and one classes call per tick)")

    # the records as arrays [read, tick], padded with undecidable entries
    width = max(len(r) for r in records)
    n = np.zeros((len(records), width), np.int64)
    on = np.full((len(records), width), np.inf, np.float32)
    off = np.full((len(records), width), np.inf, np.float32)
    ok = np.zeros((len(records), width), bool)
    sent = np.zeros((len(records), width), np.int64)
    last = np.array([len(r) - 1 for r in records])
    for i, r in enumerate(records):
        for k, (ne, a_on, a_off, cal, s) in enumerate(r):
            n[i, k], on[i, k], off[i, k], ok[i, k], sent[i, k] = ne, a_on, a_off, cal, s

    # the numpy rule against the library's on a sample of the records
    rng = np.random.default_rng(0)
    rec = np.zeros(1, S.CLASS_DTYPE)
    checked = 0
    for i in rng.integers(0, len(records), 400):
        for k in range(len(records[i])):
            for me, mg in ((30, 0.02), (100, 0.2)):
                rec["on_score"], rec["off_score"], rec["n_events"], rec["valid"] = on[i, k], off[i, k], n[i, k], int(ok[i, k])
                rec["on_rid"], rec["off_rid"] = (-1 if np.isinf(on[i, k]) else 0), (-1 if np.isinf(off[i, k]) else 0)
                want = {"A": 1, "U": -1, None: 0}[S.target_decide(rec[0], S.ENRICH, me, mg)]
                got = int(decide(n[i:i + 1, k], on[i:i + 1, k], off[i:i + 1, k], ok[i:i + 1, k], me, mg)[0])
                assert got == want, (i, k, me, mg, rec, got, want)
                checked += 1
    say(f"the offline rule equals sfa_target_decide on {checked} sampled records")

    file_share = size[true_t].sum() / size.sum()
    say("")
    say("| min_events | margin | decided before the end | T reads decided, right | O reads decided, right | edge reads decided, right | mean events at decision | mean samples at decision | on-target share sequenced | enrichment by signal |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    rows = np.arange(len(records))
    for me in MIN_EVENTS:
        for mg in MARGINS:
            d = decide(n, on, off, ok, me, mg)
            has = (d != 0).any(axis=1)
            first = np.where(has, (d != 0).argmax(axis=1), last)
            cls = d[rows, first]
            early = has & (first < last)
            t_dec, o_dec, e_dec = has & true_t & ~edge, has & ~true_t, has & edge

            def right(sel, of, want):
                return f"{int(sel.sum())} of {int(of.sum())}, " + (f"{100.0 * (cls[sel] == want).mean():.1f}%" if sel.any() else "-")

            t_all, o_all = true_t & ~edge, ~true_t
            sequenced = np.where(cls == -1, sent[rows, first], size)  # --enrich: unblocked at the decision, else to the read's end
            share = sequenced[true_t].sum() / sequenced.sum()
            say(f"| {me} | {mg} | {100.0 * early.mean():.1f}% | {right(t_dec, t_all, 1)} | {right(o_dec, o_all, -1)} | {right(e_dec, edge, 1)} T | "
                f"{n[rows, first][has].mean() if has.any() else float('nan'):.1f} | "
                f"{sent[rows, first][has].mean() if has.any() else float('nan'):.0f} | {100.0 * share:.2f}% | {share / file_share:.3f} |")
    say("")
    say("right: the decided class equals the true class, among the reads of that true class that were decided at all (edge reads apart: share decided on target).")
    say("on-target share sequenced: samples of true-T reads among all samples sequenced under --enrich; enrichment: that share over the file's share.")
    log.close()


if __name__ == "__main__":
    main()
