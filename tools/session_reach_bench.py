#!/usr/bin/env python3
"""Reach targets, measured against plain targets on the same build: what Session.set_reach_targets costs (the runs prepared on the
host, their upload, the build kernel) against Session.set_targets (the mask built on the host and uploaded), and what one
Session.add_coverage call costs on a reach session (session_reach_live_kernel: the depth read at the column's anchor) against a
plain-target session (session_cover_mask_kernel, the parent's code).

Two references: nCoV (tests/golden/data, 30 kb) and a synthetic contig of 1 Mb; sessions of 512 slots; targets of 2 kb spread evenly
over the contig (a twentieth of it), for the reach session with a lead of 1 kb and alternating strands; cap 30; 512 intervals of
2 kb per add.  Every round runs A then B then, in the next round, B then A (interleaved, both orders): wall time around the
call, and for the add the device time from the context's HIP events (profile()["class_ms"]).  Medians and [min, max] over the
rounds after a warm-up round.  The expectation for the add is arithmetic only: the live kernel reads 4 bytes more per column.

    python tools/session_reach_bench.py [--rounds 11] [--slots 512] [--intervals 512] [--out DIR]
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

K, LENGTH, LEAD, CAP = 6, 2000, 1000, 30


def measure(name, ref, args, say):
    rng = np.random.default_rng(7)
    rl, off = int(ref.ref_lengths[0]), int(ref.st_offset[0])
    n_t = max(3, rl // (20 * LENGTH))  # (a twentieth of the contig; the 30 kb reference gets three)
    begins = off + (np.arange(n_t) * (rl // n_t)) + LEAD
    plain_t = np.zeros(n_t, S.TARGET_DTYPE)
    plain_t["begin"], plain_t["end"] = begins, np.minimum(begins + LENGTH, off + rl + 1)
    reach_t = np.zeros(n_t, S.REACH_TARGET_DTYPE)
    for f in ("contig", "begin", "end"):
        reach_t[f] = plain_t[f]
    reach_t["lead"], reach_t["strand"] = LEAD, np.where(np.arange(n_t) % 2, ord("-"), ord("+"))
    rows = {k: [] for k in ("set_targets wall", "set_reach_targets wall", "plain add wall", "plain add device", "reach add wall", "reach add device")}
    with S.Aligner(ref, 0) as al, al.session(args.slots) as plain, al.session(args.slots) as reach:

        def set_plain():
            t0 = time.perf_counter()
            plain.set_targets(plain_t)
            return {"set_targets wall": (time.perf_counter() - t0) * 1e3}

        def set_reach():
            t0 = time.perf_counter()
            reach.set_reach_targets(reach_t)
            return {"set_reach_targets wall": (time.perf_counter() - t0) * 1e3}

        def add(se, tag, iv):
            t0 = time.perf_counter()
            se.add_coverage(iv)
            wall = (time.perf_counter() - t0) * 1e3
            return {f"{tag} add wall": wall, f"{tag} add device": al.profile()["class_ms"]}

        set_plain(), set_reach()
        plain.configure_coverage(CAP), reach.configure_coverage(CAP)
        for r in range(args.rounds + 1):  # (round 0 warms up)
            b = rng.integers(off, off + rl + 1 - min(LENGTH, rl), args.intervals)
            iv = np.zeros(args.intervals, S.TARGET_DTYPE)
            iv["begin"], iv["end"] = b, b + min(LENGTH, rl)
            calls = [set_plain, set_reach, lambda: add(plain, "plain", iv), lambda: add(reach, "reach", iv)]
            if r % 2:
                calls = [calls[1], calls[0], calls[3], calls[2]]
            for call in calls:
                for key, v in call().items():
                    if r:
                        rows[key].append(v)
            for c in (0,):  # the same intervals went to both sessions: one depth
                assert np.array_equal(plain.coverage(c), reach.coverage(c))
        say(f"{name}: {ref.total_columns()} columns, {args.slots} slots, {n_t} targets of {LENGTH} (reach: lead {LEAD}, strands alternating), {args.intervals} intervals of "
            f"{min(LENGTH, rl)} per add, cap {CAP}, {args.rounds} rounds; live on-target columns at the end plain {plain.target_columns()} reach {reach.target_columns()}; "
            f"anchors {S.session_reach_bytes(ref, 0)} bytes")
    for key, v in rows.items():
        say(f"  {key:24s} median {np.median(v):9.4f} ms  [{min(v):.4f}, {max(v):.4f}]")
    say(f"  set_reach_targets / set_targets (wall medians): {np.median(rows['set_reach_targets wall']) / np.median(rows['set_targets wall']):.3f}")
    say(f"  reach add / plain add (device medians): {np.median(rows['reach add device']) / np.median(rows['plain add device']):.3f}; "
        f"(wall medians): {np.median(rows['reach add wall']) / np.median(rows['plain add wall']):.3f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--intervals", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", f"session_reach_{S.build_id()}")
    os.makedirs(out, exist_ok=True)
    log = open(os.path.join(out, "bench.log"), "w")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    say(f"session_reach_bench: build {S.build_id()}, version {S.version()}")
    levels = synth.kmer_levels(K, 21)
    ncov = S.RefModel.from_fasta(os.path.join(ROOT, "tests", "golden", "data", "nCoV-2019.reference.fasta"), levels, K, 0, 250)
    measure("nCoV", ncov, args, say)
    big = S.RefModel.from_records([("syn1m", synth.random_sequence(1_000_000 + K - 1, 3))], levels, K, 0, 250)
    measure("synthetic 1 Mb", big, args, say)


if __name__ == "__main__":
    main()
