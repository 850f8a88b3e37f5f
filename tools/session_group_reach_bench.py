#!/usr/bin/env python3
"""Reach groups, measured against plain target groups on the same build: what Session.set_reach_target_groups costs (the runs
prepared on the host, their upload, session_reach_label_build_kernel) against Session.set_target_groups (the table built on the
host and uploaded); what one Session.add_coverage call costs under a group cap on a reach label table
(session_reach_label_live_kernel: the depth read at the column's anchor) against a plain table (session_cover_label_kernel, the
parent's code); and Session.open_classes on a reach table against a plain one -- the kernel is the same, so that should be level.

Two references: nCoV (tests/golden/data, 30 kb) and a synthetic contig of 1 Mb; 1, 64 and 1023 groups; sessions of 512 slots with
300 events each; targets of 2 kb spread evenly over the contig (a twentieth of it; at least as many as groups on the 1 Mb
reference, group = index mod n_groups), for the reach session with a lead of 1 kb and alternating strands; group cap 30; 512
intervals of 2 kb per add.  Every round runs A then B then, in the next round, B then A (interleaved, both orders): wall time
around the call, and for the add and open_classes the device time from the context's HIP events (profile()["class_ms"]).
Medians and [min, max] over the rounds after a warm-up round.

    python tools/session_group_reach_bench.py [--rounds 11] [--slots 512] [--intervals 512] [--out DIR]
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

K, LENGTH, LEAD, CAP, EVENTS = 6, 2000, 1000, 30, 300


def measure(name, ref, n_groups, args, say):
    rng = np.random.default_rng(7)
    rl, off = int(ref.ref_lengths[0]), int(ref.st_offset[0])
    n_t = max(3, rl // (20 * LENGTH))  # (a twentieth of the contig; the 30 kb reference gets three)
    begins = off + (np.arange(n_t) * (rl // n_t)) + LEAD
    plain_t = np.zeros(n_t, S.GROUP_TARGET_DTYPE)
    plain_t["begin"], plain_t["end"], plain_t["group"] = begins, np.minimum(begins + LENGTH, off + rl + 1), np.arange(n_t) % n_groups
    reach_t = np.zeros(n_t, S.REACH_GROUP_TARGET_DTYPE)
    for f in ("contig", "begin", "end", "group"):
        reach_t[f] = plain_t[f]
    reach_t["lead"], reach_t["strand"] = LEAD, np.where(np.arange(n_t) % 2, ord("-"), ord("+"))
    keys = ("set_target_groups wall", "set_reach_target_groups wall", "plain add wall", "plain add device", "reach add wall", "reach add device", "plain open wall",
            "plain open device", "reach open wall", "reach open device")
    rows = {k: [] for k in keys}
    slots = np.arange(args.slots, dtype=np.int32)
    with S.Aligner(ref, 0) as al, al.session(args.slots) as plain, al.session(args.slots) as reach:
        ev = (rng.integers(-6, 7, args.slots * EVENTS) / 4).astype(np.float32)
        offs = (np.arange(args.slots + 1) * EVENTS).astype(np.int64)
        for se in (plain, reach):
            se.extend(slots, ev, offs)

        def timed(fn, key, device=None):
            t0 = time.perf_counter()
            fn()
            out = {f"{key} wall": (time.perf_counter() - t0) * 1e3}
            if device:
                out[f"{key} device"] = al.profile()["class_ms"]
            return out

        set_plain = lambda: timed(lambda: plain.set_target_groups(plain_t, n_groups), "set_target_groups")
        set_reach = lambda: timed(lambda: reach.set_reach_target_groups(reach_t, n_groups), "set_reach_target_groups")
        set_plain(), set_reach()
        plain.configure_group_coverage(CAP), reach.configure_group_coverage(CAP)
        for r in range(args.rounds + 1):  # (round 0 warms up)
            b = rng.integers(off, off + rl + 1 - min(LENGTH, rl), args.intervals)
            iv = np.zeros(args.intervals, S.TARGET_DTYPE)
            iv["begin"], iv["end"] = b, b + min(LENGTH, rl)
            calls = [set_plain, set_reach, lambda: timed(lambda: plain.add_coverage(iv), "plain add", True), lambda: timed(lambda: reach.add_coverage(iv), "reach add", True),
                     lambda: timed(lambda: plain.open_classes(slots), "plain open", True), lambda: timed(lambda: reach.open_classes(slots), "reach open", True)]
            if r % 2:
                calls = [calls[1], calls[0], calls[3], calls[2], calls[5], calls[4]]
            for call in calls:
                for key, v in call().items():
                    if r:
                        rows[key].append(v)
            assert np.array_equal(plain.coverage(0), reach.coverage(0))  # the same intervals went to both sessions: one depth
        labelled = int((reach.group_reach_tables()[0] != n_groups).sum())
        say(f"{name}, {n_groups} groups: {ref.total_columns()} columns, {args.slots} slots of {EVENTS} events, {n_t} targets of {LENGTH} (reach: lead {LEAD}, strands alternating, "
            f"{labelled} labelled columns), {args.intervals} intervals of {min(LENGTH, rl)} per add, group cap {CAP}, {args.rounds} rounds; tables "
            f"{S.session_group_reach_bytes(ref, 0)} bytes")
    for key, v in rows.items():
        say(f"  {key:30s} median {np.median(v):9.4f} ms  [{min(v):.4f}, {max(v):.4f}]")
    med = lambda k: float(np.median(rows[k]))
    say(f"  set_reach_target_groups / set_target_groups (wall medians): {med('set_reach_target_groups wall') / med('set_target_groups wall'):.3f}")
    say(f"  reach add / plain add (device medians): {med('reach add device') / med('plain add device'):.3f}; (wall medians): {med('reach add wall') / med('plain add wall'):.3f}")
    say(f"  reach open / plain open (device medians): {med('reach open device') / med('plain open device'):.3f}; (wall medians): {med('reach open wall') / med('plain open wall'):.3f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--intervals", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", f"session_group_reach_{S.build_id()}")
    os.makedirs(out, exist_ok=True)
    log = open(os.path.join(out, "bench.log"), "w")

    def say(text):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    say(f"session_group_reach_bench: build {S.build_id()}, version {S.version()}")
    levels = synth.kmer_levels(K, 21)
    ncov = S.RefModel.from_fasta(os.path.join(ROOT, "tests", "golden", "data", "nCoV-2019.reference.fasta"), levels, K, 0, 250)
    big = S.RefModel.from_records([("syn1m", synth.random_sequence(1_000_000 + K - 1, 3))], levels, K, 0, 250)
    for n_groups in (1, 64, 1023):
        measure("nCoV", ncov, n_groups, args, say)
        measure("synthetic 1 Mb", big, n_groups, args, say)


if __name__ == "__main__":
    main()
