#!/usr/bin/env python3
"""Group caps, measured.  Three things, each against what a client has to do WITHOUT the feature for the same answer:

  add        one Session.add_coverage call with a group cap on (the depth update and the live label table, on the device) against
             the host's way: keep depth on the host, cut every group's intervals into the still-open pieces (timed apart: `host
             pieces`) and call Session.set_target_groups again, which rebuilds the label table on the host and uploads it.
  classes    Session.open_classes and Session.group_bests of every slot with the cap on against the same calls on a session with
             the cap off: the kernels are the same, only the table's pointer differs, so the two are expected equal within the
             calls' own spread, which is printed beside them.  (The cap-off session was just given a new table; one open_classes
             call on it goes untimed first, so that the host's search for the labels' first columns is not in the comparison.)
  records    Session.group_coverage alone against copying every track back through Session.coverage and reducing on the host.

Two references: nCoV (tests/golden/data, 30 kb; 512 slots) and a synthetic contig of 1 Mb (16 slots: 512 rows of 2 M columns do
not fit beside each other); groups are equal runs of coordinates over the whole contig, n_groups 16 and 1023; 512 intervals of
2 kb per call.  Interleaved rounds after a warm-up round; wall time around the calls, device time from the context's HIP events
(profile()["class_ms"]); medians with [min, max].  The rows are cache-warm, nothing is profiled, the clock is not read.

    python tools/session_group_cover_bench.py [--rounds 9] [--intervals 512] [--length 2000] [--cap 30] [--out DIR]
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

K, TICK_S = 6, 1600 / 4000.0


def group_runs(rl, off, n_groups):
    """n_groups equal runs of coordinates over [off, off + rl + 1): (contig 0, begin, end, group)"""
    edges = np.linspace(0, rl + 1, n_groups + 1).astype(np.int64)
    return [(0, off + int(a), off + int(b), g) for g, (a, b) in enumerate(zip(edges[:-1], edges[1:])) if b > a], edges


def open_pieces(depth, cap, off, edges):
    """every group's coordinates with depth below cap as (0, begin, end, group) runs: what a client without the feature uploads"""
    out = []
    below = depth < cap
    for g, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        m = np.concatenate([[False], below[a:b], [False]])
        e = np.flatnonzero(m[1:] != m[:-1])
        out += [(0, off + int(a + x), off + int(a + y), g) for x, y in zip(e[::2], e[1::2])]
    return out


def host_records(tracks, edges, cap):
    """the records of every group from a contig's track, on the host (forward-strand columns: coordinates 0 .. rl - 1)"""
    d = tracks[:-1].astype(np.int64)
    idx = edges[:-1].clip(max=len(d) - 1)
    return np.add.reduceat(d, idx), np.add.reduceat((d >= cap).astype(np.int64), idx), np.minimum.reduceat(d, idx), np.maximum.reduceat(d, idx)


def stats(v):
    return f"median {np.median(v):9.4f} ms  [{min(v):.4f}, {max(v):.4f}]"


def measure(name, ref, n_slots, n_groups, args, say):
    rng = np.random.default_rng(7)
    rl, off = int(ref.ref_lengths[0]), int(ref.st_offset[0])
    targets, edges = group_runs(rl, off, n_groups)
    depth = np.zeros(rl + 1, np.int64)
    keys = ["add wall", "add device", "set_target_groups wall", "host pieces", "open_classes cap on", "open_classes cap off", "group_bests cap on", "group_bests cap off",
            "group_coverage wall", "group_coverage device", "coverage() + host reduce"]
    rows = {k: [] for k in keys}
    slots = list(range(n_slots))
    with S.Aligner(ref, 0) as al, al.session(n_slots, starts=False) as capped, al.session(n_slots, starts=False) as plain:
        ev = (rng.integers(-6, 7, 40 * n_slots) / 4).astype(np.float32)
        ev_off = np.arange(0, 40 * n_slots + 1, 40, dtype=np.int64)
        for se in (capped, plain):
            se.extend(slots, ev, ev_off)
            se.set_target_groups(targets, n_groups)
        capped.configure_group_coverage(args.cap)
        for r in range(args.rounds + 1):  # (round 0 warms up)
            length = min(args.length, rl)
            begin = rng.integers(off, off + rl + 1 - length, args.intervals)
            iv = np.zeros(args.intervals, S.TARGET_DTYPE)
            iv["begin"], iv["end"] = begin, begin + length
            t = {}
            t0 = time.perf_counter()
            capped.add_coverage(iv)
            t["add wall"] = (time.perf_counter() - t0) * 1e3
            t["add device"] = al.profile()["class_ms"]
            np.add.at(depth, np.concatenate([np.arange(b - off, e - off) for b, e in zip(iv["begin"], iv["end"])]), 1)  # (the client's own book-keeping: not timed)
            t0 = time.perf_counter()
            pieces = open_pieces(depth, args.cap, off, edges)
            t["host pieces"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            plain.set_target_groups(pieces if pieces else targets[:1], n_groups)
            t["set_target_groups wall"] = (time.perf_counter() - t0) * 1e3
            plain.open_classes(slots)  # (not timed: the first call behind a new table finds the labels' first columns on the host)
            for key, call in (("open_classes", lambda se: se.open_classes(slots)), ("group_bests", lambda se: se.group_bests(slots))):
                got = {}
                for which, se in (("cap on", capped), ("cap off", plain)):
                    t0 = time.perf_counter()
                    got[which] = call(se)
                    t[f"{key} {which}"] = (time.perf_counter() - t0) * 1e3
                a, b = got["cap on"], got["cap off"]
                same = a.tobytes() == b.tobytes() if key == "open_classes" else (a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes())
                if pieces and not same:
                    raise SystemExit(f"{name}: round {r}: {key} differs between the capped session and the one given the open pieces")
            t0 = time.perf_counter()
            rec = capped.group_coverage()
            t["group_coverage wall"] = (time.perf_counter() - t0) * 1e3
            t["group_coverage device"] = al.profile()["class_ms"]
            t0 = time.perf_counter()
            s, c, lo, hi = host_records(capped.coverage(0), edges, args.cap)
            t["coverage() + host reduce"] = (time.perf_counter() - t0) * 1e3
            live = [g for g, (a, b) in enumerate(zip(edges[:-1], edges[1:])) if min(b, rl) > a]
            if not (np.array_equal(rec["depth_sum"][live].astype(np.int64), s[live]) and np.array_equal(rec["capped"][live], c[live])):
                raise SystemExit(f"{name}: round {r}: group_coverage and the host's reduction of the tracks differ")
            if r:
                for k in keys:
                    rows[k].append(t[k])
        say(f"{name}, {n_groups} groups: {ref.total_columns()} columns, {n_slots} slots, {args.intervals} intervals of {length} per call, cap {args.cap}, {args.rounds} rounds; "
            f"group cap memory {S.session_group_coverage_bytes(ref, n_groups, 0)} bytes")
    for k in keys:
        say(f"  {k:26s} {stats(rows[k])}  = {100 * np.median(rows[k]) / 1e3 / TICK_S:.4f} % of a tick's {TICK_S} s of signal")
    say(f"  add_coverage wall / (host pieces + set_target_groups wall), medians: {np.median(rows['add wall']) / (np.median(rows['host pieces']) + np.median(rows['set_target_groups wall'])):.3f}")
    say(f"  group_coverage wall / (coverage() + host reduce), medians: {np.median(rows['group_coverage wall']) / np.median(rows['coverage() + host reduce']):.3f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--intervals", type=int, default=512)
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--cap", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", f"session_group_cover_{S.build_id()}")
    os.makedirs(out, exist_ok=True)
    log = open(os.path.join(out, "bench.log"), "w")

    def say(text):
        print(text)
        log.write(text + "\n")
        log.flush()

    say(f"session_group_cover_bench: build {S.build_id()}, version {S.version()}")
    levels = synth.kmer_levels(K, 21)
    ncov = S.RefModel.from_fasta(os.path.join(ROOT, "tests", "golden", "data", "nCoV-2019.reference.fasta"), levels, K, 0, 250)
    big = S.RefModel.from_records([("syn1m", synth.random_sequence(1_000_000 + K - 1, 3))], levels, K, 0, 250)
    for n_groups in (16, 1023):
        measure("nCoV", ncov, 512, n_groups, args, say)
        measure("synthetic 1 Mb", big, 16, n_groups, args, say)
    say(f"log: {os.path.relpath(os.path.join(out, 'bench.log'), ROOT)}")


if __name__ == "__main__":
    main()
