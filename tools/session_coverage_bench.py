#!/usr/bin/env python3
"""Coverage caps, measured: what one Session.add_coverage call costs (512 intervals of 2 kb: the depth update and the live mask, on
the device) against what a client has to do WITHOUT the feature for the same effect -- keep depth on the host, cut its target
list into the still-open pieces and call Session.set_targets again, which rebuilds the whole mask on the host and uploads it.

Two references: nCoV (tests/golden/data, 30 kb) and a synthetic contig of 1 Mb; the whole reference is the target; cap 30.  Per
round, interleaved: one add_coverage call (wall time around the call; device time from the context's HIP events, profile()
["class_ms"]), then on a second session the baseline: the open pieces from a numpy depth track (timed apart: `host pieces`) and
set_targets(pieces) (wall).  After every round the two sessions must report the same number of on-target columns.  Medians and
[min, max] over the rounds after a warm-up round; the yardstick is a tick's signal time, 1600 samples / 4000 Hz = 0.4 s.

    python tools/session_coverage_bench.py [--rounds 9] [--intervals 512] [--length 2000] [--cap 30] [--out DIR]
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


def open_pieces(depth, cap, off):
    """the runs of coordinates with depth below cap as (0, begin, end) targets: what a client without the feature hands set_targets"""
    below = np.concatenate([[False], depth < cap, [False]])
    edges = np.flatnonzero(below[1:] != below[:-1])
    return [(0, int(a) + off, int(b) + off) for a, b in zip(edges[::2], edges[1::2])]


def measure(name, ref, args, say):
    rng = np.random.default_rng(7)
    rl, off = int(ref.ref_lengths[0]), int(ref.st_offset[0])
    depth = np.zeros(rl + 1, np.int64)
    rows = {"add wall": [], "add device": [], "set_targets wall": [], "host pieces": []}
    with S.Aligner(ref, 0) as al, al.session(1) as cover, al.session(1) as plain:
        cover.set_targets([(0, off, off + rl + 1)])
        cover.configure_coverage(args.cap)
        for r in range(args.rounds + 1):  # (round 0 warms up)
            begin = rng.integers(off, off + rl + 1 - min(args.length, rl), args.intervals)
            iv = np.zeros(args.intervals, S.TARGET_DTYPE)
            iv["begin"], iv["end"] = begin, begin + min(args.length, rl)
            t0 = time.perf_counter()
            n_open = cover.add_coverage(iv)
            t1 = time.perf_counter()
            dev = al.profile()["class_ms"]
            np.add.at(depth, np.concatenate([np.arange(b - off, e - off) for b, e in zip(iv["begin"], iv["end"])]), 1)  # (the client's own book-keeping: not timed)
            t2 = time.perf_counter()
            pieces = open_pieces(depth, args.cap, off)
            t3 = time.perf_counter()
            plain.set_targets(pieces if pieces else [(0, off, off + 1)])
            t4 = time.perf_counter()
            if pieces and plain.target_columns() != n_open:
                raise SystemExit(f"{name}: round {r}: add_coverage left {n_open} open columns, set_targets(pieces) {plain.target_columns()}")
            if r:
                for key, v in (("add wall", (t1 - t0) * 1e3), ("add device", dev), ("set_targets wall", (t4 - t3) * 1e3), ("host pieces", (t3 - t2) * 1e3)):
                    rows[key].append(v)
        say(f"{name}: {ref.total_columns()} columns, {args.intervals} intervals of {min(args.length, rl)} per call, cap {args.cap}, {args.rounds} rounds; open columns at the end {n_open}, "
            f"coverage memory {S.session_coverage_bytes(ref, 0)} bytes")
    for key, v in rows.items():
        say(f"  {key:18s} median {np.median(v):9.4f} ms  [{min(v):.4f}, {max(v):.4f}]  = {100 * np.median(v) / 1e3 / TICK_S:.4f} % of a tick's {TICK_S} s of signal")
    say(f"  add_coverage wall / set_targets wall (medians): {np.median(rows['add wall']) / np.median(rows['set_targets wall']):.3f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--intervals", type=int, default=512)
    ap.add_argument("--length", type=int, default=2000)
    ap.add_argument("--cap", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "profiles", f"session_coverage_{S.build_id()}")
    os.makedirs(out, exist_ok=True)
    log = open(os.path.join(out, "bench.log"), "w")

    def say(text):
        print(text)
        log.write(text + "\n")
        log.flush()

    say(f"session_coverage_bench: build {S.build_id()}, version {S.version()}")
    levels = synth.kmer_levels(K, 21)
    ncov = S.RefModel.from_fasta(os.path.join(ROOT, "tests", "golden", "data", "nCoV-2019.reference.fasta"), levels, K, 0, 250)
    measure("nCoV", ncov, args, say)
    big = S.RefModel.from_records([("syn1m", synth.random_sequence(1_000_000 + K - 1, 3))], levels, K, 0, 250)
    measure("synthetic 1 Mb", big, args, say)
    say(f"log: {os.path.relpath(os.path.join(out, 'bench.log'), ROOT)}")


if __name__ == "__main__":
    main()
