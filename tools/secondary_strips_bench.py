#!/usr/bin/env python3
"""What secondary mappings cost on reads beyond 2048 events (option "secondary_strips"): one batch of long reads, align_db with

  A  "secondary" 0                          (the row strips as they always ran)
  B  "secondary" 4, "secondary_strips" 0    (the baseline: the wave path's secondary kernels run over a batch without short reads,
                                             the long reads' slots stay valid = 0)
  C  "secondary" 4, "secondary_strips" 1    (pass 1 keeps the lists, a merge, pass 2 once more per rank, the rows)

interleaved A B C A B C ..., in one context, at the strip benchmarks' own shapes (--shapes, default the `ncov_r9_dna_q3000` and
`ncov_r9_dna_q8000` workloads of bench.py: 8 333 reads of 3 000 events, 3 125 of 8 000).  Every call is timed by the wall clock and
by the context's HIP events (sfa_get_profile: total = first to last event of the batch on its stream, the join with the strips'
streams included).  Prints the medians, checks that the primaries are the same bytes in all three and that C fills the slots.  For
the per-kernel split run it under `rocprofv3 --kernel-trace --stats -- python tools/secondary_strips_bench.py --rounds 2 --no-log`.

    python tools/secondary_strips_bench.py [--rounds 5] [--shapes 8333x3000,3125x8000] [--out DIR]
    (log: DIR/secondary_strips_bench.log, default profiles/secondary_strips_<build id>/)
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

SETTINGS = {"A": (0, 0), "B": (4, 0), "C": (4, 1)}  # name: ("secondary", "secondary_strips")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="8333x3000,3125x8000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-log", action="store_true")
    a = ap.parse_args()
    log = None
    if not a.no_log:
        out = a.out or os.path.join(ROOT, "profiles", f"secondary_strips_{S.build_id()}")
        os.makedirs(out, exist_ok=True)
        log = open(os.path.join(out, "secondary_strips_bench.log"), "a")

    def say(s):
        print(s, flush=True)
        if log:
            log.write(s + "\n")
            log.flush()

    say(f"# build {S.build_id()}  {time.strftime('%Y-%m-%d %H:%M:%S')}  rounds {a.rounds}, interleaved A B C")
    for shape in a.shapes.split(","):
        n, qlen = (int(x) for x in shape.split("x"))
        ref, flag, q, q_off, _ = synth.workload(f"ncov_r9_dna_q{qlen}", n_reads=n, seed=3)
        n_long = int(((q_off[1:] - q_off[:-1]) > 2048).sum())
        with S.Aligner(ref, flag) as al:
            def call(name):
                n_sec, strips = SETTINGS[name]
                al.set_secondary(n_sec)
                al.set_option("secondary_strips", strips)
                t0 = time.perf_counter()
                rows = al.align_db(q, q_off)
                wall = (time.perf_counter() - t0) * 1e3
                p = al.profile()
                filled = int(al.secondary_rows()["valid"].sum()) if n_sec else 0
                return rows.tobytes(), wall, p["total_ms"], filled

            for name in SETTINGS:  # warm-up: every buffer of every setting is allocated
                call(name)
            wall, dev, prim, filled = {k: [] for k in SETTINGS}, {k: [] for k in SETTINGS}, {}, {}
            for r in range(a.rounds):
                for name in SETTINGS:
                    rows, w, d, f = call(name)
                    assert prim.setdefault(name, rows) == rows
                    wall[name].append(w)
                    dev[name].append(d)
                    filled[name] = f
                    say(f"{n} x {qlen} round {r} {name}: wall {w:.2f} ms  HIP events {d:.2f} ms  valid secondary rows {f}")
        assert prim["A"] == prim["B"] == prim["C"], "primaries differ between the settings"
        assert filled["C"] > filled["B"] and filled["C"] >= 4 * n_long * 0.9, (filled, n_long)
        say(f"{n} reads x {qlen} events on nCoV ({n_long} beyond 2048 events): primaries identical in A, B and C")
        for name, (n_sec, strips) in SETTINGS.items():
            say(f"  {name} secondary {n_sec} secondary_strips {strips}: wall median {np.median(wall[name]):.2f} ms (min {min(wall[name]):.2f}, max {max(wall[name]):.2f}); "
                f"HIP events median {np.median(dev[name]):.2f} ms (min {min(dev[name]):.2f}, max {max(dev[name]):.2f}); valid secondary rows {filled[name]}")
        say(f"  C / B: wall {np.median(wall['C']) / np.median(wall['B']):.3f}, HIP events {np.median(dev['C']) / np.median(dev['B']):.3f};  "
            f"B / A: wall {np.median(wall['B']) / np.median(wall['A']):.3f}, HIP events {np.median(dev['B']) / np.median(dev['A']):.3f}")


if __name__ == "__main__":
    main()
