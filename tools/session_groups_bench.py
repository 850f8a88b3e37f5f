#!/usr/bin/env python3
"""Device time of sfa_session_group_bests beside sfa_session_classes on the same session in the same process: 512 slots x the nCoV
reference.  Times are HIP events on the context's stream (sfa_get_profile: class_ms of either call -- for group_bests the memset of
the keys, the labelled reduction and the heads kernel, which also writes the [slots][n_groups + 1] result records), 5 repeats,
interleaved: every repeat runs the class call and then each group case once, after one warm-up round.  The cases: n_groups = 1, 16
and 1023 with long runs (the row cut into n_groups equal stretches), and 1023 single-column groups, the worst case (every lane
flushes at every column of that stretch; the rest of the row is background).  The traffic of a group call is what it must read and
write: the named slots' cost rows once (4 bytes per column), the labels once (2 bytes per column), keys and results.

    python tools/session_groups_bench.py [--slots 512] [--events 100] [--repeats 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sigfish_amd as S  # noqa: E402
from sigfish_amd import synth  # noqa: E402


def stretches(rl, n):
    """the contig's coordinates [0, rl + 1) cut into n stretches, group g the g-th"""
    edges = np.linspace(0, rl + 1, n + 1).astype(np.int64)
    return [(0, int(edges[g]), int(edges[g + 1]), g) for g in range(n) if edges[g + 1] > edges[g]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--events", type=int, default=100, help="events every slot holds")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    ref, flag, q, q_off, _ = synth.workload("ncov_r9_dna_q250", n_reads=a.slots, seed=3)
    cols = ref.total_columns()
    rl = int(ref.ref_lengths[0])
    print(f"build {S.build_id()}  slots {a.slots}  columns per slot {cols}  events per slot {a.events}")
    cases = [("1 group, long runs", stretches(rl, 1), 1), ("16 groups, long runs", stretches(rl, 16), 16), ("1023 groups, long runs", stretches(rl, 1023), 1023),
             ("1023 single-column groups", [(0, 5000 + g, 5001 + g, g) for g in range(1023)], 1023)]
    targets = [(0, 1000, 4000), (0, 20000, 21563), (0, rl - 500, rl + 1)]
    slots = np.arange(a.slots, dtype=np.int32)
    with S.Aligner(ref, flag) as al, al.session(a.slots) as se:
        chunks = [q[q_off[i]:][:a.events] for i in range(a.slots)]
        se.extend(slots, np.concatenate(chunks), np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.int64))
        se.set_targets(targets)
        cls, grp = [], {name: [] for name, _, _ in cases}
        for k in range(a.repeats + 1):  # (round 0 warms up: first launches, buffers grown)
            got = se.classes(slots)
            cls.append(al.profile()["class_ms"])
            assert (got["valid"] == 1).all()
            for name, gt, n_groups in cases:
                se.set_target_groups(gt, n_groups)
                _, heads = se.group_bests(slots)
                grp[name].append(al.profile()["class_ms"])
                assert (heads["valid"] == 1).all()
        cls = np.array(cls[1:])
        base = a.slots * cols * 4
        print(f"classes: class_ms {' '.join(f'{x:.4f}' for x in cls)} (median {np.median(cls):.4f}, min {cls.min():.4f}, max {cls.max():.4f}); "
              f"{(base + cols // 8 + 36 * a.slots) / np.median(cls) / 1e6:.1f} GB/s at the median")
        for name, _, n_groups in cases:
            t = np.array(grp[name][1:])
            traffic = base + 2 * cols + a.slots * ((n_groups + 1) * (8 + 8 + 16) + 24)  # rows, labels, keys set and read, results
            r = t / cls
            print(f"{name}: class_ms {' '.join(f'{x:.4f}' for x in t)} (median {np.median(t):.4f}, min {t.min():.4f}, max {t.max():.4f}); "
                  f"{traffic / np.median(t) / 1e6:.1f} GB/s at the median; ratio to classes per repeat {' '.join(f'{x:.3f}' for x in r)} "
                  f"(median {np.median(r):.3f}, min {r.min():.3f}, max {r.max():.3f})")


if __name__ == "__main__":
    main()
