#!/usr/bin/env python3
"""Device time of sfa_session_open_classes beside sfa_session_classes and sfa_session_group_bests (heads only) on the same session
in the same process: 512 slots x the nCoV reference.  Times are HIP events on the context's stream (sfa_get_profile: class_ms of
each call), 5 repeats, interleaved: every repeat runs the class call and then, per label layout, the group call and the open-class
call under two bitmaps (every group open; every second group closed), after one warm-up round.  The layouts: n_groups = 1, 16 and
1023 with long runs (the row cut into n_groups equal stretches), and 1023 single-column groups (the rest of the row is background).
The rows were written just before and partly sit in the last-level cache: this is no HBM measurement.

    python tools/session_quota_bench.py [--slots 512] [--events 100] [--repeats 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sigfish_amd as S  # noqa: E402
from sigfish_amd import _lib, synth  # noqa: E402


def stretches(rl, n):
    """the contig's coordinates [0, rl + 1) cut into n stretches, group g the g-th"""
    edges = np.linspace(0, rl + 1, n + 1).astype(np.int64)
    return [(0, int(edges[g]), int(edges[g + 1]), g) for g in range(n) if edges[g + 1] > edges[g]]


def show(name, t, cls):
    t, r = np.array(t), np.array(t) / cls
    print(f"  {name}: class_ms {' '.join(f'{x:.4f}' for x in t)} (median {np.median(t):.4f}, min {t.min():.4f}, max {t.max():.4f}); ratio to classes per repeat "
          f"{' '.join(f'{x:.3f}' for x in r)} (median {np.median(r):.3f}, min {r.min():.3f}, max {r.max():.3f})")


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
        cls = []
        times = {name: {"group_bests (heads)": [], "open_classes, all open": [], "open_classes, every second closed": []} for name, _, _ in cases}
        for k in range(a.repeats + 1):  # (round 0 warms up: first launches, buffers grown)
            got = se.classes(slots)
            cls.append(al.profile()["class_ms"])
            assert (got["valid"] == 1).all()
            for name, gt, n_groups in cases:
                se.set_target_groups(gt, n_groups)
                heads = np.zeros(a.slots, S.GROUP_HEAD_DTYPE)
                rc = se._L.sfa_session_group_bests(se._h, slots.ctypes.data_as(_lib.i32p), a.slots, None, heads.ctypes.data_as(_lib.C.c_void_p))  # heads only
                assert rc == 0 and (heads["valid"] == 1).all()
                times[name]["group_bests (heads)"].append(al.profile()["class_ms"])
                half = np.zeros(S.open_words(n_groups), np.uint32)
                for g in range(0, n_groups, 2):
                    half[g >> 5] |= np.uint32(1 << (g & 31))
                for key, bits in (("open_classes, all open", None), ("open_classes, every second closed", half)):
                    rec = se.open_classes(slots, bits)
                    times[name][key].append(al.profile()["class_ms"])
                    assert (rec["cls"]["valid"] == 1).all()
        cls = np.array(cls[1:])
        print(f"classes: class_ms {' '.join(f'{x:.4f}' for x in cls)} (median {np.median(cls):.4f}, min {cls.min():.4f}, max {cls.max():.4f}); "
              f"{(a.slots * cols * 4 + cols // 8 + 36 * a.slots) / np.median(cls) / 1e6:.1f} GB/s at the median")
        for name, _, _ in cases:
            print(name)
            for key, t in times[name].items():
                show(key, t[1:], cls)


if __name__ == "__main__":
    main()
