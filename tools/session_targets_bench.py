#!/usr/bin/env python3
"""Device time of sfa_session_classes beside the sfa_session_extend call of the same process: 512 slots x the nCoV reference,
both session kinds (with start columns, SFA_SESSION_NO_START).  Times are HIP events on the context's stream (sfa_get_profile:
class_ms of the classes call, total_ms of the extend call), 5 repeats after a warm-up each; the traffic is what the call must read
and write -- the named slots' cost rows once (4 bytes per column), the mask once, the results (the partial minima the merge reads
are well under 1 % of that and are left out, so the figure does not depend on the kernel's part size) -- over class_ms, to be held against the HBM figure of the machine.

    python tools/session_targets_bench.py [--slots 512] [--chunk 50] [--repeats 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sigfish_amd as S  # noqa: E402
from sigfish_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=50, help="events per slot and extend call")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    ref, flag, q, q_off, _ = synth.workload("ncov_r9_dna_q250", n_reads=a.slots, seed=3)
    cols = ref.total_columns()
    traffic = a.slots * cols * 4 + cols // 8 + 36 * a.slots
    print(f"build {S.build_id()}  slots {a.slots}  columns per slot {cols}  bytes per classes call {traffic}")
    rl = int(ref.ref_lengths[0])
    targets = [(0, 1000, 4000), (0, 20000, 21563), (0, rl - 500, rl + 1)]
    slots = np.arange(a.slots, dtype=np.int32)
    with S.Aligner(ref, flag) as al:
        for starts in (True, False):
            with al.session(a.slots, starts=starts) as se:
                se.set_targets(targets)
                ext, cls = [], []
                for k in range(a.repeats + 1):  # (call 0 warms up: first launches, buffers grown)
                    chunks = [q[q_off[i] + k * a.chunk % 200:][:a.chunk] for i in range(a.slots)]
                    off = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.int64)
                    se.extend(slots, np.concatenate(chunks), off)
                    ext.append(al.profile()["total_ms"])
                    got = se.classes(slots)
                    cls.append(al.profile()["class_ms"])
                    assert (got["valid"] == 1).all()
                ext, cls = np.array(ext[1:]), np.array(cls[1:])
                kind = "with starts" if starts else "NO_START  "
                print(f"{kind}: on-target columns {se.target_columns()}; extend ({a.chunk} events per slot) total_ms {' '.join(f'{x:.3f}' for x in ext)} (median {np.median(ext):.3f})")
                print(f"{kind}: classes class_ms {' '.join(f'{x:.4f}' for x in cls)} (median {np.median(cls):.4f}, min {cls.min():.4f}, max {cls.max():.4f}); "
                      f"{traffic / np.median(cls) / 1e6:.1f} GB/s at the median, {traffic / cls.min() / 1e6:.1f} GB/s at the best")


if __name__ == "__main__":
    main()
