#!/usr/bin/env python3
"""What the option "map_strips" changes about sfa_event_maps for rows beyond 2048 events: one call over a batch of long rows with the
option on (band fill in row strips on the device) against the same call with it off (band_traceback per row on the calling
thread, inside the call), in one process on the same rows.

Per shape (--shapes ROWSxEVENTS,..., default 256x3000,64x8000; synthetic R9 reads on nCoV): align_db once, then --warmup calls and
--reps timed calls of each setting, alternating.  Every call is timed by the wall clock and by a pair of HIP events on the
context's stream around it (the call is blocking and ends with a stream synchronisation, so the two differ by the host work
outside the stream: planning, the host rows).  Prints median, minimum and maximum, the pairs and band cells of the batch, and
whether the maps are the same bytes; lines are stamped with the build id and appended to
profiles/map_strips_<build id>/map_strips_bench.log (--no-log: stdout only)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sigfish_amd as S  # noqa: E402
from sigfish_amd import _lib, synth  # noqa: E402

LOG = None


def say(msg):
    line = f"[{S.build_id()}] {msg}"
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


def shape(a, n_rows, qlen):
    import torch
    ref, flag, q, q_off, _ = synth.workload(f"ncov_r9_dna_q{qlen}", n_reads=n_rows, seed=5)
    L = _lib.load()
    with S.Aligner(ref, flag, device=0) as al:
        rows = al.align_db(q, q_off)
        size = np.where((rows["valid"] == 1) & (rows["rid"] >= 0), rows["pos_end"].astype(np.int64) - rows["pos_st"] + 1, 0)
        off = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
        qlens = q_off[1:] - q_off[:-1]
        cells = int((size * qlens).sum())
        stream = torch.cuda.ExternalStream(al.stream())
        out = {1: np.zeros((int(off[-1]) + 1, 2), np.int32), 0: np.zeros((int(off[-1]) + 1, 2), np.int32)}
        on_host = C.c_int32(0)
        wall, dev, hosted = {0: [], 1: []}, {0: [], 1: []}, {}

        def call(on):
            al.set_option("map_strips", on)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            rc = L.sfa_event_maps(al._h, rows.ctypes.data_as(C.c_void_p), None, len(rows), off.ctypes.data_as(_lib.i64p), out[on].ctypes.data_as(_lib.i32p),
                                  C.byref(on_host))
            e1.record(stream)
            e1.synchronize()
            t = time.perf_counter() - t0
            assert rc == 0, L.sfa_last_error()
            hosted[on] = on_host.value
            return t * 1e3, e0.elapsed_time(e1)

        for _ in range(a.warmup):
            call(1), call(0)
        for _ in range(a.reps):
            for on in (1, 0):
                w, d = call(on)
                wall[on].append(w)
                dev[on].append(d)
    same = out[0].tobytes() == out[1].tobytes()
    say(f"{n_rows} rows x {qlen} events on nCoV: {int((size > 0).sum())} mapped, {int(off[-1])} pairs, {cells / 1e9:.2f} G band cells; {a.warmup} warm-up + {a.reps} calls each, alternating")
    for on in (1, 0):
        w, d = np.array(wall[on]), np.array(dev[on])
        say(f"  map_strips {on}: wall median {np.median(w):.1f} ms (min {w.min():.1f}, max {w.max():.1f}); HIP events median {np.median(d):.1f} ms "
            f"(min {d.min():.1f}, max {d.max():.1f}); rows on the host {hosted[on]}")
    say(f"  wall ratio off / on {np.median(wall[0]) / np.median(wall[1]):.1f}; maps {'==' if same else '!='}")
    return same


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x3000,64x8000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-log", action="store_true")
    ap.add_argument("--log-dir", default=None)
    a = ap.parse_args()
    if not a.no_log:
        d = a.log_dir or os.path.join(ROOT, "profiles", f"map_strips_{S.build_id()}")
        os.makedirs(d, exist_ok=True)
        LOG = os.path.join(d, "map_strips_bench.log")
    ok = True
    for s in a.shapes.split(","):
        n, ql = (int(x) for x in s.split("x"))
        ok = shape(a, n, ql) and ok
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
