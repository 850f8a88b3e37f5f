#!/usr/bin/env python3
"""Latency of Session.event_maps against what a caller had without it.

--slots (512) slots of a raw DNA session on the nCoV model, q = 250, every slot fed 1600-sample ticks until it is full.  Then one
Session.event_maps call over the first 8, 64 and 512 slots (--decided): wall time and HIP-event time (two events on the context's
stream around the call) per call, median and p95 over --repeat calls after --warmup.
Baseline, in the same process, for the same rows: Session.events() per slot, the normalisation on the host, and
api.r2qevent_map on --threads (16) host threads -- the route a caller of a decided read had before; it is not the code under test.
The maps of the two routes are compared (they must be the same integers); a difference ends the run with a non-zero status.
The project's condition: a tick of 1600 samples at 4 kHz stands for 0.4 s, and the maps of a tick's decided slots must fit well
inside it.  Lines are stamped with the build id and appended to profiles/session_maps_<build id>/session_maps_latency.log; the
medians and the spread also go to session_maps_latency.json beside it (--no-log: stdout only)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sigfish_amd as S  # noqa: E402
from sigfish_amd import synth  # noqa: E402

LOG = None
TICK_MS = 400.0  # 1600 samples at 4 kHz


def say(msg):
    line = f"[{S.build_id()}] {msg}"
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


class HipEvents:
    """two HIP events on a stream of the library's: device time of what was enqueued between start() and stop()"""

    def __init__(self, stream):
        self.hip = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            if self.hip.hipEventCreate(C.byref(e)) != 0:
                raise RuntimeError("hipEventCreate failed")

    def start(self):
        self.hip.hipEventRecord(self.a, self.stream)

    def stop(self):
        self.hip.hipEventRecord(self.b, self.stream)
        self.hip.hipEventSynchronize(self.b)
        ms = C.c_float(0)
        if self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) != 0:
            raise RuntimeError("hipEventElapsedTime failed")
        return float(ms.value)

    def close(self):
        for e in (self.a, self.b):
            self.hip.hipEventDestroy(e)


def stats(x):
    x = np.asarray(x)
    return dict(median=float(np.median(x)), p95=float(np.percentile(x, 95)), min=float(x.min()), max=float(x.max()))


def main():
    global LOG
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--decided", default="8,64,512", help="decided slots per call, comma separated")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="host threads of the baseline")
    ap.add_argument("--log-dir", default=None, help="directory under profiles/ for the records [session_maps_<build id>]")
    ap.add_argument("--no-log", action="store_true")
    a = ap.parse_args()
    out_dir = None
    if not a.no_log:
        out_dir = os.path.join(ROOT, "profiles", a.log_dir or f"session_maps_{S.build_id()}")
        os.makedirs(out_dir, exist_ok=True)
        LOG = os.path.join(out_dir, "session_maps_latency.log")
    skip, query, chunk, k = 50, 250, 1600, 6
    lv = synth.kmer_levels(k, 1)
    records = S.read_fasta(os.path.join(ROOT, "tests", "golden", "data", "nCoV-2019.reference.fasta"))
    ref = S.RefModel.from_records(records, lv, k, 0, query)
    reads = synth.make_dna_raw_reads(records, lv, k, a.slots, seed=11, samples=(4800, 4800))
    sigs = [r[5] for r in reads]
    scaling = [(r[1], r[2], r[3]) for r in reads]
    n = a.slots
    slots = np.arange(n, dtype=np.int32)
    counts = [min(int(x), n) for x in a.decided.split(",")]
    record = dict(build_id=S.build_id(), slots=n, query=query, skip=skip, chunk_samples=chunk, repeat=a.repeat, warmup=a.warmup, threads=a.threads, tick_ms=TICK_MS, calls={})
    failed = False
    with S.Aligner(ref, 0) as al, al.session(n) as se:
        se.configure_raw(skip, query, query)
        for at in range(0, 4800, chunk):
            rows, info = se.extend_raw(slots, np.concatenate([s[at:at + chunk] for s in sigs]), np.arange(n + 1, dtype=np.int64) * chunk, scaling, [False] * n)
        full = int(((info["status"] & S.RAW_FULL) != 0).sum())
        ok = (rows["valid"] != 0) & (rows["rid"] >= 0)
        say(f"{n} slots x nCoV ({ref.total_columns()} columns), raw DNA session, q = {query}: {full} slots full, {int(ok.sum())} rows mapped; "
            f"band columns per row: median {int(np.median((rows['pos_end'] - rows['pos_st'] + 1)[ok]))}")
        ev = HipEvents(al.stream())
        pool = ThreadPoolExecutor(a.threads)

        def host_one(i, table):
            evn = table.copy()
            evn["mean"][skip:skip + query] = S.znormalise(table["mean"][skip:skip + query])
            j, plus = int(rows[i]["rid"]), rows[i]["strand"] == ord("+")
            try:
                return S.r2qevent_map(rows[i], evn, skip, skip + query, ref.forward[j] if plus else ref.reverse[j], int(ref.st_offset[j]), 0)
            except S.SfaError:
                return None

        for m in counts:
            wall, dev, base = [], [], []
            for rep in range(a.warmup + a.repeat):
                t0 = time.perf_counter()
                ev.start()
                pairs, off, on_host = se.event_maps(rows[:m], slots[:m])
                d = ev.stop()
                w = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                tables = [se.events(int(sl)) for sl in slots[:m]]
                host = list(pool.map(lambda i: host_one(i, tables[i]) if ok[i] else None, range(m)))
                b = (time.perf_counter() - t0) * 1e3
                if rep >= a.warmup:
                    wall.append(w), dev.append(d), base.append(b)
                if rep == 0:
                    bad = 0
                    for i in range(m):
                        got = pairs[off[i]:off[i + 1]]
                        if host[i] is None:
                            bad += len(got) > 0 and not (got == np.iinfo(np.int32).min).all()
                        else:
                            bad += not np.array_equal(got, host[i])
                    failed = failed or bad > 0
                    say(f"decided {m}: maps {'equal the host routine' if bad == 0 else f'DIFFER from the host routine on {bad} rows'}; {int(off[-1])} pairs, {on_host} rows on the host inside the call")
            sw, sd, sb = stats(wall), stats(dev), stats(base)
            record["calls"][str(m)] = dict(wall_ms=sw, hip_event_ms=sd, baseline_wall_ms=sb, pairs=int(off[-1]))
            say(f"decided {m}: Session.event_maps wall {sw['median']:.3f} ms (p95 {sw['p95']:.3f}, min {sw['min']:.3f}, max {sw['max']:.3f}), HIP events {sd['median']:.3f} ms (p95 {sd['p95']:.3f}); "
                f"baseline (events() per slot + normalise + r2qevent_map on {a.threads} threads) wall {sb['median']:.3f} ms (p95 {sb['p95']:.3f}); "
                f"{sw['median'] / TICK_MS * 100:.2f} % of a {TICK_MS:.0f} ms tick against {sb['median'] / TICK_MS * 100:.2f} %")
        pool.shutdown()
        ev.close()
    if out_dir:
        with open(os.path.join(out_dir, "session_maps_latency.json"), "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    if failed:
        sys.exit("maps differ: the times above are of maps that are not the expected ones")


if __name__ == "__main__":
    main()
