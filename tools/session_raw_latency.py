#!/usr/bin/env python3
"""Per-call time of raw-signal sessions against the route without them.

--slots (512) slots x the nCoV model, synthetic signals (levels ~N(90, 12) pA, dwell 6..12 samples, noise sd 1.5), chunks of --chunk
(1600) samples -- 0.4 s of a 4 kHz channel -- for --calls (8) calls.  Per call: wall time of Session.extend_raw and its device split
(sfa_profile_t events_ms / normalise_ms / fill_ms).  Beside it the baseline, the only route without raw mode: sfa_detect_events over
every slot's WHOLE PREFIX on --threads (16) host threads, the tail events dropped, normalisation on the host, Session.extend.  The
workload's own condition is printed: a call must take less than the --chunk / 4000 s of signal it consumes.  Lines are stamped with
the build id and appended to profiles/session_raw_<build id>/session_raw_latency.log (--no-log: stdout only)."""
import argparse
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
META = dict(digitisation=8192.0, offset=6.0, range=1467.61)


def say(msg):
    line = f"[{S.build_id()}] {msg}"
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


def signal(rng, n):
    n_lv = n // 6 + 2
    pa = np.repeat(rng.normal(90, 12, n_lv), rng.integers(6, 13, n_lv))[:n] + rng.normal(0, 1.5, n)
    return np.round(pa * META["digitisation"] / META["range"] - META["offset"]).astype(np.int16)


def main():
    global LOG
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=1600)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--skip", type=int, default=50)
    ap.add_argument("--norm", type=int, default=100)
    ap.add_argument("--query", type=int, default=2048)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-log", action="store_true")
    a = ap.parse_args()
    if not a.no_log:
        d = os.path.join(ROOT, "profiles", f"session_raw_{S.build_id()}")
        os.makedirs(d, exist_ok=True)
        LOG = os.path.join(d, "session_raw_latency.log")
    ref, flag, _, _, _ = synth.workload("ncov_r9_dna_q250", n_reads=1, seed=11)
    rng = np.random.default_rng(11)
    n, slots = a.slots, np.arange(a.slots, dtype=np.int32)
    sigs = [signal(rng, a.chunk * a.calls) for _ in range(n)]
    scaling = [(META["digitisation"], META["offset"], META["range"])] * n
    raw_off = np.arange(n + 1, dtype=np.int64) * a.chunk
    budget_ms = a.chunk / 4000.0 * 1e3
    say(f"{n} slots x nCoV ({ref.total_columns()} columns), {a.calls} calls of {a.chunk} samples per slot, skip {a.skip} norm {a.norm} query {a.query}; "
        f"raw mode adds {S.session_raw_bytes(n, a.skip, a.query) / 1e6:.1f} MB to {S.session_bytes(ref.total_columns(), n) / 1e6:.0f} MB of carried rows")
    with S.Aligner(ref, flag) as al:
        with al.session(n) as se:
            se.configure_raw(a.skip, a.norm, a.query)
            say("raw session:  call  wall_ms  events_ms  normalise_ms  fill_ms  total_ms  calibrated  q_events")
            worst = 0.0
            for k in range(a.calls):
                chunk = np.concatenate([s[k * a.chunk:(k + 1) * a.chunk] for s in sigs])
                t0 = time.perf_counter()
                rows, info = se.extend_raw(slots, chunk, raw_off, scaling)
                wall = (time.perf_counter() - t0) * 1e3
                p = al.profile()
                worst = max(worst, wall)
                say(f"              {k + 1:4d}  {wall:7.2f}  {p['events_ms']:9.3f}  {p['normalise_ms']:12.3f}  {p['fill_ms']:7.3f}  {p['total_ms']:8.3f}  "
                    f"{int((info['status'] & S.RAW_CALIBRATED != 0).sum()):10d}  {int(info['q_events'].sum()):8d}")
            say(f"a call consumes {budget_ms:.0f} ms of signal per slot; the slowest call took {worst:.2f} ms: "
                f"{'keeps up' if worst < budget_ms else 'DOES NOT keep up'} with {n} channels")
        # the baseline: the host detector over the whole prefix again for every chunk, then Session.extend
        rna = bool(flag & S.RNA)
        w_long = 14 if rna else 6
        with al.session(n) as se, ThreadPoolExecutor(a.threads) as pool:
            say("host detector + extend:  call  wall_ms  detect_ms  extend_ms  new_events")
            sent = [0] * n
            stats = [None] * n
            for k in range(a.calls):
                hi = (k + 1) * a.chunk
                t0 = time.perf_counter()
                tables = list(pool.map(lambda s: S.detect_events(s[:hi], META, rna), sigs))
                t1 = time.perf_counter()
                chunks = []
                for i, ev in enumerate(tables):
                    # stable: the events that end at least two long windows in front of the last sample (the batch detector cannot
                    # tell which of its tail events are final), cut at skip + query
                    stable = min(int(np.searchsorted(ev["start"], hi - 2 * w_long, side="right")) - 1, a.skip + a.query)
                    m = ev["mean"][:max(stable, 0)]
                    if stats[i] is None and len(m) >= a.skip + a.norm:
                        w = m[a.skip:a.skip + a.norm]  # sfa_znormalise's sums: sequential fp32 (cumsum adds in order)
                        cnt = np.float32(len(w))
                        mean = np.float32(np.cumsum(w, dtype=np.float32)[-1] / cnt)
                        dv = (w - mean).astype(np.float32)
                        var = np.float32(np.cumsum(dv * dv, dtype=np.float32)[-1] / cnt)
                        stats[i] = (mean, np.float32(np.sqrt(np.float64(var))))
                    if stats[i] is None:
                        chunks.append(np.zeros(0, np.float32))
                        continue
                    q = ((m[a.skip:] - stats[i][0]) / stats[i][1]).astype(np.float32)
                    chunks.append(q[sent[i]:])
                    sent[i] = len(q)
                ev_off = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.int64)
                t2 = time.perf_counter()
                rows = se.extend(slots, np.concatenate(chunks), ev_off)
                t3 = time.perf_counter()
                del rows  # (a timing baseline: its tail rule is by position, so its queries trail raw mode's by an event or two)
                say(f"                         {k + 1:4d}  {(t3 - t0) * 1e3:7.2f}  {(t1 - t0) * 1e3:9.2f}  {(t3 - t2) * 1e3:9.2f}  {int(ev_off[-1]):6d}")


if __name__ == "__main__":
    main()
