#!/usr/bin/env python3
"""Wall time per call of a raw session with the automatic query start (sfa_session_raw_auto_start), on the GPU.

512 slots over the RNA sequin reference, synthetic direct-RNA reads (synth.make_rna_polya_reads), one chunk of 1600 samples per
busy slot per call; a slot whose read has ended is reset and takes the next read.  Per call: the wall time of extend_raw, the
device time of the feature's own kernels (Session.auto_ms: retention and evaluation) and of detector, normaliser and sweep
(Aligner.profile).  Three runs on the same samples:
  auto      the session with the feature (a point every --every samples, the final point at the end or at --max-samples)
  off       the same session without it, skip 50: what the feature adds is auto - off
  baseline  what a caller can do today: at every call Aligner.align_raw(prefix_size=-1) over the WHOLE prefix of every busy slot
            (--baseline-calls of them, it is slow)
The workload's own condition: a call takes less than the 1600 / 3000 Hz = 0.533 s of signal it consumes.  Writes a log under
profiles/session_autostart_<build id>/ and prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sigfish_amd as S  # noqa: E402
from sigfish_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=1600)
    ap.add_argument("--every", type=int, default=1600)
    ap.add_argument("--max-samples", type=int, default=65536)
    ap.add_argument("--max-skip", type=int, default=4096)
    ap.add_argument("--query", type=int, default=250)
    ap.add_argument("--norm", type=int, default=25)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--baseline-calls", type=int, default=12)
    ap.add_argument("--reads", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    gd = os.path.join(ROOT, "tests", "golden")
    levels = synth.kmer_levels(5, 2, 100.0, 14.0)
    ref = S.RefModel.from_fasta(os.path.join(gd, "data", "rnasequin_sequences_2.4.fa"), levels, 5, S.RNA, a.query)
    reads = synth.make_rna_polya_reads(a.reads, seed=a.seed, kinds=["normal", "normal", "normal", "adaptor_edge", "polya_edge", "no_polya", "no_adaptor"])
    at = tuple(S.recal_double(a.norm, a.query))
    out = {"build_id": S.build_id(), "slots": a.slots, "chunk": a.chunk, "every": a.every, "max_samples": a.max_samples, "budget_ms": 1000.0 * a.chunk / 3000.0}
    log = []

    def drive(al, se, n_calls, baseline=False):
        on, pos, nxt = list(range(a.slots)), [0] * a.slots, a.slots
        wall, auto_ms, dev_ms = [], [], []
        for call in range(n_calls):
            chunks = [reads[on[s]][5][pos[s]:pos[s] + a.chunk] for s in range(a.slots)]
            ends = [len(c) < a.chunk for c in chunks]
            off = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.int64)
            raw = np.concatenate(chunks)
            scal = [reads[on[s]][1:4] for s in range(a.slots)]
            t0 = time.perf_counter()
            if baseline:
                pre = [reads[on[s]][5][:pos[s] + len(chunks[s])] for s in range(a.slots)]
                poff = np.concatenate([[0], np.cumsum([len(p) for p in pre])]).astype(np.int64)
                al.align_raw(np.concatenate(pre), poff, np.array(scal, np.float64), -1, a.query)
            else:
                se.extend_raw(list(range(a.slots)), raw, off, scal, ends)
            wall.append(1000.0 * (time.perf_counter() - t0))
            if not baseline:
                pr = al.profile()
                dev_ms.append(pr["total_ms"])
                auto_ms.append(max(se.auto_ms(), 0.0))
            done = [s for s in range(a.slots) if ends[s]]
            for s in range(a.slots):
                pos[s] += len(chunks[s])
            if done and not baseline:
                se.reset(done)
            for s in done:
                on[s], pos[s], nxt = nxt % len(reads), 0, nxt + 1
        return wall, auto_ms, dev_ms

    def stats(x):
        x = np.asarray(x[2:] if len(x) > 4 else x)  # (the first calls allocate)
        return {"median": float(np.median(x)), "p95": float(np.percentile(x, 95)), "max": float(x.max())} if len(x) else {}

    with S.Aligner(ref, S.RNA) as al:
        with al.session(a.slots, resweep=True, auto_start=dict(skip=a.max_skip, norm=a.norm, query=a.query, recalibrate=at, at_end=True, every=a.every,
                                                                max_samples=a.max_samples)) as se:
            w, au, dv = drive(al, se, a.calls)
            out["auto"] = {"wall_ms": stats(w), "auto_kernels_ms": stats(au), "device_ms": stats(dv)}
            log += [f"auto call {i} wall {x:.3f} ms auto-kernels {y:.3f} ms device {z:.3f} ms" for i, (x, y, z) in enumerate(zip(w, au, dv))]
        with al.session(a.slots, resweep=True) as se:
            se.configure_raw(50, a.norm, a.query, recalibrate=at, at_end=True)
            w, _, dv = drive(al, se, a.calls)
            out["off"] = {"wall_ms": stats(w), "device_ms": stats(dv)}
            log += [f"off call {i} wall {x:.3f} ms device {z:.3f} ms" for i, (x, z) in enumerate(zip(w, dv))]
        w, _, _ = drive(al, None, a.baseline_calls, baseline=True)
        out["baseline_align_raw_whole_prefix"] = {"wall_ms": stats(w), "calls": a.baseline_calls}
        log += [f"baseline call {i} wall {x:.3f} ms" for i, x in enumerate(w)]
    out["added_wall_ms_median"] = out["auto"]["wall_ms"]["median"] - out["off"]["wall_ms"]["median"]
    out["meets_budget"] = out["auto"]["wall_ms"]["p95"] < out["budget_ms"]
    d = os.path.join(ROOT, "profiles", f"session_autostart_{S.build_id()}")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "latency.log"), "w") as f:
        f.write("\n".join(log) + "\n" + json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
