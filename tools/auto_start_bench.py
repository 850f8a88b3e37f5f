#!/usr/bin/env python3
"""The RNA automatic query start (-p -1) on the device, measured two ways:

  lib   sfa_align_raw on synthetic RNA reads (synth.make_rna_polya_reads, 20-50 k samples) with -p -1 and with -p 50, -q 500,
        one context; device-event stage timers of the call (events_ms holds the ev_autostart_* kernels).  Run it once more
        under `rocprofv3 --kernel-trace --stats -- python tools/auto_start_bench.py lib` for the per-kernel table.
  cli   the command line `dtw --rna -q 500 -p -1 -t T` on a generated file (zlib + svb-zd records), default route (events,
        adaptor and poly-A search on the GPU) against --host-events; reads/s of both, and whether the two PAFs are identical.

    python tools/auto_start_bench.py lib [--reads 32768]
    python tools/auto_start_bench.py cli [--reads 100000] [--threads 16] [--dir DIR (scratch files; default: a new temporary directory)]
Prints one line per measurement, prefixed with the library's build id."""
import argparse
import filecmp
import itertools
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sigfish_amd as S  # noqa: E402
from sigfish_amd import synth  # noqa: E402
from tests.util import write_blow5  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
FASTA = os.path.join(GOLD, "data", "rnasequin_sequences_2.4.fa")


def unique_reads(n, seed, body):
    """n distinct normal-shaped reads (adaptor, tail, body; plus the generator's fallback kinds at their usual share)"""
    return synth.make_rna_polya_reads(n, seed=seed, pore=0, body=body)


def lib(a):
    uniq = unique_reads(4096, 1, (12_000, 42_000))  # leader + adaptor + tail + body: 20-50 k samples
    pick = [uniq[i % len(uniq)] for i in range(a.reads)]
    raw = np.concatenate([r[5] for r in pick])
    off = np.concatenate([[0], np.cumsum([len(r[5]) for r in pick])]).astype(np.int64)
    sc = np.array([[r[1], r[2], r[3]] for r in pick], np.float64)
    lv = np.fromfile(os.path.join(GOLD, "models", "syn5.f32"), np.float32)
    ref = S.RefModel.from_fasta(FASTA, lv, 5, S.RNA, 500)
    lens = np.diff(off)
    print(f"[{S.build_id()}] lib: {a.reads} reads, {lens.min()}..{lens.max()} samples (mean {lens.mean():.0f}), {raw.size / 1e9:.2f} G samples")
    with S.Aligner(ref, S.RNA, device=0) as al:
        for prefix in (-1, 50):
            rows, info = al.align_raw(raw, off, sc, prefix, 500)  # warm-up (allocations)
            ev = nm = tot = 0.0
            t0 = time.perf_counter()
            for _ in range(a.reps):
                rows, info = al.align_raw(raw, off, sc, prefix, 500)
                p = al.profile()
                ev += p["events_ms"]
                nm += p["normalise_ms"]
                tot += p["total_ms"]
            wall = (time.perf_counter() - t0) / a.reps
            fb = int(((info["status"] & 4) != 0).sum())
            print(f"[{S.build_id()}] lib -p {prefix:>2} -q 500: events (incl. auto start) {ev / a.reps:.2f} ms, normalise {nm / a.reps:.2f} ms, "
                  f"alignment {tot / a.reps:.2f} ms, call {wall * 1e3:.1f} ms wall; prefix fail {fb}, kept {int((rows['valid'] == 1).sum())}")


def cli(a):
    d = a.dir or tempfile.mkdtemp(prefix="auto_start_bench_")  # (a memory-backed directory keeps the disk out of the timing)
    os.makedirs(d, exist_ok=True)
    model = os.path.join(d, "syn5.model")
    lv = np.fromfile(os.path.join(GOLD, "models", "syn5.f32"), np.float32)
    with open(model, "w") as f:
        f.write("#k\t5\nkmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\n")
        for kmer, v in zip(itertools.product("ACGT", repeat=5), lv):
            f.write("%s\t%.4f\t1.5000\t1.0\t1.0\n" % ("".join(kmer), v))
    src = os.path.join(d, "pauto_src.blow5")
    big = os.path.join(d, "pauto_big.blow5")
    uniq = unique_reads(1000, 2, (5_000, 15_000))
    write_blow5(src, uniq, attrs=(("experiment_type", "rna"), ("sequencing_kit", "unknown")))
    copies = max(1, a.reads // len(uniq))
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_blow5.py"), src, big, "--copies", str(copies), "--compress", "--jobs",
                    str(a.threads)], check=True, capture_output=True)
    n = copies * len(uniq)
    samples = sum(len(r[5]) for r in uniq) * copies
    print(f"[{S.build_id()}] cli: {n} reads, {samples / 1e9:.2f} G samples, {os.path.getsize(big) / 1e6:.0f} MB (zlib + svb-zd)")
    binp = os.path.join(ROOT, "sigfish_amd", "bin", "sigfish-amd")
    outs = {}
    for name, extra in (("device", []), ("host-events", ["--host-events"])):
        out = os.path.join(d, f"pauto_{name}.paf")
        cmd = [binp, "dtw", "--kmer-model", model, "--rna", "-q", "500", "-p", "-1", "-t", str(a.threads), "--verbose", "3", *extra, FASTA, big]
        t0 = time.perf_counter()
        with open(out, "w") as fo:
            r = subprocess.run(cmd, stdout=fo, stderr=subprocess.PIPE, timeout=a.timeout)
        wall = time.perf_counter() - t0
        if r.returncode != 0:
            print(r.stderr.decode()[-2000:])
            raise SystemExit(f"{name}: exit {r.returncode}")
        summary = [ln for ln in r.stderr.decode().splitlines() if "total entries" in ln or "time" in ln]
        print(f"[{S.build_id()}] cli {name:>11}: {wall:.1f} s wall, {n / wall:,.0f} reads/s")
        for ln in summary:
            print(f"    {ln}")
        outs[name] = out
    same = filecmp.cmp(outs["device"], outs["host-events"], shallow=False)
    print(f"[{S.build_id()}] cli: PAF device route {'==' if same else '!='} host route ({os.path.getsize(outs['device'])} bytes)")
    for p in (src, big, model, *outs.values()):
        os.remove(p)
    if not a.dir:
        os.rmdir(d)
    if not same:
        raise SystemExit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["lib", "cli"])
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--timeout", type=int, default=1200)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    if a.what == "lib":
        a.reads = a.reads or 32768
        lib(a)
    else:
        a.reads = a.reads or 100_000
        cli(a)


if __name__ == "__main__":
    main()
