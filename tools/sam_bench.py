#!/usr/bin/env python3
"""What --sam costs, and what the event maps from the device (sfa_event_maps) change about it.

  cli   `sigfish-amd dtw --sam --device-paths` (maps from the device), `--sam --host-paths` (warp paths rebuilt read by read on the -t threads) and
        plain PAF on one generated file: the DNA fixture's reads replicated to --reads reads (default 100 000), -q 250, compressed;
        reads/s of each, SAM of the two routes compared byte for byte.  --rocprof: one more --sam --device-paths run under
        `rocprofv3 --kernel-trace --stats`, its kernel summary copied next to the log.
  lib   the library call alone: align_db on --reads synthetic R9 reads x nCoV (-q 250), then sfa_event_maps of the primaries against
        sfa_r2qevent_map per row over --threads host threads on the same rows; maps compared.

Both print lines stamped with the build id and append them to profiles/event_maps_<build id>/sam_bench.log (--no-log: stdout only)."""
import argparse
import ctypes as C
import filecmp
import glob
import itertools
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sigfish_amd as S  # noqa: E402
from sigfish_amd import _lib, synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
LOG = None


def say(msg):
    line = f"[{S.build_id()}] {msg}"
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


def cli(a):
    d = a.dir or tempfile.mkdtemp(prefix="sam_bench_")  # (a memory-backed directory keeps the disk out of the timing)
    os.makedirs(d, exist_ok=True)
    model = os.path.join(d, "syn6.model")
    lv = np.fromfile(os.path.join(GOLD, "models", "syn6.f32"), np.float32)
    with open(model, "w") as f:
        f.write("#k\t6\nkmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\n")
        for kmer, v in zip(itertools.product("ACGT", repeat=6), lv):
            f.write("%s\t%.4f\t1.5000\t1.0\t1.0\n" % ("".join(kmer), v))
    src = os.path.join(GOLD, "data", "sp1_dna.blow5")
    fasta = os.path.join(GOLD, "data", "nCoV-2019.reference.fasta")
    n_src = sum(1 for _ in S.Blow5File(src))
    copies = max(1, a.reads // n_src)
    big = os.path.join(d, "sam_bench.blow5")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_blow5.py"), src, big, "--copies", str(copies), "--compress", "--jobs",
                    str(a.threads)], check=True, capture_output=True)
    n = copies * n_src
    say(f"cli: {n} reads, {os.path.getsize(big) / 1e6:.0f} MB (zlib + svb-zd), -q 250 -t {a.threads}, {a.reps} runs each, alternating")
    binp = os.path.join(ROOT, "sigfish_amd", "bin", "sigfish-amd")
    base = [binp, "dtw", "--kmer-model", model, "-q", "250", "-t", str(a.threads), "--verbose", "0"]
    legs = {"sam --device-paths": ["--sam", "--device-paths"], "sam --host-paths": ["--sam", "--host-paths"], "paf": []}
    rates = {k: [] for k in legs}
    outs = {}
    for rep in range(a.reps):
        for name, extra in legs.items():
            out = os.path.join(d, "out_" + name.replace(" ", "_").replace("-", ""))
            t0 = time.perf_counter()
            with open(out, "w") as fo:
                r = subprocess.run(base + extra + [fasta, big], stdout=fo, stderr=subprocess.PIPE, timeout=a.timeout)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise SystemExit(f"{name}: exit {r.returncode}\n{r.stderr.decode()[-2000:]}")
            rates[name].append(n / wall)
            outs[name] = out
    for name, v in rates.items():
        say(f"cli {name:>19}: " + " ".join(f"{x:,.0f}" for x in v) + f" reads/s (median {np.median(v):,.0f})")
    same = filecmp.cmp(outs["sam --device-paths"], outs["sam --host-paths"], shallow=False)
    say(f"cli: SAM from the device maps {'==' if same else '!='} SAM from host paths ({os.path.getsize(outs['sam --device-paths'])} bytes)")
    if a.rocprof and shutil.which("rocprofv3"):
        pd = os.path.join(d, "rocprof")
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", pd, "-o", "sam", "--"] + base + ["--sam", "--device-paths", fasta, big],
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=a.timeout, check=True)
        for p in glob.glob(os.path.join(pd, "**", "*kernel_stats.csv"), recursive=True):
            if LOG:
                shutil.copy(p, os.path.join(os.path.dirname(LOG), "cli_sam_kernel_stats.csv"))
            with open(p) as f:
                for ln in f.read().splitlines()[:12]:
                    say("    " + ln)
        shutil.rmtree(pd, ignore_errors=True)
    for p in (big, model, *outs.values()):
        os.remove(p)
    if not a.dir:
        os.rmdir(d)
    if not same:
        raise SystemExit(1)


def lib(a):
    ref, flag, q, q_off, _ = synth.workload("ncov_r9_dna_q250", n_reads=a.reads, seed=5)
    L = _lib.load()
    with S.Aligner(ref, flag, device=0) as al:
        rows = al.align_db(q, q_off)
        size = np.where(rows["valid"] == 1, rows["pos_end"].astype(np.int64) - rows["pos_st"] + 1, 0)
        off = np.concatenate([[0], np.cumsum(size)]).astype(np.int64)
        pairs = np.zeros((int(off[-1]) + 1, 2), np.int32)
        on_host = C.c_int32(0)

        def device():
            rc = L.sfa_event_maps(al._h, rows.ctypes.data_as(C.c_void_p), None, len(rows), off.ctypes.data_as(_lib.i64p),
                                  pairs.ctypes.data_as(_lib.i32p), C.byref(on_host))
            assert rc == 0, L.sfa_last_error()

        device()  # warm-up (allocations)
        t_dev = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            device()
            t_dev.append(time.perf_counter() - t0)
    # the same rows through the per-read host routine on --threads threads (ctypes releases the GIL inside the call)
    host = np.zeros_like(pairs)
    evs = np.zeros(int(q_off[-1]), S.EVENT_DTYPE)
    evs["mean"] = q
    evp = C.cast(evs.ctypes.data, C.POINTER(_lib.SfaEvent))
    hp_base = host.ctypes.data
    rp = C.cast(rows.ctypes.data, C.POINTER(_lib.SfaResult))
    arrs = [(np.ascontiguousarray(f, np.float32), np.ascontiguousarray(r, np.float32)) for f, r in zip(ref.forward, ref.reverse)]

    def chunk(lo, hi):
        for i in range(lo, hi):
            if not size[i]:
                continue
            y = arrs[int(rows["rid"][i])][0 if rows["strand"][i] == ord("+") else 1]
            L.sfa_r2qevent_map(C.byref(rp[i]), evp, int(q_off[i]), int(q_off[i + 1]), y.ctypes.data_as(_lib.f32p), len(y),
                               int(ref.st_offset[int(rows["rid"][i])]), flag, C.cast(hp_base + 8 * int(off[i]), _lib.i32p), int(size[i]))

    t_host = []
    step = max(1, len(rows) // (a.threads * 8))
    with ThreadPoolExecutor(a.threads) as ex:
        for _ in range(a.reps):
            t0 = time.perf_counter()
            list(ex.map(lambda lo: chunk(lo, min(lo + step, len(rows))), range(0, len(rows), step)))
            t_host.append(time.perf_counter() - t0)
    same = np.array_equal(pairs[:int(off[-1])], host[:int(off[-1])])
    say(f"lib: {len(rows)} rows, {int(off[-1])} map columns, rows on the host inside sfa_event_maps: {on_host.value}")
    say("lib sfa_event_maps: " + " ".join(f"{t * 1e3:.1f}" for t in t_dev) + f" ms per call (median {len(rows) / np.median(t_dev):,.0f} rows/s)")
    say(f"lib sfa_r2qevent_map x {a.threads} threads (Python driver): " + " ".join(f"{t * 1e3:.1f}" for t in t_host) +
        f" ms (median {len(rows) / np.median(t_host):,.0f} rows/s)")
    say(f"lib: maps {'==' if same else '!='}")
    if not same:
        raise SystemExit(1)


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["lib", "cli"])
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--timeout", type=int, default=1200)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--no-log", action="store_true")
    ap.add_argument("--log-dir", default=None)
    a = ap.parse_args()
    if not a.no_log:
        d = a.log_dir or os.path.join(ROOT, "profiles", f"event_maps_{S.build_id()}")
        os.makedirs(d, exist_ok=True)
        LOG = os.path.join(d, "sam_bench.log")
    (lib if a.what == "lib" else cli)(a)


if __name__ == "__main__":
    main()
