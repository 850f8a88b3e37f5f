#!/usr/bin/env python3
"""Cost of secondary mappings (option "secondary"): align_db with the option at 0 against 4, alternating, on

  ncov    100 000 synthetic R9 DNA reads x nCoV-2019, -q 250 (the headline workload)
  rna1k   8 192 synthetic R9 RNA reads x the sequin transcriptome, -q 1000

one context, device-event stage timers of every call (fill = pass 1, trace = pass 2 of the primaries, finalize = everything after:
the merge, the pass-2 launches of the secondaries and the row kernels).  Primaries are checked to be equal in both settings.  For the
per-kernel table run it once more under `rocprofv3 --kernel-trace --stats -- python tools/secondary_bench.py`.

    python tools/secondary_bench.py [--rounds 3] [--out DIR]   (log: DIR/secondary.log, default profiles/secondary_<build id>/)
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

GOLD = os.path.join(ROOT, "tests", "golden")


def workloads():
    ref, flag, q, q_off, _ = synth.workload("ncov_r9_dna_q250", n_reads=100_000, seed=3)
    yield "ncov_q250_100k", ref, flag, q, q_off
    lv = synth.kmer_levels(5, 2, 100.0, 14.0)
    ref = S.RefModel.from_fasta(os.path.join(GOLD, "data", "rnasequin_sequences_2.4.fa"), lv, 5, S.RNA, 1000)
    q, q_off, _ = synth.make_reads(ref, 8192, qlen=1000, seed=4)
    yield "rna_q1000_8k", ref, S.RNA, q, q_off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "profiles", f"secondary_{S.build_id()}")
    os.makedirs(out, exist_ok=True)
    log = open(os.path.join(out, "secondary.log"), "a")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")

    say(f"# build {S.build_id()}  {time.strftime('%Y-%m-%d %H:%M:%S')}")
    for name, ref, flag, q, q_off in workloads():
        with S.Aligner(ref, flag) as al:
            al.align_db(q, q_off)  # warm-up of both routes
            al.set_secondary(4)
            al.align_db(q, q_off)
            prim = {}
            for r in range(a.rounds):
                for n_sec in (0, 4):
                    al.set_secondary(n_sec)
                    t0 = time.perf_counter()
                    rows = al.align_db(q, q_off)
                    wall = (time.perf_counter() - t0) * 1e3
                    p = al.profile()
                    n_valid = int(al.secondary_rows()["valid"].sum()) if n_sec else 0
                    if n_sec in prim:
                        assert rows.tobytes() == prim[n_sec]
                    prim[n_sec] = rows.tobytes()
                    say(f"{name} round {r} secondary {n_sec}: wall {wall:.2f} ms  total {p['total_ms']:.2f}  fill {p['fill_ms']:.2f}  "
                        f"trace {p['trace_ms']:.2f}  finalize {p['finalize_ms']:.2f}  lds_ckpt {p['lds_ckpt']}  fused {p['fused_trace']}  "
                        f"secondary rows {n_valid}")
            assert prim[0] == prim[4], "primaries differ with the option"
            say(f"{name}: primaries identical with secondary 0 and 4")


if __name__ == "__main__":
    main()
