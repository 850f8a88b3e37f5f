#!/usr/bin/env python3
"""`sigfish-amd realtime` on a generated flow cell's worth of reads: the time a tick takes against the signal time it stands for.

Generates --reads (20 000) synthetic R9 DNA reads of 2 000 .. 9 000 samples that follow the nCoV reference (synth.make_dna_raw_reads,
seeded k-mer model), writes them as an uncompressed BLOW5 file into --workdir, and replays it with --channels (512) channels and
--chunk-samples (1600, 0.4 s of a 4 kHz channel) twice:
  defaults   normalisation over the whole query (-q 250), never early: dtw's lines, one read decided per 300 events
  early      -q 1000 --norm-events 100 --min-events 100 --min-mapq 20: a read is decided as soon as 100 query events map with mapq 20
Every run is its own process under its own `timeout -k 10`; the driver stops at the first one that fails.  The report each run
prints on stderr (reads, lines by reason, samples sent, per-tick wall time: mean, median, 99th percentile, maximum, ticks beyond the
tick's signal time) is stored as profiles/realtime_<build id>/<name>.log, the PAF next to the BLOW5 file.  The condition to read it
against: the 99th percentile of the tick time must stay under chunk-samples / sampling rate ("Replaying a file in real
time").
With --rna the reads are direct RNA instead (they follow the forward strand of the RNA sequin reference backwards, dwell 10 .. 24
samples per k-mer for the RNA detector's longer windows) and there is one run, through a resweep session:
  rna_resweep  --rna --resweep --norm-events 25 --recalibrate double: calibrated on 25 events, swept again at 50, 100, 200 and 250
Its log goes to profiles/realtime_resweep_<build id>/."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sigfish_amd as S  # noqa: E402
from sigfish_amd import synth  # noqa: E402

BIN = os.path.join(ROOT, "sigfish_amd", "bin", "sigfish-amd")
FASTA = os.path.join(ROOT, "tests", "golden", "data", "nCoV-2019.reference.fasta")
RUNS = (("defaults", []), ("early", ["-q", "1000", "--norm-events", "100", "--min-events", "100", "--min-mapq", "20"]))
RNA_FASTA = os.path.join(ROOT, "tests", "golden", "data", "rnasequin_sequences_2.4.fa")
RNA_RUNS = (("rna_resweep", ["--rna", "--resweep", "--norm-events", "25", "--recalibrate", "double"]),)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--chunk-samples", type=int, default=1600)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per replay")
    ap.add_argument("--workdir", default=None, help="where the BLOW5 file and the PAFs go [a temporary directory]")
    ap.add_argument("--no-log", action="store_true")
    ap.add_argument("--rna", action="store_true", help="direct RNA reads through a resweep session (one run: rna_resweep)")
    a = ap.parse_args()
    work = a.workdir or tempfile.mkdtemp(prefix="realtime_replay_")
    os.makedirs(work, exist_ok=True)
    k = 5 if a.rna else 6
    fasta, runs = (RNA_FASTA, RNA_RUNS) if a.rna else (FASTA, RUNS)
    model = os.path.join(work, f"syn{k}.model")
    with open(model, "w") as f:
        import itertools
        f.write(f"#k\t{k}\nkmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\n")
        for kmer, v in zip(itertools.product("ACGT", repeat=k), synth.kmer_levels(k, 1)):
            f.write("%s\t%.4f\t1.5000\t1.0\t1.0\n" % ("".join(kmer), v))
    levels, _ = S.read_kmer_model(model)
    t0 = time.perf_counter()
    reads = synth.make_dna_raw_reads(S.read_fasta(fasta), levels, k, a.reads, seed=5, **(dict(dwell=(10, 25), rna=True) if a.rna else {}))
    blow5 = os.path.join(work, "reads.blow5")
    synth.write_blow5(blow5, reads)
    n_samples = sum(len(r[5]) for r in reads)
    del reads
    print(f"[{S.build_id()}] {a.reads} reads, {n_samples} samples written to {blow5} in {time.perf_counter() - t0:.1f} s", flush=True)
    logdir = os.path.join(ROOT, "profiles", f"realtime_{'resweep_' if a.rna else ''}{S.build_id()}")
    for name, extra in runs:
        cmd = ["timeout", "-k", "10", str(a.timeout), BIN, "realtime", "--kmer-model", model, "--verbose", "3", "-t", str(a.threads), "--channels", str(a.channels),
               "--chunk-samples", str(a.chunk_samples), *extra, "-o", os.path.join(work, name + ".paf"), fasta, blow5]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True)
        head = f"[{S.build_id()}] {name}: {' '.join(cmd[4:])}\n[{S.build_id()}] exit status {r.returncode} after {time.perf_counter() - t0:.1f} s\n"
        text = head + r.stderr.decode()
        print(text, flush=True)
        if not a.no_log:
            os.makedirs(logdir, exist_ok=True)
            with open(os.path.join(logdir, name + ".log"), "w") as f:
                f.write(text)
        if r.returncode != 0:  # nothing more is started on the device after a run that failed
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
