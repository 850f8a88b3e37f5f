#!/usr/bin/env python3
"""Per-call device time of alignment sessions against re-alignment of the growing prefix.

--slots (512) slots x the nCoV model, chunks of --chunk (50) events up to --events (1 000) per slot, with and without start columns:
after every chunk the device time of Session.extend (sfa_profile_t.total_ms / fill_ms of the call) next to the device time of
align_db on the same prefixes in the same process.  Rows of the two are compared (every field with start columns, every field but
the -1 coordinate without).  Lines are stamped with the build id and appended to profiles/session_<build id>/session_latency.log
(--no-log: stdout only)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sigfish_amd as S  # noqa: E402
from sigfish_amd import synth  # noqa: E402

LOG = None


def say(msg):
    line = f"[{S.build_id()}] {msg}"
    print(line, flush=True)
    if LOG:
        with open(LOG, "a") as f:
            f.write(line + "\n")


def same(got, want, starts):
    if starts:
        return got.tobytes() == want.tobytes()
    plus = want["strand"] == ord("+")
    w = want.copy()
    w["pos_st"][plus] = -1
    w["pos_end"][~plus] = -1
    return got.tobytes() == w.tobytes()


def main():
    global LOG
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--events", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=3, help="runs per configuration; the median per chunk is reported")
    ap.add_argument("--no-log", action="store_true")
    a = ap.parse_args()
    if not a.no_log:
        d = os.path.join(ROOT, "profiles", f"session_{S.build_id()}")
        os.makedirs(d, exist_ok=True)
        LOG = os.path.join(d, "session_latency.log")
    ref, flag, q, q_off, _ = synth.workload(f"ncov_r9_dna_q{a.events}", n_reads=a.slots, seed=11)
    n, slots = a.slots, np.arange(a.slots, dtype=np.int32)
    reads = [q[q_off[i]:q_off[i + 1]] for i in range(n)]
    n_chunks = a.events // a.chunk
    say(f"{n} slots x nCoV ({ref.total_columns()} columns), chunks of {a.chunk} events up to {n_chunks * a.chunk}; "
        f"carried rows {S.session_bytes(ref.total_columns(), n) / 1e6:.0f} MB with starts, {S.session_bytes(ref.total_columns(), n, False) / 1e6:.0f} MB without")
    with S.Aligner(ref, flag) as al:
        batch = np.zeros((a.repeat, n_chunks))
        rows = []
        for rep in range(a.repeat):
            for k in range(n_chunks):
                hi = (k + 1) * a.chunk
                r = al.align_db(np.concatenate([x[:hi] for x in reads]), np.arange(n + 1, dtype=np.int64) * hi)
                batch[rep, k] = al.profile()["total_ms"]
                if rep == 0:
                    rows.append(r)
        ext = {}
        for starts in (True, False):
            t = np.zeros((a.repeat, n_chunks))
            f = np.zeros((a.repeat, n_chunks))
            ok = True
            with al.session(n, starts=starts) as se:
                for rep in range(a.repeat):
                    se.reset()
                    for k in range(n_chunks):
                        lo, hi = k * a.chunk, (k + 1) * a.chunk
                        got = se.extend(slots, np.concatenate([x[lo:hi] for x in reads]), np.arange(n + 1, dtype=np.int64) * a.chunk)
                        p = al.profile()
                        t[rep, k], f[rep, k] = p["total_ms"], p["fill_ms"]
                        ok = ok and same(got, rows[k], starts)
            ext[starts] = (np.median(t, 0), np.median(f, 0), ok)
            say(f"session starts={starts}: rows {'equal' if ok else 'DIFFER from'} align_db's on every prefix")
        b = np.median(batch, 0)
        say("chunk  prefix  align_db_ms  extend_ms(starts)  sweeps_ms  extend_ms(no_start)  sweeps_ms")
        for k in range(n_chunks):
            say(f"{k + 1:5d}  {(k + 1) * a.chunk:6d}  {b[k]:11.3f}  {ext[True][0][k]:17.3f}  {ext[True][1][k]:9.3f}  {ext[False][0][k]:19.3f}  {ext[False][1][k]:9.3f}")
        for starts in (True, False):
            t = ext[starts][0]
            first = next((k + 1 for k in range(n_chunks) if t[k] < b[k]), None)
            say(f"starts={starts}: extend is below align_db from chunk {first}; extend of chunk 2 / last chunk {t[1]:.3f} / {t[-1]:.3f} ms; "
                f"sum over the read {t.sum():.1f} ms against {b.sum():.1f} ms of re-alignment")


if __name__ == "__main__":
    main()
