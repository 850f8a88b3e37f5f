#!/usr/bin/env python3
"""Per-call device time of alignment sessions against re-alignment of the growing prefix.

--slots (512) slots x the nCoV model, chunks of --chunk (50) events up to --events (1 000) per slot, with and without start columns:
after every chunk the device time of Session.extend (sfa_profile_t.total_ms / fill_ms of the call) next to the device time of
align_db on the same prefixes in the same process.  Rows of the two are compared (every field with start columns, every field but
the -1 coordinate without); a difference is reported by field and ends the run with a non-zero status.  --candidates N (1..4) adds a leg per kind of session with N candidates kept
(Session.configure_candidates): its rows are compared with the leg without as well (they must be the same bytes), and its time is reported against the leg without, per chunk.
Lines are stamped with the build id and appended to profiles/session_<build id>/session_latency.log
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


def differing(got, want, starts):
    """the fields in which rows differ, with the number of rows each: {} when they are the same bytes (without start columns the
    coordinate that needs one is -1 in `got`)"""
    w = want.copy()
    if not starts:
        plus = w["strand"] == ord("+")
        w["pos_st"][plus & (w["valid"] == 1)] = -1
        w["pos_end"][~plus & (w["valid"] == 1)] = -1
    if got.tobytes() == w.tobytes():
        return {}
    return {f: int((got[f].view(np.uint32) != w[f].view(np.uint32)).sum() if f in ("score", "score2") else (got[f] != w[f]).sum())
            for f in got.dtype.names if got[f].tobytes() != w[f].tobytes()}


def verdict(diffs, what):
    """one line per comparison: equal, or the first prefix that differs with its fields and row counts"""
    bad = [(k, d) for k, d in enumerate(diffs) if d]
    if not bad:
        return f"rows equal {what} on every prefix"
    k, d = bad[0]
    return f"rows DIFFER from {what} on {len(bad)} of {len(diffs)} prefixes; first at chunk {k + 1}: rows per field {d}"


def main():
    global LOG
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--chunk", type=int, default=50)
    ap.add_argument("--events", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=3, help="runs per configuration; the median per chunk is reported")
    ap.add_argument("--candidates", type=int, default=0, help="1..4: a leg with that many session candidates kept, against the leg without")
    ap.add_argument("--log-dir", default=None, help="directory under profiles/ for the log [session_<build id>]")
    ap.add_argument("--no-log", action="store_true")
    a = ap.parse_args()
    if not a.no_log:
        d = os.path.join(ROOT, "profiles", a.log_dir or f"session_{S.build_id()}")
        os.makedirs(d, exist_ok=True)
        LOG = os.path.join(d, "session_latency.log")
    ref, flag, q, q_off, _ = synth.workload(f"ncov_r9_dna_q{a.events}", n_reads=a.slots, seed=11)
    n, slots = a.slots, np.arange(a.slots, dtype=np.int32)
    reads = [q[q_off[i]:q_off[i + 1]] for i in range(n)]
    n_chunks = a.events // a.chunk
    # the workload's reads are ragged (a read drawn near the end of a contig is shorter than --events): a slot whose read has run
    # out sends empty chunks, and every offset comes from the lengths that are really there
    short = sum(len(x) < n_chunks * a.chunk for x in reads)

    def packed(parts):
        return (np.concatenate(parts) if sum(len(x) for x in parts) else np.zeros(0, np.float32),
                np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64))
    say(f"{n} slots x nCoV ({ref.total_columns()} columns), chunks of {a.chunk} events up to {n_chunks * a.chunk} ({short} reads are shorter: {sum(len(x) for x in reads)} events in all); "
        f"carried rows {S.session_bytes(ref.total_columns(), n) / 1e6:.0f} MB with starts, {S.session_bytes(ref.total_columns(), n, False) / 1e6:.0f} MB without")
    with S.Aligner(ref, flag) as al:
        batch = np.zeros((a.repeat, n_chunks))
        rows = []
        for rep in range(a.repeat):
            for k in range(n_chunks):
                hi = (k + 1) * a.chunk
                r = al.align_db(*packed([x[:hi] for x in reads]))
                batch[rep, k] = al.profile()["total_ms"]
                if rep == 0:
                    rows.append(r)
        ext, kept, failed = {}, {}, False
        for starts, cand in [(st, cd) for cd in ([0, a.candidates] if a.candidates else [0]) for st in (True, False)]:
            t = np.zeros((a.repeat, n_chunks))
            f = np.zeros((a.repeat, n_chunks))
            diffs, mine = [{} for _ in range(n_chunks)], []
            with al.session(n, starts=starts, candidates=cand) as se:
                for rep in range(a.repeat):
                    se.reset()
                    for k in range(n_chunks):
                        lo, hi = k * a.chunk, (k + 1) * a.chunk
                        got = se.extend(slots, *packed([x[lo:hi] for x in reads]))
                        p = al.profile()
                        t[rep, k], f[rep, k] = p["total_ms"], p["fill_ms"]
                        diffs[k] = diffs[k] or differing(got, rows[k], starts)
                        if rep == 0:
                            mine.append(got)
            ext[(starts, cand)] = (np.median(t, 0), np.median(f, 0), t)
            kept[(starts, cand)] = mine
            name = f"session starts={starts}" + (f" candidates={cand}" if cand else "")
            say(f"{name}: {verdict(diffs, 'align_db')}")
            failed = failed or any(diffs)
            if cand:  # the lists must not move the rows: the same bytes as the leg without
                plain = [differing(x, y, True) for x, y in zip(mine, kept[(starts, 0)])]
                say(f"{name}: {verdict(plain, 'the session without candidates')}")
                failed = failed or any(plain)
        b = np.median(batch, 0)
        say("chunk  prefix  align_db_ms  extend_ms(starts)  sweeps_ms  extend_ms(no_start)  sweeps_ms")
        for k in range(n_chunks):
            say(f"{k + 1:5d}  {(k + 1) * a.chunk:6d}  {b[k]:11.3f}  {ext[(True, 0)][0][k]:17.3f}  {ext[(True, 0)][1][k]:9.3f}  {ext[(False, 0)][0][k]:19.3f}  {ext[(False, 0)][1][k]:9.3f}")
        for starts in (True, False):  # run-to-run spread of the plain legs: every repeat's sum over the read
            say(f"starts={starts}: sum of extend_ms over the read per repeat: " + " ".join(f"{x:.3f}" for x in ext[(starts, 0)][2].sum(1)))
        if a.candidates:
            say(f"chunk  prefix  extend_ms(starts, {a.candidates} candidates)  ratio to without  extend_ms(no_start, {a.candidates} candidates)  ratio to without")
            for k in range(n_chunks):
                ct, cf = ext[(True, a.candidates)][0][k], ext[(False, a.candidates)][0][k]
                say(f"{k + 1:5d}  {(k + 1) * a.chunk:6d}  {ct:10.3f}  {ct / ext[(True, 0)][0][k]:6.3f}  {cf:10.3f}  {cf / ext[(False, 0)][0][k]:6.3f}")
            for starts in (True, False):
                tc = ext[(starts, a.candidates)]
                say(f"starts={starts} candidates={a.candidates}: sum over the read {tc[0].sum():.1f} ms against {ext[(starts, 0)][0].sum():.1f} ms without "
                    f"(ratio {tc[0].sum() / ext[(starts, 0)][0].sum():.3f}); per repeat: " + " ".join(f"{x:.3f}" for x in tc[2].sum(1)))
        for starts in (True, False):
            t = ext[(starts, 0)][0]
            first = next((k + 1 for k in range(n_chunks) if t[k] < b[k]), None)
            say(f"starts={starts}: extend is below align_db from chunk {first}; extend of chunk 2 / last chunk {t[1]:.3f} / {t[-1]:.3f} ms; "
                f"sum over the read {t.sum():.1f} ms against {b.sum():.1f} ms of re-alignment")
    if failed:
        sys.exit("rows differ: the times above are of sessions whose rows are not the expected ones")


if __name__ == "__main__":
    main()
