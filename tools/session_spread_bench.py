#!/usr/bin/env python3
"""What a spread session (SFA_SESSION_SPREAD) costs per sfa_session_extend call, and whether plain sessions are unharmed.

--slots (512) slots x the nCoV model, --events (180) events per slot and call, every slot named in every call.  Legs:
  plain        a plain session on device 0
  spread[0]    a spread session on a context over [0]: the plain session behind the flag
  spread[0,0]  a spread session on a context over [0, 0]: two shards on ONE GPU -- this measures the layer (partition, packing,
               the shard thread, two smaller launches), not scaling
  spread[all]  where the box has several GPUs, a spread session over all of them
Every leg has its own context and session.  After --warmup (5) rounds, --calls (40) rounds are timed; in a round every leg makes
one call, in turn (interleaved: drift hits all legs alike); the slots are never reset, so every timed call extends carried rows
and does the same work.  Wall time per call is a host clock around Session.extend, which
returns after the call's device work has been waited for; beside it the device time the library reports (sfa_profile_t.total_ms:
on a group context the slowest shard's).  Reported per leg: median, 10th / 90th percentile, minimum, maximum.  The rows of every
leg are compared with the plain leg's in the first round (they must be the same bytes).

--parent-lib PATH: a library built from the parent commit.  Then plain sessions are timed on both builds, in child processes of
their own (a process loads one library), alternating parent / branch, --ab-repeats (5) times each: the medians per repeat are
listed, and the verdict compares the difference of their medians with the spread of the PARENT's own repeats -- nothing tighter can
be told from noise.  (--leg-only plain is what a child runs: one leg, one JSON line.)

Lines are stamped with the build id and appended to profiles/session_spread_<build id>/session_spread_bench.log, the numbers to
session_spread_bench.json beside it (--no-log: stdout only).  rocm-smi --showclocks is asked once, idle, before the first leg: the
clocks under load are not read."""
import argparse
import json
import os
import subprocess
import sys
import time

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


def stats(x):
    x = np.asarray(x, float)
    return dict(median=float(np.median(x)), p10=float(np.percentile(x, 10)), p90=float(np.percentile(x, 90)), min=float(x.min()), max=float(x.max()), n=int(len(x)))


def fmt(s):
    return f"median {s['median']:.3f} ms, p10 {s['p10']:.3f}, p90 {s['p90']:.3f}, min {s['min']:.3f}, max {s['max']:.3f} ({s['n']} calls)"


def workload(a):
    ref, flag, q, q_off, _ = synth.workload("ncov_r9_dna_q250", n_reads=a.slots, seed=11)
    rng = np.random.default_rng(3)
    # every slot sends --events events per call: drawn once from the workload's queries, the same chunk in every call
    # (a carried row's cost does not depend on what the events are)
    ev = np.concatenate([np.resize(q[q_off[i]:q_off[i + 1]] if q_off[i + 1] > q_off[i] else rng.normal(size=8).astype(np.float32), a.events) for i in range(a.slots)])
    return ref, flag, ev.astype(np.float32), np.arange(a.slots + 1, dtype=np.int64) * a.events


def run_legs(a, legs):
    """legs: [(name, devices or None)] -> {name: dict(wall=stats, device=stats)}; rows of every leg against the first's"""
    ref, flag, ev, off = workload(a)
    slots = np.arange(a.slots, dtype=np.int32)
    open_legs = []
    for name, devices in legs:
        al = S.Aligner(ref, flag) if devices is None else S.Aligner(ref, flag, devices=devices)
        open_legs.append((name, al, al.session(a.slots, spread=devices is not None)))
    wall = {name: [] for name, _ in legs}
    dev = {name: [] for name, _ in legs}
    try:
        for rnd in range(a.warmup + a.calls):
            first = None
            for name, al, se in open_legs:
                t0 = time.perf_counter()
                rows = se.extend(slots, ev, off)
                t1 = time.perf_counter()
                if rnd == 0:
                    first = rows if first is None else first
                    if rows.tobytes() != first.tobytes():
                        raise SystemExit(f"rows of leg {name} differ from the plain leg's")
                if rnd >= a.warmup:
                    wall[name].append(1e3 * (t1 - t0))
                    dev[name].append(al.profile()["total_ms"])
    finally:
        for _, al, se in open_legs:
            se.close()
            al.close()
    return {name: dict(wall=stats(wall[name]), device=stats(dev[name])) for name, _ in legs}


def child(a, lib):
    """one plain leg in a process of its own, on the library `lib` -> its stats"""
    env = dict(os.environ, SFA_LIB=lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg-only", "plain", "--no-log", "--slots", str(a.slots), "--events", str(a.events), "--calls", str(a.calls),
           "--warmup", str(a.warmup)]
    r = subprocess.run(["timeout", "-k", "10", str(a.timeout)] + cmd, env=env, capture_output=True)
    if r.returncode != 0:
        raise SystemExit(f"the child on {lib} failed ({r.returncode}): {r.stderr.decode()[-2000:]}")
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def main():
    global LOG
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=512)
    ap.add_argument("--events", type=int, default=180)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libsigfish_amd.so built from the parent commit: plain sessions on both builds")
    ap.add_argument("--ab-repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--leg-only", default=None, help="(what a child runs) one leg, one JSON line")
    ap.add_argument("--no-log", action="store_true")
    a = ap.parse_args()
    if a.leg_only:
        res = run_legs(a, [("plain", None)])["plain"]
        print(json.dumps(dict(build_id=S.build_id(), **res)))
        return 0
    out_dir = os.path.join(ROOT, "profiles", f"session_spread_{S.build_id()}")
    if not a.no_log:
        os.makedirs(out_dir, exist_ok=True)
        LOG = os.path.join(out_dir, "session_spread_bench.log")
    try:
        clocks = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, timeout=60).stdout.decode()
        say("clocks, idle, before the first leg (rocm-smi --showclocks): " + "; ".join(ln.strip() for ln in clocks.splitlines() if "clk" in ln and "GPU[0]" in ln))
    except Exception as e:  # (a note, not a measurement)
        say(f"clocks: rocm-smi --showclocks not available ({e})")
    import torch
    n_gpus = torch.cuda.device_count()
    legs = [("plain", None), ("spread[0]", [0]), ("spread[0,0]", [0, 0])] + ([(f"spread[all {n_gpus}]", list(range(n_gpus)))] if n_gpus > 1 else [])
    say(f"{a.slots} slots x nCoV, {a.events} events per slot and call, {a.warmup} warm-up rounds, {a.calls} timed rounds, legs interleaved; {n_gpus} GPU(s) visible")
    res = run_legs(a, legs)
    for name, _ in legs:
        say(f"{name:14s} wall   {fmt(res[name]['wall'])}")
        say(f"{name:14s} device {fmt(res[name]['device'])}")
    base = res["plain"]["wall"]["median"]
    for name, _ in legs[1:]:
        say(f"{name} against plain: {res[name]['wall']['median'] - base:+.3f} ms per call (wall, medians), {res[name]['wall']['median'] / base:.3f} x")
    if n_gpus <= 1:
        say("one GPU: spread[0,0] is two shards on the same device -- the cost of the layer, not scaling; no scaling figure is claimed")
    report = dict(build_id=S.build_id(), slots=a.slots, events=a.events, calls=a.calls, warmup=a.warmup, gpus=n_gpus, legs=res)
    if a.parent_lib:
        mine = os.path.join(ROOT, "sigfish_amd", "lib", "libsigfish_amd.so")
        ab = {"parent": [], "branch": []}
        for rep in range(a.ab_repeats):  # alternating: parent, branch, parent, ...
            for who, lib in (("parent", a.parent_lib), ("branch", mine)):
                r = child(a, lib)
                ab[who].append(r)
                say(f"plain session, {who} build {r['build_id']}, repeat {rep + 1}: wall {fmt(r['wall'])}; device median {r['device']['median']:.3f} ms")
        pm, bm = [r["wall"]["median"] for r in ab["parent"]], [r["wall"]["median"] for r in ab["branch"]]
        pd, bd = [r["device"]["median"] for r in ab["parent"]], [r["device"]["median"] for r in ab["branch"]]
        margin, margin_d = max(pm) - min(pm), max(pd) - min(pd)
        diff, diff_d = float(np.median(bm) - np.median(pm)), float(np.median(bd) - np.median(pd))
        say(f"plain sessions, branch against parent (medians of {a.ab_repeats} repeats): wall {diff:+.3f} ms per call, the parent's own repeats span {margin:.3f} ms -> "
            + ("within the parent's spread" if abs(diff) <= margin else ("SLOWER than the parent's spread" if diff > 0 else "faster than the parent's spread")))
        say(f"  device time: {diff_d:+.3f} ms per call, the parent's own repeats span {margin_d:.3f} ms")
        report["parent_vs_branch"] = dict(parent=ab["parent"], branch=ab["branch"], wall_diff_ms=diff, wall_parent_span_ms=margin, device_diff_ms=diff_d, device_parent_span_ms=margin_d)
    if not a.no_log:
        with open(os.path.join(out_dir, "session_spread_bench.json"), "w") as f:
            json.dump(report, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
