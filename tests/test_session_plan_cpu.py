"""The host rules of a session call as the library ships them (sigfish_amd/csrc/session_plan.hpp), without a GPU: the stand-alone
program tests/c/session_plan.cpp, built from that header alone with -Wall -Werror and once more under ASan + UBSan, against the
Python restatements the GPU tests rely on -- the wave planner (tests/session_waves.py: plan_call, counts) and the schedule of
the automatic query start's points (tests/autostart_oracle.py: points_between)."""
import itertools
import os
import shutil
import subprocess

import pytest

from tests import session_waves as W
from tests.autostart_oracle import points_between
from tests.util import ROOT

MAX_CLASSES = 12  # kSessionMaxClasses


def _build(tmp, sanitize):
    exe = str(tmp / ("session_plan_san" if sanitize else "session_plan"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "session_plan.cpp")]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """[plain build, sanitizer build or None]: every request goes through all of them, and their answers must be the same lines"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("session_plan")
    exe, build = _build(tmp, False)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    san, build = _build(tmp, True)
    # (the plain build went through, so the source compiles; only a toolchain that says its sanitizer runtime is missing counts as without)
    if build.returncode != 0 and any(m in build.stderr for m in (b"libasan", b"libubsan", b"-lasan", b"-lubsan", b"unrecognized command-line option", b"unsupported option")):
        san = None
    else:
        assert build.returncode == 0, build.stderr.decode()[-2000:]
    return [exe, san]


def _ask(programs, text):
    outs = []
    for exe in programs:
        if exe is None:
            continue
        run = subprocess.run([exe], input=text.encode(), capture_output=True, timeout=300)
        assert run.returncode == 0, (run.returncode, (run.stdout + run.stderr).decode()[-3000:])
        assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]
        outs.append(run.stdout.decode().splitlines())
    assert all(o == outs[0] for o in outs)
    return outs[0]


def test_the_program_runs_under_sanitizers(programs):
    if programs[1] is None:
        pytest.skip("toolchain without sanitizer runtimes")
    assert _ask(programs[1:], "plan 2 1\n0 5 0 0\nauto 0 10 1 0 100 0 0\n")[-1] == "auto 0 0 10 0 1 1"


# ---- the wave planner ----
def _parse_call(lines):
    """-> (new_events, call_slot, [launch]); launch: dict(n_cls, n_tasks, cls, g_qlen, w_entry, groups) with groups as lists of
    (call, slot, len, total, first) in task order"""
    head = lines[0].split()
    assert head[0] == "call"
    n_launches, new_events, call_slot = int(head[1]), int(head[2]), [int(x) for x in head[3:]]
    launches, at = [], 1
    for _ in range(n_launches):
        tag, n_cls, n_tasks, n_groups, n_entries = lines[at].split()
        assert tag == "launch"
        at += 1
        rows = {}
        for kind, count in (("cls", int(n_cls)), ("group", int(n_groups)), ("entry", int(n_entries))):
            rows[kind] = [[int(x) for x in ln.split()[1:]] for ln in lines[at:at + count]]
            assert all(ln.split()[0] == kind for ln in lines[at:at + count])
            at += count
        groups = []
        for g, (qlen, *w) in enumerate(rows["group"]):
            first = [c[2] for c in rows["cls"] if c[3] <= g < c[3] + c[4]]
            assert len(first) == 1  # every group lies in exactly one class
            assert all(e >= 0 for e in w[:sum(e >= 0 for e in w)])  # entries first, then the padding
            groups.append([tuple(rows["entry"][e][:4]) + (first[0],) for e in w if e >= 0])
        # the entries are the groups' pieces in task order, each once, and their events lie where the chunks were laid out
        assert [e for _, *w in rows["group"] for e in w if e >= 0] == list(range(int(n_entries)))
        launches.append(dict(n_cls=int(n_cls), n_tasks=int(n_tasks), cls=[tuple(c) for c in rows["cls"]], g_qlen=[g[0] for g in rows["group"]],
                             w_entry=[tuple(g[1:]) for g in rows["group"]], groups=groups, off=[e[4] for e in rows["entry"]]))
    assert at == len(lines)
    return new_events, call_slot, launches


def _expected(chunks, held, poisoned, n_jobs):
    """the same from W.plan_call; a poisoned slot is planned as a chunk without events (it keeps its place in the call)"""
    eff = [(s, 0 if s in poisoned else n) for s, n in chunks]
    launches = []
    for gs in W.plan_call(eff, held):
        cls = []
        for g, grp in enumerate(gs):
            if not cls or cls[-1][:3] != (grp.R, grp.lanes, grp.first):
                cls.append((grp.R, grp.lanes, grp.first, g, 0, g * n_jobs))
            cls[-1] = cls[-1][:4] + (cls[-1][4] + 1, cls[-1][5])
        launches.append(dict(n_cls=len(cls), n_tasks=len(gs) * n_jobs, cls=cls, g_qlen=[g.qlen for g in gs],
                             w_entry=None, groups=[[tuple(p) for p in g.pieces] for g in gs]))
    call_slot = [s if n > 0 else -1 for s, n in eff]
    return sum(n for _, n in eff), call_slot, launches, W.counts(W.plan_call(eff, held), n_jobs)


def _matrix(kind):
    m = W.build_matrix(kind)
    return list(zip(m.slots, m.lens)), dict(zip(m.slots, m.prefix))


CALLS = {
    "three launches": ([(0, 4097)], {}, ()),
    "seven slots mixed": ([(0, 9), (1, 61), (2, 5), (3, 1), (4, 60), (5, 13), (6, 300)], {6: 10}, ()),
    "matrix first": _matrix("first") + ((),),
    "matrix carried": _matrix("carried") + ((),),
    "a poisoned slot": ([(0, 9), (5, 2100), (2, 70)], {5: 40, 2: 3}, (5,)),
    "a zero-length chunk": ([(4, 300), (1, 0), (9, 2049)], {1: 50}, ()),
    "all chunks empty": ([(3, 0), (1, 0)], {3: 7}, ()),
}


@pytest.mark.parametrize("n_jobs", [1, 18])
@pytest.mark.parametrize("name", list(CALLS))
def test_planner_equals_the_restatement(programs, name, n_jobs):
    chunks, held, poisoned = CALLS[name]
    text = f"plan {n_jobs} {len(chunks)}\n" + "".join(f"{s} {n} {held.get(s, 0)} {int(s in poisoned)}\n" for s, n in chunks)
    new_events, call_slot, got = _parse_call(_ask(programs, text))
    want_events, want_slot, want, (n_tasks, n_launches) = _expected(chunks, held, poisoned, n_jobs)
    assert (new_events, call_slot, len(got)) == (want_events, want_slot, n_launches)
    assert sum(la["n_tasks"] for la in got) == n_tasks
    starts = dict(zip(range(len(chunks)), itertools.accumulate([0] + [n for _, n in chunks])))  # chunks back to back
    for p, (g, w) in enumerate(zip(got, want)):
        assert g["groups"] == w["groups"], (name, p)                      # (call, slot, len, total, first) per group, task order
        assert g["g_qlen"] == w["g_qlen"], (name, p)
        cap = [64 // next(c[1] for c in g["cls"] if c[3] <= i < c[3] + c[4]) for i in range(len(g["groups"]))]
        at = 0
        for grp, we, ns in zip(g["groups"], g["w_entry"], cap):          # w_entry: the group's entries, padded with -1
            assert len(grp) <= ns and we == tuple(range(at, at + len(grp))) + (-1,) * (4 - len(grp)), (name, p)
            at += len(grp)
        assert g["cls"] == w["cls"], (name, p)                            # (R, lanes, first, group_base, n_groups, task_base)
        assert g["n_tasks"] == w["n_tasks"] and g["n_cls"] == w["n_cls"] <= MAX_CLASSES, (name, p)
        flat = [e for grp in g["groups"] for e in grp]
        assert g["off"] == [starts[call] + p * W.MAX_PIECE for call, *_ in flat], (name, p)
    if name == "a poisoned slot":
        assert call_slot == [0, -1, 2] and all(e[1] != 5 for la in got for grp in la["groups"] for e in grp)
    if name == "all chunks empty":
        assert got == [] and call_slot == [-1, -1] and new_events == 0
    if name == "a zero-length chunk":
        assert call_slot == [4, -1, 9] and len(got) == 2
    if name.startswith("matrix"):
        assert got[0]["n_cls"] == 6


# ---- the points of the automatic query start ----
COUNTS = [0, 1, 999, 1000, 1001, 3999, 4000, 4001, 5999, 6000, 6001, 12000]


def _cells():
    for every, max_samples, ended in itertools.product((0, 1000, 4000), (4000, 6000, 10000), (False, True)):
        for have, after in itertools.combinations_with_replacement(COUNTS, 2):
            if have < max_samples:  # (beyond it the final point has been taken: settled)
                yield every, max_samples, ended, have, after, (min(have, max_samples) // every if every else 0)


def test_point_schedule_equals_the_restatement(programs):
    cells = list(_cells())
    assert len(cells) > 1000
    text = "".join(f"auto {have} {after} {int(ended)} {every} {m} {k_done} {settled}\n" for every, m, ended, have, after, k_done in cells for settled in (0, 1))
    lines = _ask(programs, text)
    assert len(lines) == 2 * len(cells)
    n_periodic_cells = n_final_cells = n_merged = 0
    for i, (every, m, ended, have, after, k_done) in enumerate(cells):
        tag, n0, n_periodic, n_final, k_after, final_now, pending = lines[2 * i].split()
        got = [int(n0) + j * every for j in range(int(n_periodic))]
        pts, final = points_between(have, after, ended, every, m)
        cell = (every, m, ended, have, after)
        assert tag == "auto" and int(n_final) == (-1 if final is None else final), cell
        assert [p for p in got if p != int(n_final)] == pts, cell
        assert len(got) - len(pts) in (0, 1) and int(final_now) == int(final is not None), cell
        assert int(k_after) == (min(after, m) // every if every else 0), cell
        assert int(pending) == int(bool(pts) or final is not None), cell
        # settled (frozen, or final point already taken): nothing is pending, whatever else holds, and k_done stands
        s = lines[2 * i + 1].split()
        assert s[0] == "auto" and int(s[6]) == 0 and int(s[5]) == 0 and int(s[3]) == -1 and int(s[4]) == k_done, cell
        n_periodic_cells += bool(pts)
        n_final_cells += final is not None
        n_merged += len(got) - len(pts)
    assert n_periodic_cells > 100 and n_final_cells > 100 and n_merged > 10  # (the cells reach every branch of the rule)
