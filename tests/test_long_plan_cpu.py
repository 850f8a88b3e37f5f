"""The plan of a batch's reads beyond 2048 events (sfa_plan.hpp, plan_long_reads), which the row strips' driver in sfa_align.hip
stages, slices and launches from: the stand-alone program tests/c/long_plan.cpp, built with -Wall -Werror and once more under
ASan + UBSan, prints one line per plan.  What a plan has to say is stated here, by formula, from the line's inputs."""
import os
import shutil
import subprocess

import pytest

from tests.util import ROOT

CSRC = os.path.join(ROOT, "sigfish_amd", "csrc")
NCOV = [29898, 29898]
THREE = [100, 5000, 29898]
# sdtw_strips.hpp: strips of 64 lanes x 32 rows; a checkpoint record is 33 planes of 64 floats; 256 words behind every boundary row;
# a boundary row is handed over in blocks of 256 columns
STRIP_ROWS, CK_REC, BND_PAD, PIPE_BLOCK = 2048, 33 * 64, 256, 256


def _build(tmp, sanitize):
    exe = str(tmp / ("long_plan_san" if sanitize else "long_plan"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "c", "long_plan.cpp")]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """[lines of the plain build, lines of the sanitizer build or None]"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("long_plan")
    exe, build = _build(tmp, False)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    san, build = _build(tmp, True)
    # (the plain build went through, so the source compiles; only a toolchain that says its sanitizer runtime is missing counts as without)
    if build.returncode != 0 and any(m in build.stderr for m in (b"libasan", b"libubsan", b"-lasan", b"-lubsan", b"unrecognized command-line option", b"unsupported option")):
        san = None
    else:
        assert build.returncode == 0, build.stderr.decode()[-2000:]
    outs = []
    for prog in (exe, san):
        if prog is None:
            outs.append(None)
            continue
        run = subprocess.run([prog], capture_output=True, timeout=600)
        assert run.returncode == 0, (run.returncode, (run.stdout + run.stderr).decode()[-3000:])
        assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]
        outs.append(run.stdout.decode().splitlines())
    return outs


def _ints(v):
    return [] if v == "-" else [int(x) for x in v.split(",")]


@pytest.fixture(scope="module")
def plans(outputs):
    """name -> the plan's line as a dict: lists for the arrays, ints for the rest, groups as (begin, size, set, off_word, strips)"""
    out = {}
    for ln in outputs[0]:
        if not ln.startswith("plan "):
            continue
        name, *items = ln.split()[1:]
        p = dict(it.split("=", 1) for it in items)
        for k, v in p.items():
            if k == "groups":
                p[k] = [] if v == "-" else [tuple(int(x) for x in g.split(":")) for g in v.split(";")]
            elif k in ("jobs", "qlens", "reads", "n_strips", "bnd_off", "ck_off", "strip_off"):
                p[k] = _ints(v)
            else:
                p[k] = int(v)
        assert name not in out
        out[name] = p
    return out


def _long(p):
    """(batch index, events) of the reads beyond 2048 events, input order"""
    return [(i, l) for i, l in enumerate(p["qlens"]) if l > STRIP_ROWS]


def _ck_bytes_per_read(p, shift):
    """checkpoint records of one read: every job, every strip of the longest read, every 1 << shift steps; 33 x 64 floats each"""
    return sum(p["max_strips"] * ((m - 1) >> shift) for m in p["jobs"]) * CK_REC * 4


def test_both_builds_print_the_same_lines(outputs):
    if outputs[1] is None:
        pytest.skip("toolchain without sanitizer runtimes")
    assert outputs[0] == outputs[1]


def test_every_case_was_planned(outputs, plans):
    assert not [ln for ln in outputs[0] if ln.startswith("FAIL")]
    assert outputs[0][-1] == f"done {len(plans)}" and len(plans) == 25
    assert outputs[0][0] == "consts kStripR=32 kStripRows=2048 kCkRec=2112 kBndPad=256 kPipeBlock=256 kMaxQuery=2048"
    assert {tuple(p["jobs"]) for p in plans.values()} == {tuple(NCOV), tuple(THREE)}
    assert {l for p in plans.values() for _, l in _long(p)} == {2049, 2500, 4096, 4097, 5000, 6500, 20000}


def test_long_reads_strip_counts_and_cells(plans):
    """ceil(events / 2048) strips per read; reads in input order; events and max for the profile's cell count"""
    for name, p in plans.items():
        lr = _long(p)
        assert p["n_long"] == len(lr) and p["reads"] == [i for i, _ in lr], name
        assert p["n_strips"] == [-(-l // STRIP_ROWS) for _, l in lr], name
        assert p["events"] == sum(l for _, l in lr) and p["max"] == max([l for _, l in lr], default=0), name
        assert p["max_strips"] == max(p["n_strips"], default=0), name
    assert [plans[n]["n_strips"] for n in ("one_2049", "one_4096", "one_4097")] == [[2], [2], [3]]
    assert plans["mixed"]["reads"] == [1, 2, 4, 5, 7] and plans["mixed"]["n_strips"] == [2, 4, 3, 10, 2] and plans["mixed"]["max_strips"] == 10
    none = plans["none"]  # no read beyond 2048 events: nothing to stage, nothing to launch
    assert none["n_long"] == 0 and none["n_groups"] == 0 and none["groups"] == [] and none["events"] == 0


def test_boundary_rows(plans):
    """a row of job_len + 256 words, rounded up to 4; max(1, max_strips - 1) rows per read and job, the reads' rows behind each other"""
    for name, p in plans.items():
        if not p["n_long"]:
            continue
        off = p["bnd_off"]
        assert len(off) == len(p["jobs"]) + 1 and off[0] == 0 and all(o % 4 == 0 for o in off), name
        assert [b - a for a, b in zip(off, off[1:])] == [(m + BND_PAD + 3) // 4 * 4 for m in p["jobs"]], name
        assert p["cost_rows"] == max(1, p["max_strips"] - 1), name
        assert p["bnd_stride"] == p["cost_rows"] * off[-1], name
    assert plans["mixed"]["bnd_off"] == [0, 356, 356 + 5256, 356 + 5256 + 30156] and plans["mixed"]["cost_rows"] == 9
    assert plans["one_2049"]["cost_rows"] == 1 and plans["one_4097"]["cost_rows"] == 2


def test_checkpoint_interval(plans):
    """T = 512 when that fits the budget for all long reads together; the option's power of two, budget not consulted; else doubling,
    16 384 at most.  ck_off: prefix sum over the jobs of max_strips * ((job_len - 1) >> ck_shift)."""
    for name, p in plans.items():
        if not p["n_long"]:
            continue
        if p["interval"] > 0:
            want = p["interval"].bit_length() - 1
            assert 1 << want == p["interval"]
        else:
            want = 9
            while _ck_bytes_per_read(p, want) * p["n_long"] > p["budget"] and want < 14:
                want += 1
        assert p["ck_shift"] == want, name
        per_job = [p["max_strips"] * ((m - 1) >> want) for m in p["jobs"]]
        assert p["ck_off"] == [sum(per_job[:j]) for j in range(len(per_job) + 1)], name
    assert [plans[n]["ck_shift"] for n in ("interval_4", "interval_64", "interval_512")] == [2, 6, 9]  # with a budget of one byte
    assert [plans[n]["ck_shift"] for n in ("one_2049", "mixed", "groups_16gib", "waves_at_cu256")] == [9, 9, 9, 9]
    got = [plans[n]["ck_shift"] for n in ("budget_fits_9", "budget_below_9", "budget_fits_10", "budget_below_10", "budget_below_11", "budget_one_byte")]
    assert got == [9, 10, 10, 11, 12, 14]
    one = plans["budget_one_byte"]
    assert _ck_bytes_per_read(one, 14) * one["n_long"] > one["budget"]  # still over the budget at the cap
    assert plans["mixed"]["ck_off"] == [0, 0, 10 * 9, 10 * 9 + 10 * 58]  # the 100-column job has no checkpoint


def _groups_by_rule(p):
    """(reads per group, two sets): two groups when the waves of pass 1 (one per read, job and strip) are at least four rounds of 16
    wave slots per CU, and no more reads than fit the budget twice over (boundary rows + checkpoints of a read, two sets of scratch)"""
    n = p["n_long"]
    waves = sum(p["n_strips"]) * len(p["jobs"])
    want_groups = 2 if waves >= 4 * 16 * p["cu"] else 1
    per_read = p["bnd_stride"] * 4 + _ck_bytes_per_read(p, p["ck_shift"])
    group = max(1, min(-(-n // want_groups), p["budget"] // (2 * per_read)))
    return group, group < n


def test_groups(plans):
    for name, p in plans.items():
        if not p["n_long"]:
            continue
        group, two = _groups_by_rule(p)
        n = p["n_long"]
        assert (p["group"], p["two_sets"]) == (group, int(two)), name
        assert p["n_groups"] == -(-n // group) == len(p["groups"]), name
        for gi, (begin, size, gset, _, _) in enumerate(p["groups"]):
            assert (begin, size, gset) == (gi * group, min(group, n - gi * group), gi & 1 if two else 0), (name, gi)

    def shape(name):
        p = plans[name]
        return p["group"], p["two_sets"], [g[1] for g in p["groups"]], [g[2] for g in p["groups"]]

    assert shape("groups_1mib") == (1, 1, [1, 1, 1], [0, 1, 0])  # what test_row_strips_ncov_and_groups sets up on the device
    assert shape("groups_16gib") == (3, 0, [3], [0])
    assert shape("one_2049") == (1, 0, [1], [0])
    assert sum(plans["waves_below_cu1"]["n_strips"]) * 2 == 62 and shape("waves_below_cu1") == (15, 0, [15], [0])
    assert sum(plans["waves_at_cu1"]["n_strips"]) * 2 == 64 and shape("waves_at_cu1") == (8, 1, [8, 8], [0, 1])
    assert sum(plans["waves_below_cu256"]["n_strips"]) * 2 == 16382 and shape("waves_below_cu256") == (823, 0, [823], [0])
    assert sum(plans["waves_at_cu256"]["n_strips"]) * 2 == 16384 and shape("waves_at_cu256") == (410, 1, [410, 410], [0, 1])
    assert shape("two_per_set") == shape("two_per_set_upper") == (2, 1, [2, 2, 1], [0, 1, 0])


def test_strip_offset_words(plans):
    """group gi, from read g0, has the prefix sum of its reads' strip counts at words g0 + gi ... g0 + gi + gn of the staging area's
    last section; groups follow each other without sharing a word; the last word lies inside the staging area"""
    for name, p in plans.items():
        if not p["n_long"]:
            continue
        words = p["strip_off"]
        assert p["sg_soff"] + 4 * len(words) == p["sg_bytes"], name
        end = 0
        for gi, (g0, gn, _, word, strips) in enumerate(p["groups"]):
            assert word == g0 + gi and word >= end, (name, gi)
            end = word + gn + 1
            mine = p["n_strips"][g0:g0 + gn]
            assert words[word:end] == [sum(mine[:i]) for i in range(gn + 1)], (name, gi)
            assert strips == sum(mine), (name, gi)
        assert end <= len(words), name
    assert plans["groups_1mib"]["strip_off"][:6] == [0, 2, 0, 3, 0, 2]
    assert plans["two_per_set"]["strip_off"][:8] == [0, 3, 6, 0, 3, 6, 0, 3]


def test_staging_layout(plans):
    """reads[n_long] (32-bit) | bnd_off[n_jobs + 1] (64-bit) | ck_off[n_jobs + 1] (64-bit) | the strip-offset words, with room for
    n_long groups of one read (two words each)"""
    for name, p in plans.items():
        if not p["n_long"]:
            continue
        n, jobs = p["n_long"], len(p["jobs"])
        assert p["sg_reads"] == 0 and p["sg_reads"] + 4 * n <= p["sg_bnd"], name
        assert p["sg_bnd"] % 8 == 0 and p["sg_bnd"] + 8 * (jobs + 1) <= p["sg_ck"], name
        assert p["sg_ck"] % 8 == 0 and p["sg_ck"] + 8 * (jobs + 1) <= p["sg_soff"], name
        assert p["sg_soff"] % 4 == 0 and p["sg_soff"] + 4 * 2 * n <= p["sg_bytes"], name
        assert p["sg_bytes"] <= 4 * (n + 1) + 16 * (jobs + 1) + 4 * (2 * n + 2), name  # and no larger than its sections, padded once
    assert plans["groups_1mib"]["sg_bnd"] == 16 and plans["one_2049"]["sg_bnd"] == 8  # three reads / one read, padded to 8 bytes


def test_scratch_sizes(plans):
    """of one set: a progress word per (read of a group, job, strip), the boundary rows and the checkpoints of a group's reads
    (one float at least per read); the partial results of all (read, job) pairs"""
    for name, p in plans.items():
        if not p["n_long"]:
            continue
        jobs = len(p["jobs"])
        assert p["prog_bytes"] == 4 * p["group"] * jobs * p["max_strips"], name
        assert p["bndc_floats"] == p["bnd_stride"] * p["group"], name
        assert p["lck_floats"] == max(_ck_bytes_per_read(p, p["ck_shift"]) // 4, 1) * p["group"], name
        assert p["n_part"] == p["n_long"] * jobs, name
        if p["interval"] == 0 and p["n_groups"] > 1:  # two sets of a group's boundary rows and checkpoints fit the budget, unless a single read does not
            assert p["group"] == 1 or 2 * 4 * (p["bndc_floats"] + p["lck_floats"]) <= p["budget"], name


def test_wait_limit(plans):
    """the option, but never less than (256 + 72) columns x max_strips at 10 us each, rounded up to whole ms"""
    for name, p in plans.items():
        if p["n_long"]:
            assert p["limit_ms"] == max(p["spin"], (PIPE_BLOCK + 72) * p["max_strips"] // 100 + 1), name
    assert plans["limit_option"]["limit_ms"] == 20000
    assert plans["limit_floor"]["limit_ms"] == 33  # ten strips
    assert plans["limit_floor_short"]["limit_ms"] == 7  # two strips


def test_one_long_read_and_long_reads_only(plans):
    one = plans["one_4097"]
    assert one["n_long"] == 1 and one["reads"] == [0] and one["groups"] == [(0, 1, 0, 0, 3)] and one["strip_off"] == [0, 3, 0, 0]
    only = plans["groups_16gib"]
    assert only["reads"] == [0, 1, 2] == list(range(len(only["qlens"]))) and only["groups"] == [(0, 3, 0, 0, 7)]
