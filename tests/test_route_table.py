"""The route of every batch (sfa_plan.hpp, choose_route) on synthetic batches, CPU only: tests/c/route_table.cpp runs the
planner and the route function.  Expected routes follow the conditions the alignment stage has always used: pass 2 rides in
the fill launch when the launch has more tasks than wave slots (fused_trace=1) or always (2), never at 0; LDS checkpoints need
R <= 16 and queries of <= 256 events (lds_ckpt=1) or <= 1024 (2), and at lds_ckpt=1 the planner drops them for batches of
(4, 6] tasks per SIMD; the 32-row fill carries pass 2 only for subsequence DTW with checkpoints; column segments for small
sDTW batches of the 64-lane shapes; secondaries take the plain two-pass route whatever else is set.

Every case runs with 8 SIMDs (32 wave slots on the LDS route) and one reference job unless it says otherwise, so a batch of
n reads of <= 256 events at 16 lanes per read is n/4 tasks."""
import os
import shutil
import subprocess

import pytest

from tests.util import ROOT

CASES = {
    # LDS window at lds_ckpt=1 (R = 8): <= 4x SIMDs: LDS, pass 2 on its own; (4, 6]x: no LDS; > 6x: LDS + fused pass 2
    "lds_at_4x": ("n=128", "Lds"),
    "lds_dropped_above_4x": ("n=132", "TwoPass"),
    "lds_dropped_at_6x": ("n=192", "TwoPass"),
    "lds_fused_above_6x": ("n=196", "LdsFused"),
    "lds_fused_always": ("n=128 fused=2", "LdsFused"),
    "lds_fused_never": ("n=196 fused=0", "Lds"),
    "lds2_keeps_window": ("n=132 lds=2", "LdsFused"),
    "lds2_within_slots": ("n=128 lds=2", "Lds"),
    "lds_off": ("n=196 lds=0", "TwoPass"),
    "lds_off_by_interval": ("n=196 interval=512", "TwoPass"),
    # query-length limits of the LDS route
    "lds1_q256": ("n=128 qlen=256", "Lds"),
    "lds1_q257_r16": ("n=64 qlen=257 widening=2", "TwoPass"),
    "lds2_q257_r16": ("n=64 qlen=257 widening=2 lds=2", "Lds"),
    "lds2_q1024_r16": ("n=32 qlen=1024 widening=2 lds=2", "Lds"),
    "lds2_q1024_fused": ("n=33 qlen=1024 widening=2 lds=2", "LdsFused"),
    "lds1_q1024_r16": ("n=33 qlen=1024 widening=2", "TwoPass"),
    "lds2_q1025_r32": ("n=33 qlen=1025 widening=2 lds=2", "Fused32"),
    # the 32-row fill (R = 32): fused when tasks (quads x chunks) exceed the wave slots
    "r32_within_slots": ("n=128 qlen=300", "TwoPass"),
    "r32_fused": ("n=132 qlen=300", "Fused32"),
    "r32_fused_always": ("n=4 qlen=300 fused=2", "Fused32"),
    "r32_fused_never": ("n=200 qlen=300 fused=0", "TwoPass"),
    "r32_chunks_within_slots": ("n=32 qlen=300 jobs=4", "TwoPass"),
    "r32_chunks_fused": ("n=36 qlen=300 jobs=4", "Fused32"),
    "r32_ck_shift_0": ("n=200 qlen=300 interval=1", "TwoPass"),
    "r32_ck_shift_2": ("n=200 qlen=300 interval=4", "Fused32"),
    "r32_std": ("n=200 qlen=300 std=1", "TwoPass"),
    "r32_std_fused_always": ("n=200 qlen=300 std=1 fused=2", "TwoPass"),
    # std_dtw with R <= 16: the LDS route (sparse HBM store), same window
    "std_lds": ("n=128 std=1", "Lds"),
    "std_lds_dropped": ("n=132 std=1", "TwoPass"),
    "std_lds_fused": ("n=196 std=1", "LdsFused"),
    # small batches (lane widening by batch size): column segments unless turned off or std_dtw
    "small_segments": ("n=8 qlen=200 widening=0", "Segments"),
    "small_two_segments": ("n=8 qlen=200 widening=0 segments=2", "Segments"),
    "small_no_segments": ("n=8 qlen=200 widening=0 segments=1", "Lds"),
    "small_no_segments_no_lds": ("n=8 qlen=200 widening=0 segments=1 lds=0", "TwoPass"),
    "small_std": ("n=8 qlen=200 widening=0 std=1", "Lds"),
    # every query beyond 2048 events: row strips only
    "no_quads": ("n=4 qlen=3000", "NoQuads"),
}


def _run(tmp_path, lines):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "route_table")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "sigfish_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "route_table.cpp"), "-o", exe])
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return dict(l.split(" ", 1) for l in out.splitlines())


def test_route_table(tmp_path):
    lines = [f"{name} {args}" for name, (args, _) in CASES.items()]
    # secondary mappings: the plain two-pass route under every other setting (a batch without quads has no wave kernels)
    lines += [f"{name}_sec{k} {args} sec={k}" for name, (args, _) in CASES.items() for k in (1, 4)]
    got = _run(tmp_path, lines)
    want = {name: route for name, (_, route) in CASES.items()}
    want.update({f"{name}_sec{k}": ("NoQuads" if route == "NoQuads" else "Secondary") for name, (_, route) in CASES.items() for k in (1, 4)})
    assert got == want
    assert set(want.values()) == {"NoQuads", "Segments", "Lds", "LdsFused", "Fused32", "Secondary", "TwoPass"}
