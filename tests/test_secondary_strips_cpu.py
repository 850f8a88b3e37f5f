"""Secondary mappings of reads beyond 2048 events ("secondary_strips"), the parts that need no GPU: the command line's checks, the
option in the header, the planner's sizes and offsets (the stand-alone program tests/c/long_plan_sec.cpp, built with -Wall -Werror
and once more under ASan + UBSan).  The merge rule of the strips' lists against update_aln: tests/test_row_rules_cpu.py."""
import os
import shutil
import subprocess

import pytest

from tests.util import ROOT

CSRC = os.path.join(ROOT, "sigfish_amd", "csrc")
EXE = os.path.join(ROOT, "sigfish_amd", "bin", "sigfish-amd")


def _cli(*args):
    if not os.path.exists(EXE):
        pytest.skip("command line not built")
    return subprocess.run([EXE, "dtw", *args, "/nonexistent.fa", "/nonexistent.blow5"], capture_output=True, text=True, timeout=60)


def test_cli_switch_needs_secondary_yes():
    """Refused by the option checks: neither file is opened (their names would be the complaint otherwise)."""
    for extra in ([], ["--secondary", "no"], ["-q", "3000"]):
        p = _cli("--secondary-strips", *extra)
        assert p.returncode != 0
        assert "--secondary-strips needs --secondary yes" in p.stderr and "nonexistent" not in p.stderr


def test_cli_switch_lifts_the_refusal_of_long_queries():
    p = _cli("-q", "3000", "--secondary", "yes", "--secondary-strips")
    assert p.returncode != 0 and "supports -q up to 2048" not in p.stderr
    assert "nonexistent" in p.stderr  # past the option checks: the first thing missing is a file
    assert "--secondary-strips" in subprocess.run([EXE, "dtw", "--help"], capture_output=True, text=True, timeout=60).stdout


def test_option_is_named_in_the_header():
    header = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    assert '"secondary_strips"' in header
    assert "the row strips keep no list" not in header


def _build(tmp, sanitize):
    exe = str(tmp / ("long_plan_sec_san" if sanitize else "long_plan_sec"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "c", "long_plan_sec.cpp")]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    """[lines of the plain build, lines of the sanitizer build or None]"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("long_plan_sec")
    exe, build = _build(tmp, False)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    san, build = _build(tmp, True)
    if build.returncode != 0 and any(m in build.stderr for m in (b"libasan", b"libubsan", b"-lasan", b"-lubsan", b"unrecognized command-line option", b"unsupported option")):
        san = None  # (the plain build went through: only a toolchain that says its sanitizer runtime is missing counts as without)
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


def test_both_builds_print_the_same_lines(outputs):
    if outputs[1] is None:
        pytest.skip("toolchain without sanitizer runtimes")
    assert outputs[0] == outputs[1]


def test_plan_sizes_and_offsets(outputs):
    lines = outputs[0]
    assert not [ln for ln in lines if ln.startswith("FAIL")] and lines[-1] == "done 0"
    got = {ln.split()[1]: {kv.split("=")[0]: int(kv.split("=")[1]) for kv in ln.split()[2:]} for ln in lines if ln.startswith("sec ")}
    assert sorted(got) == ["mixed", "none", "one", "one_per_group", "three_groups"]
    assert got["none"]["list_words"] == 0 and got["none"]["rank_words"] == 0
    for name, n_long, n_jobs in (("one", 1, 2), ("mixed", 3, 2), ("three_groups", 6, 4), ("one_per_group", 3, 4)):
        g = got[name]
        assert (g["n_long"], g["n_jobs"]) == (n_long, n_jobs)
        assert g["list_words"] == 15 * n_long * n_jobs  # 5 x (score bits, end, job) per (read, job) pair
        assert g["rank_words"] == 25 * n_long and g["traced"] == 15 * n_long and g["traced_words"] == 10 * n_long
    # the budget of tests/test_secondary_strips_gpu.py::test_groups_on_two_scratch_sets: two reads per set, three groups
    assert (got["three_groups"]["group"], got["three_groups"]["n_groups"], got["three_groups"]["two_sets"]) == (2, 3, 1)
    assert (got["one_per_group"]["group"], got["one_per_group"]["n_groups"]) == (1, 3)
