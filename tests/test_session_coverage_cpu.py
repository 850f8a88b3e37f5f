"""The host rules of a session's coverage cap without a GPU: the stand-alone program tests/c/coverage_rules.cpp, built from
sigfish_amd/csrc/coverage_rules.hpp alone with -Wall -Werror and once more under ASan + UBSan, against the numpy model of
tests/coverage_model.py -- depth tracks, live mask, live count, lowest column of either class -- on contigs whose lengths are no
multiples of 32 (a mask word straddles two jobs), with non-zero offsets, for DNA (two strands) and RNA (one); the model's open
pieces given back as a target list reproduce the live mask; the list errors; the four new symbols of the C ABI; the refusals of
`realtime --depth-cap` and replay(depth_cap=), which come before any file, session or device is opened."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib, realtime
from tests import coverage_model as M
from tests.realtime_util import BIN, write_model
from tests.util import GOLD, ROOT


def _build(tmp, sanitize):
    exe = str(tmp / ("coverage_rules_san" if sanitize else "coverage_rules"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "coverage_rules.cpp")]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """[plain build, sanitizer build or None]: every request goes through all of them, and their answers must be the same lines"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("coverage_rules")
    exe, build = _build(tmp, False)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    san, build = _build(tmp, True)
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


def _request(strands, lens, offs, cap, targets, intervals):
    lst = lambda t: f"{len(t)} " + " ".join(f"{c} {b} {e}" for c, b, e in t)
    return f"live {strands} {len(lens)} " + " ".join(f"{n} {o}" for n, o in zip(lens, offs)) + f" {cap} {lst(targets)} {lst(intervals)}\n"


def test_selftest_plain_and_under_sanitizers(programs):
    line = _ask(programs, "selftest\n")[-1].split()
    assert line[:2] == ["selftest", "ok"] and int(line[2]) > 50


def test_the_program_runs_under_sanitizers(programs):
    if programs[1] is None:
        pytest.skip("toolchain without sanitizer runtimes")
    got = _ask(programs[1:], _request(2, [5], [0], 1, [(0, 0, 6)], [(0, 2, 3)]))
    # '+' columns 0..4 are coordinates 0..4, '-' columns 5..9 are coordinates 5..1: coordinate 2 closes column 2 and column 8
    assert got == ["live 8 0 2 000002fb", "depth 0 0 0 1 0 0 0", "base 000003ff"]


# ---- the header against the numpy model ----
LENS = [1, 31, 33, 45, 70]   # none a multiple of 32: the words of the mask straddle jobs
OFFS = [0, 7, 100, 3, 1000]
whole = lambda r: (r, OFFS[r], OFFS[r] + LENS[r] + 1)
CASES = {
    "nothing added": (2, [whole(r) for r in range(5)], []),
    "one-base intervals": (1, [whole(r) for r in range(5)], [(4, 1000, 1001), (4, 1070, 1071), (4, 1031, 1032), (4, 1032, 1033), (1, 7, 8), (1, 38, 39), (0, 0, 1), (0, 1, 2)]),
    "whole contigs": (1, [whole(r) for r in range(5)], [whole(3), whole(0)]),
    "cap - 1 and cap": (3, [whole(2), whole(4)], [(2, 110, 120)] * 2 + [(2, 115, 125)] + [(4, 1000, 1071)] * 3 + [(4, 1010, 1011)]),
    "below the offset": (1, [whole(r) for r in range(5)], [(2, 0, 101), (4, 5, 1000), (3, 0, 3)]),
    "off-target depth": (1, [(3, 10, 20), (4, 1060, 1071)], [(3, 0, 12), (3, 30, 49), (4, 1000, 1065), (1, 7, 39)]),
    "overlapping, two contigs interleaved": (2, [whole(1), whole(3), (4, 1005, 1050)], [(3, 5, 30), (1, 8, 20), (3, 20, 40), (1, 10, 39), (3, 5, 30), (4, 1000, 1071), (1, 8, 20)]),
}


@pytest.mark.parametrize("strands", [1, 2], ids=["rna_one_strand", "dna_two_strands"])
@pytest.mark.parametrize("name", list(CASES))
def test_live_mask_equals_the_models(programs, name, strands):
    cap, targets, intervals = CASES[name]
    lines = _ask(programs, _request(strands, LENS, OFFS, cap, targets, intervals))
    model = M.Coverage(LENS, OFFS, strands, cap)
    model.add(intervals)
    live, base = model.live_mask(targets), model.base_mask(targets)
    tag, n_live, first_on, first_off, *words = lines[0].split()
    assert tag == "live" and int(n_live) == int(live.sum()) == model.open_columns(targets)
    assert [int(w, 16) for w in words] == M.words_of(live)
    assert int(first_on) == (int(np.flatnonzero(live)[0]) if live.any() else -1)
    assert int(first_off) == (int(np.flatnonzero(~live)[0]) if not live.all() else -1)
    for r in range(len(LENS)):
        assert lines[1 + r].split() == ["depth", str(r)] + [str(int(v)) for v in model.depth[r]], (name, r)
    assert [int(w, 16) for w in lines[-1].split()[1:]] == M.words_of(base)
    if name == "nothing added":
        assert np.array_equal(live, base)
    if name == "whole contigs":  # contigs 0 and 3 are closed on every strand, the others untouched
        assert int(n_live) == strands * (31 + 33 + 70) and not live[:strands].any()
    if name == "below the offset":  # of the three intervals only coordinate 100 of contig 2 is one a row reports: '+' column 0 alone
        assert model.depth[2][0] == 1 and model.depth[2][1:].sum() == 0 and model.depth[4].sum() == 0 and model.depth[3].sum() == 0
        assert int(live.sum()) == int(base.sum()) - 1
    if name == "cap - 1 and cap":  # depth 2 stays open under cap 3, depth 3 is closed
        assert set(model.depth[2][10:25]) == {2, 3, 1} and int(live.sum()) == strands * 33 - strands * 5
    # the model's open pieces as ONE target list give the live mask back: the rule closes a coordinate on both strands at once, so the
    # open set is a set of coordinates -- through the header's own target_mask (nothing added)
    again = _ask(programs, _request(strands, LENS, OFFS, 1, model.open_list(targets), []))
    assert again[0].split()[1:] == lines[0].split()[1:] and again[-1].split()[1:] == lines[0].split()[4:]
    pieces = model.open_pieces(targets)
    if strands == 2:  # where both strands report a coordinate they agree on it
        both = lambda runs, r: {x for c, b, e in runs if c == r for x in range(b, e) if OFFS[r] < x < OFFS[r] + LENS[r]}
        for r in range(len(LENS)):
            assert both(pieces["+"], r) == both(pieces["-"], r), (name, r)


REFUSALS = [((-1, 0, 1), "contig"), ((5, 0, 1), "contig"), ((2, -1, 4), "negative"), ((2, 4, 4), "empty"), ((2, 105, 104), "empty"), ((2, 100, 135), "beyond")]


@pytest.mark.parametrize("iv,word", REFUSALS)
def test_list_errors_are_a_target_lists(programs, iv, word):
    line = _ask(programs, _request(2, LENS, OFFS, 1, [whole(2)], [(2, 100, 134), iv]))[0]
    assert line.startswith("refused target 1:") and word in line
    as_target = _ask(programs, _request(2, LENS, OFFS, 1, [whole(2), iv], []))[0]
    assert as_target == line  # the same function, the same words


# ---- the C ABI ----
NEW = ["sfa_session_coverage_config", "sfa_session_coverage_add", "sfa_session_coverage_depth", "sfa_session_coverage_bytes"]


def test_the_library_exports_the_four_functions():
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    for sym in NEW:
        assert sym in _lib.SYMBOLS and getattr(L, sym) is not None, sym
        assert f" {sym}(" in header, sym


def test_coverage_bytes_is_host_arithmetic():
    rng = np.random.default_rng(5)
    lens = [31, 33, 70]
    fw = [rng.normal(size=n).astype(np.float32) for n in lens]
    dna = S.RefModel(["a", "b", "c"], [n + 5 for n in lens], lens, [0, 7, 100], fw, [x.copy() for x in fw])
    rna = S.RefModel(["a", "b", "c"], [n + 5 for n in lens], lens, [0, 7, 100], fw, None)
    words = lambda cols: (cols + 31) // 32 + 1
    assert S.session_coverage_bytes(dna, 0) == 4 * (sum(lens) + 3) + 4 * words(2 * sum(lens))
    assert S.session_coverage_bytes(rna, S.RNA | S.INV) == 4 * (sum(lens) + 3) + 4 * words(sum(lens))


# ---- the front ends: every refusal before any file, session or device ----
def test_replay_refuses_bad_depth_caps_before_any_session():
    class NoAligner:
        def session(self, *a, **kw):
            raise AssertionError("a session was opened")

    class NoStarts:
        starts = False

        def __getattr__(self, name):
            raise AssertionError("the session was used")

    t = [(0, 0, 10)]
    groups = (np.zeros(1, S.GROUP_TARGET_DTYPE), ["g"])
    ok = dict(targets=t, mode=S.ENRICH, margin=0.1)
    for kw, word in ((dict(ok, depth_cap=0), "integer 1"), (dict(ok, depth_cap=-3), "integer 1"), (dict(ok, depth_cap=1.5), "integer 1"), (dict(ok, depth_cap=True), "integer 1"),
                     (dict(ok, depth_cap=(1 << 30) + 1), "integer 1"), (dict(depth_cap=2), "pass targets="), (dict(targets=t, margin=0.1, depth_cap=2), "pass targets="),
                     (dict(targets=t, mode=S.DEPLETE, margin=0.1, depth_cap=2), "not built"), (dict(targets=groups, by_name=True, mode=S.ENRICH, margin=0.1, depth_cap=2), "not built"),
                     (dict(targets=groups, by_name=True, quota=3, mode=S.ENRICH, margin=0.1, depth_cap=2), "not built"),
                     (dict(ok, depth_cap=2, session=NoStarts()), "start columns")):
        with pytest.raises(S.SfaError, match=word):
            list(realtime.replay(NoAligner(), [], 2, 100, 3, 25, 70, 30, 5, **kw))


BED = "nCoV.bed"
T_OK = ["--targets", BED, "--enrich", "--margin", "0.1"]
REFUSED = [(T_OK + ["--depth-cap", "0"], "--depth-cap should be an integer 1.."), (T_OK + ["--depth-cap", "-2"], "--depth-cap should be an integer 1.."),
           (T_OK + ["--depth-cap", "x"], "--depth-cap should be an integer 1.."), (T_OK + ["--depth-cap", "1073741825"], "--depth-cap should be an integer 1.."),
           (["--depth-cap", "3"], "pass --targets FILE.bed --enrich"), (["--targets", BED, "--deplete", "--margin", "0.1", "--depth-cap", "3"], "--deplete is not built"),
           (T_OK + ["--by-name", "--depth-cap", "3"], "it is not built"), (T_OK + ["--by-name", "--quota", "2", "--depth-cap", "3"], "it is not built")]


@pytest.mark.parametrize("extra,msg", REFUSED, ids=["_".join(e).replace("--", "") for e, _ in REFUSED])
def test_binary_refuses_depth_cap_options_before_any_file_or_device(extra, msg, tmp_path):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    model = write_model(tmp_path / "syn.model", 6)
    # (the BED file and the reads do not exist: a refusal that came after opening either would name them)
    r = subprocess.run([BIN, "realtime", "--kmer-model", model, *extra, os.path.join(GOLD, "data", "nCoV-2019.reference.fasta"), str(tmp_path / "no_such.blow5")],
                       capture_output=True, timeout=60)
    err = r.stderr.decode()
    assert r.returncode > 0 and r.stdout == b"", (r.returncode, err)
    assert err.count("[sigfish-amd] ERROR:") == 1 and msg in err, err
    assert "no_such" not in err and BED not in err.split("ERROR:")[1].replace("FILE.bed", "") and "accelerator" not in err, err
