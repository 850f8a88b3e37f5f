"""The entry selection of a session's query calls as the library ships it (sigfish_amd/csrc/session_query.hpp: which entries of
sfa_session_classes / sfa_session_group_bests / sfa_session_open_classes launch, the block-count refusal, the scatter index),
without a GPU: the stand-alone program tests/c/session_query.cpp, built from that header alone with -Wall -Werror and once more
under ASan + UBSan; both builds must print the same lines, and the lines must be what the rule says."""
import os
import shutil
import subprocess

import pytest

from tests.util import ROOT

INT32_MAX = 2**31 - 1


def _build(tmp, sanitize):
    exe = str(tmp / ("session_query_san" if sanitize else "session_query"))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + (["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else [])
    cmd += ["-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "session_query.cpp")]
    return exe, subprocess.run(cmd, capture_output=True, timeout=600)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """[plain build, sanitizer build or None]: every request goes through all of them, and their answers must be the same lines"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("session_query")
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
    assert _ask(programs[1:], "live 2 2\n0 5\n1 5\n1 0\nfit 1 1\n") == ["live 1 1", "slots 0", "out -1 0", "fit 1"]


# name -> (per slot (poisoned, events held), the slots of the call)
CALLS = {
    "n = 0": ([(0, 9), (0, 0)], []),
    "all poisoned": ([(1, 9), (1, 30), (1, 0)], [2, 0, 1]),
    "all empty": ([(0, 0), (0, 0), (0, 0), (0, 0)], [3, 1]),
    "mixed": ([(0, 30), (0, 0), (1, 12), (0, 1), (1, 0), (0, 7)], [5, 2, 0, 1, 4, 3]),
    "caller order, descending slots": ([(0, 4), (0, 5), (0, 6), (0, 7)], [3, 2, 1, 0]),
    "one live entry behind the others": ([(1, 3), (0, 0), (0, 2)], [0, 1, 2]),
}


def _ask_live(programs, slots, call):
    text = f"live {len(slots)} {len(call)}\n" + "".join(f"{p} {n}\n" for p, n in slots) + " ".join(map(str, call)) + "\n"
    lines = _ask(programs, text)
    assert [ln.split()[0] for ln in lines] == ["live", "slots", "out"]
    live, up, out = ([int(x) for x in ln.split()[1:]] for ln in lines)
    assert live[0] == len(live) - 1
    return live[1:], up, out


@pytest.mark.parametrize("name", list(CALLS))
def test_entries_that_launch_and_where_their_records_go(programs, name):
    slots, call = CALLS[name]
    live, up, out = _ask_live(programs, slots, call)
    want = [i for i, sl in enumerate(call) if not slots[sl][0] and slots[sl][1] > 0]  # not poisoned, and it has events
    assert live == want and live == sorted(live)                # in the caller's order
    assert up == [call[i] for i in want]                        # launched entry k is the slot of the caller's entry live[k]
    assert len(out) == len(call)
    for i, sl in enumerate(call):                               # every other entry keeps its "none" record
        assert out[i] == (1000 * want.index(i) + sl if i in want else -1), (name, i)
    if name in ("n = 0", "all poisoned", "all empty"):
        assert live == [] and all(r == -1 for r in out)
    if name == "mixed":
        assert live == [0, 2, 5] and up == [5, 0, 3] and out == [5, -1, 1000, -1, -1, 2003]
    if name == "caller order, descending slots":
        assert up == [3, 2, 1, 0] and out == [3, 1002, 2001, 3000]


FITS = [(0, 1), (0, INT32_MAX), (1, 1), (1, INT32_MAX), (INT32_MAX, 1), (2, 2**30), (2**16, 2**15), (2**15, 2**16), (3, 715827882), (3, 715827883),
        (INT32_MAX, 2), (INT32_MAX, INT32_MAX), (46341, 46341), (46340, 46341)]


def test_block_count_refusal_at_and_above_int32_max(programs):
    lines = _ask(programs, "".join(f"fit {m} {parts}\n" for m, parts in FITS))
    assert lines == [f"fit {int(m * parts <= INT32_MAX)}" for m, parts in FITS]
    at = dict(zip(FITS, lines))
    assert at[(1, INT32_MAX)] == at[(INT32_MAX, 1)] == "fit 1"                     # exactly at the limit (2^31 - 1 is prime)
    assert at[(2, 2**30)] == at[(2**16, 2**15)] == "fit 0"                         # one above it
    assert at[(3, 715827882)] == "fit 1" and at[(3, 715827883)] == "fit 0"         # 2^31 - 2 and 2^31 + 1
