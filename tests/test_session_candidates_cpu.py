"""Session candidates without a GPU: the two entry points are declared and exported and refuse a NULL handle, `sigfish-amd realtime`
refuses a --candidates outside 1..4 before anything touches a file or a device and names the option in its help, and the Python
twin formats a candidate line as the tp:A:S line of sfa_paf_row_ex with the primary's three tags."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib, realtime
from tests.realtime_util import BIN, write_model
from tests.util import GOLD, ROOT

NAMES = ("sfa_session_candidates_config", "sfa_session_candidates")


def test_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    L = _lib.load()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name


def test_null_handle():
    L = _lib.load()
    assert L.sfa_session_candidates_config(None, 2) == -1
    assert L.sfa_session_candidates(None, None, 0, None) == -1


@pytest.mark.parametrize("value", ["0", "5", "x", "-1", "2x", ""])
def test_candidates_out_of_range_exit_before_any_device_call(value, tmp_path):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    model = write_model(tmp_path / "syn.model", 6)
    # (files that do not exist: opening one would be the error reported instead)
    r = subprocess.run([BIN, "realtime", "--kmer-model", model, "--candidates", value, str(tmp_path / "no.fa"), str(tmp_path / "no.blow5")], capture_output=True, timeout=60)
    err = r.stderr.decode()
    assert r.returncode not in (0, None) and r.returncode > 0 and r.stdout == b"", (r.returncode, err)
    assert err.count("[sigfish-amd] ERROR:") == 1 and "--candidates should be 1..4" in err, err
    assert "accelerator" not in err and "hip" not in err.lower() and "no.fa" not in err and "no.blow5" not in err, err


def test_secondary_refusal_names_candidates(tmp_path):
    model = write_model(tmp_path / "syn.model", 6)
    files = [os.path.join(GOLD, "data", "nCoV-2019.reference.fasta"), os.path.join(GOLD, "data", "sp1_dna.blow5")]
    r = subprocess.run([BIN, "realtime", "--kmer-model", model, "--secondary", "yes", "--candidates", "4", *files], capture_output=True, timeout=60)
    err = r.stderr.decode()
    assert r.returncode > 0 and r.stdout == b"" and err.count("[sigfish-amd] ERROR:") == 1, err
    assert "--secondary yes is not available" in err and "--candidates" in err, err


def test_help_names_candidates():
    r = subprocess.run([BIN, "realtime", "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and "--candidates" in r.stdout.decode()


def _row(rid, st, end, score, score2, strand, mapq, valid):
    r = np.zeros(1, S.RESULT_DTYPE)[0]
    r["rid"], r["pos_st"], r["pos_end"], r["score"], r["score2"], r["strand"], r["mapq"], r["valid"] = rid, st, end, score, score2, ord(strand), mapq, valid
    return r


def test_python_twin_formats_candidate_lines():
    names, seq_lengths = ["c0", "c1"], [905, 310]
    prim = _row(0, 100, 169, 31.25, 33.5, "+", 7, 1)
    cand = np.zeros(4, S.RESULT_DTYPE)
    cand[0] = _row(1, 40, 111, 33.5, 36.0, "-", 0, 1)
    cand[1] = _row(-1, -1, -1, np.inf, np.inf, "+", 0, 0)  # not valid: no line, and the ranks behind it are still looked at
    cand[2] = _row(0, 300, 372, 36.0, np.inf, "+", 0, 1)
    info = np.zeros(1, S.SESSION_RAW_INFO_DTYPE)[0]
    info["q_events"], info["n_samples"] = 70, 2400
    span, why, n_samples = (123, 2345), "E", 9000
    text = realtime.format_candidates("read7", n_samples, names, seq_lengths, prim, cand, info, span, why)
    want = ""
    for k in (0, 2):
        rid = int(cand[k]["rid"])
        base = S.paf_row(cand[k], "read7", names[rid], span[0], span[1], 69, n_samples, seq_lengths[rid], tp="S")
        assert "tp:A:S" in base and base.endswith("\n")
        want += base[:-1] + "\tne:i:70\tns:i:2400\tdc:A:E\n"
    assert text == want and text.count("\n") == 2
    # the same tags as the primary line, which comes first and stays as it was
    line = realtime.format_line("read7", n_samples, names, seq_lengths, prim, info, span, why)
    assert "tp:A:P" in line and line.split("\t")[-3:] == text.splitlines(keepends=True)[0].split("\t")[-3:]
    # a decision without a line has no candidate lines either
    assert realtime.format_candidates("read7", n_samples, names, seq_lengths, _row(-1, -1, -1, np.inf, np.inf, "+", 0, 0), cand, info, span, why) == ""
