"""Resweep sessions (SFA_SESSION_RESWEEP) without a GPU: the flag is declared, sfa_session_bytes takes it and nothing else new,
the command line still refuses what a session cannot do before anything touches a device, and the Python scheduler does not
depend on the flag."""
import os
import re
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib, realtime
from tests.realtime_util import BIN, write_model
from tests.test_realtime_cpu import CHUNK, StubSession, script_for
from tests.util import GOLD, ROOT


@pytest.mark.parametrize("cols,slots", [(1, 1), (59796, 512), (700, 3), (2 ** 31 + 5, 7)])
def test_session_bytes_takes_the_flag(cols, slots):
    L = _lib.load()
    # the carried rows are still needed (a window beyond 2048 events runs as consecutive pieces): the same numbers
    assert L.sfa_session_bytes(cols, slots, 4) == L.sfa_session_bytes(cols, slots, 0) == slots * cols * 8
    assert L.sfa_session_bytes(cols, slots, 5) == L.sfa_session_bytes(cols, slots, 1) == slots * cols * 4
    assert S.session_bytes(cols, slots, resweep=True) == slots * cols * 8
    assert S.session_bytes(cols, slots, starts=False, resweep=True) == slots * cols * 4


@pytest.mark.parametrize("flags", [2, 6, 8])
def test_session_bytes_refuses_unknown_bits(flags):
    assert _lib.load().sfa_session_bytes(100, 4, flags) < 0


def test_names():
    assert S.SESSION_RESWEEP == 4
    hdr = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    assert re.search(r"#define\s+SFA_SESSION_RESWEEP\s+0x4\b", hdr)
    assert not re.search(r"#define\s+SFA_SESSION_\w+\s+0x2\b", hdr)  # 0x2 stays unassigned


REFUSED = [(["--rna"], "--rna needs --invert"), (["--resweep", "--dtw-std"], "--dtw-std is not available"),
           (["--rna", "--resweep", "--dtw-std"], "--dtw-std is not available"), (["--resweep", "--from-end"], "--from-end is not available"),
           (["--resweep", "--sam"], "--sam is not available"), (["--rna", "--resweep", "-p", "-1"], "-p must be >= 0"),
           (["--resweep", "--invert"], "Inversion is only available for RNA.")]


@pytest.mark.parametrize("extra,msg", REFUSED, ids=["_".join(e).replace("--", "") for e, _ in REFUSED])
def test_refused_options_exit_before_any_device_call(extra, msg, tmp_path):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    rna = "--rna" in extra
    model = write_model(tmp_path / "syn.model", 5 if rna else 6)
    files = [os.path.join(GOLD, "data", "rnasequin_sequences_2.4.fa" if rna else "nCoV-2019.reference.fasta"),
             os.path.join(GOLD, "data", "sequin_rna.blow5" if rna else "sp1_dna.blow5")]
    r = subprocess.run([BIN, "realtime", "--kmer-model", model, *extra, *files], capture_output=True, timeout=60)
    err = r.stderr.decode()
    assert r.returncode not in (0, None) and r.returncode > 0 and r.stdout == b"", (r.returncode, err)
    assert err.count("[sigfish-amd] ERROR:") == 1 and msg in err, err
    assert "accelerator" not in err and "hip" not in err.lower(), err


def test_help_lists_the_flag():
    r = subprocess.run([BIN, "realtime", "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and "--resweep" in r.stdout.decode()


def test_schedule_does_not_depend_on_the_flag():
    """the same stub statuses with and without resweep: the same trace, the same decisions"""
    for channels in (1, 3, 8):
        for n_reads in (0, 1, 7, 20):
            runs = []
            for resweep in (False, True):
                reads = ((f"read{i}", dict(digitisation=1.0, offset=float(i), range=1.0), np.zeros(script_for(i)[0], np.int16)) for i in range(n_reads))
                trace = []
                out = [(t, c, i, why) for t, c, i, _, _, _, why in
                       realtime.replay(None, reads, channels, CHUNK, 0, 25, 25, 30, 20, session=StubSession(), trace=trace, resweep=resweep)]
                runs.append((trace, out))
            assert runs[0] == runs[1], (channels, n_reads)
            assert n_reads == 0 or runs[0][0]
    sch = realtime.Schedule(2, CHUNK, resweep=True)
    assert sch.resweep is True and realtime.Schedule(2, CHUNK).resweep is False
