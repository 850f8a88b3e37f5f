"""Alignment sessions without a GPU: the symbols are declared and exported, sfa_session_bytes is host arithmetic, and the
Python names exist."""
import ctypes as C
import os
import re

import pytest

import sigfish_amd as S
from sigfish_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ["sfa_session_create", "sfa_session_extend", "sfa_session_reset", "sfa_session_lengths", "sfa_session_destroy",
        "sfa_session_bytes", "sfa_session_row"]


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    L = _lib.load()
    for s in SYMS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in _lib.SYMBOLS
        assert getattr(L, s) is not None
    assert re.search(r"#define\s+SFA_SESSION_NO_START\s+0x1\b", hdr)
    assert "typedef struct sfa_session sfa_session_t;" in hdr


@pytest.mark.parametrize("cols,slots", [(1, 1), (59796, 512), (700, 3), (2 ** 31 + 5, 7)])
def test_session_bytes_is_rows_times_columns(cols, slots):
    L = _lib.load()
    # one carried row per slot, updated in place: a cost (and a start column) per reference column
    assert L.sfa_session_bytes(cols, slots, 0) == slots * cols * 8
    assert L.sfa_session_bytes(cols, slots, 1) == slots * cols * 4
    assert S.session_bytes(cols, slots) == slots * cols * 8
    assert S.session_bytes(cols, slots, starts=False) == slots * cols * 4


def test_issue_figure():
    """both nCoV strands with start columns: 478 KB per read, 245 MB for 512 channels"""
    cols = 2 * 29898
    assert S.session_bytes(cols, 1) == 478368
    assert S.session_bytes(cols, 512) == 244924416


@pytest.mark.parametrize("cols,slots,flags", [(0, 4, 0), (-5, 4, 0), (100, 0, 0), (100, -1, 1), (100, 4, 2), (100, 4, 0x80000001),
                                              (2 ** 62, 8, 0)])
def test_session_bytes_refuses(cols, slots, flags):
    assert _lib.load().sfa_session_bytes(cols, slots, flags) < 0
    if flags in (0, 1):
        with pytest.raises(S.SfaError):
            S.session_bytes(cols, slots, starts=flags == 0)


def test_python_names():
    assert callable(S.Aligner.session)
    for name in ("extend", "reset", "lengths", "row", "close", "__enter__", "__exit__"):
        assert callable(getattr(S.Session, name)), name
    assert callable(S.session_bytes)
    assert S.SESSION_NO_START == 1


def test_null_arguments_are_einval():
    L = _lib.load()
    h = C.c_void_p()
    assert L.sfa_session_create(None, 4, 0, C.byref(h)) == -1
    assert L.sfa_session_extend(None, None, None, None, 1, None) == -1
    assert L.sfa_session_reset(None, None, 0) == -1
    assert L.sfa_session_lengths(None, None, 0, None) == -1
    assert L.sfa_session_row(None, 0, 0, ord("+"), None, None) == -1
    L.sfa_session_destroy(None)
