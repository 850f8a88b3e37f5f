"""sfa_truth_class, sfa_truth_edge, sfa_truth_group, sfa_truth_verdict and sfa_truth_group_verdict (host only) against a numpy
restatement that counts shared bases one by one, on a few thousand seeded random target lists and reads; the symbols are bound and
declared."""
import ctypes as C
import os

import numpy as np

import sigfish_amd as S
from sigfish_amd import _lib
from tests.util import ROOT

SYMBOLS = ["sfa_truth_class", "sfa_truth_edge", "sfa_truth_group", "sfa_truth_verdict", "sfa_truth_group_verdict"]


def test_symbols_are_bound_and_declared():
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    for sym in SYMBOLS:
        assert sym in _lib.SYMBOLS and sym + "(" in header and getattr(L, sym) is not None


def numpy_truth(targets, n_groups, contig, begin, end):
    """(class, edge, group) of a read: every base of [begin, end) against every target"""
    bases = np.arange(begin, end)
    on, inside_one, group = False, False, n_groups
    for c, b, e, g in targets:
        if c != contig:
            continue
        shared = int(((bases >= b) & (bases < e)).sum())
        if shared:
            on, group = True, min(group, g)
        inside_one |= shared == len(bases)
    return ("T" if on else "O"), on and not inside_one, group


def test_class_edge_and_group_against_numpy():
    rng = np.random.default_rng(20240611)
    L = _lib.load()
    n_cases = seen_edge = seen_t = 0
    for _ in range(300):
        n_groups = int(rng.integers(1, 7))
        n = int(rng.integers(0, 8))
        targets = []
        for _ in range(n):
            b = int(rng.integers(0, 120))
            targets.append((int(rng.integers(0, 3)), b, b + int(rng.integers(1, 40)), int(rng.integers(0, n_groups))))
        plain = np.array([t[:3] for t in targets], np.int32).reshape(-1, 3).view(S.TARGET_DTYPE).reshape(-1) if n else np.zeros(0, S.TARGET_DTYPE)
        grouped = np.array(targets, np.int32).reshape(-1, 4).view(S.GROUP_TARGET_DTYPE).reshape(-1) if n else np.zeros(0, S.GROUP_TARGET_DTYPE)
        for _ in range(12):
            contig = int(rng.integers(-1, 4))
            b = int(rng.integers(0, 150))
            e = b + int(rng.integers(1, 60))
            if n and rng.integers(0, 3) == 0:  # exactly on a target's edges: touching, one base in, the target itself
                c, tb, te, _ = targets[int(rng.integers(0, n))]
                contig, (b, e) = c, [(max(tb - 5, 0), tb), (max(tb - 5, 0), tb + 1), (te - 1, te + 5), (te, te + 5), (tb, te)][int(rng.integers(0, 5))]
                if e <= b:
                    continue
            want = numpy_truth(targets, n_groups, contig, b, e)
            got = (S.truth_class(plain, contig, b, e), S.truth_edge(plain, contig, b, e), S.truth_group(grouped, n_groups, contig, b, e))
            assert got == want, (targets, n_groups, contig, b, e, got, want)
            # lists of tuples and the raw entry points say the same
            assert S.truth_class([t[:3] for t in targets], contig, b, e) == want[0] and S.truth_group(targets, n_groups, contig, b, e) == want[2]
            assert chr(L.sfa_truth_class(C.cast(plain.ctypes.data, C.POINTER(_lib.SfaTarget)), n, contig, b, e)) == want[0]
            n_cases += 1
            seen_edge += want[1]
            seen_t += want[0] == "T"
    assert n_cases > 3000 and seen_edge > 100 and 500 < seen_t < n_cases - 500
    assert S.truth_class([], 0, 1, 2) == "O" and not S.truth_edge([], 0, 1, 2) and S.truth_group([], 5, 0, 1, 2) == 5


def test_verdicts_against_their_tables():
    for d in ("T", "O", "N", None, "A", ""):
        for t in ("T", "O", "N", None, "x"):
            want = "N" if d not in ("T", "O") or t not in ("T", "O") else ("C" if d == t else "W")
            assert S.truth_verdict(d, t) == want, (d, t)
    rng = np.random.default_rng(5)
    for d, t in rng.integers(-3, 1025, (2000, 2)):
        want = "N" if d < 0 or t < 0 else ("C" if d == t else "W")
        assert S.truth_group_verdict(int(d), int(t)) == want
    assert S.truth_group_verdict(None, 3) == "N" and S.truth_group_verdict(3, None) == "N" and S.truth_group_verdict(1023, 1023) == "C"
