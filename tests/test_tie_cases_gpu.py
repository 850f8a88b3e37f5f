"""The crafted ties of tests/tie_cases.py through the batch path: align_db against oracle.align_batch, rows compared with
assert_rows_equal (scores and score2 bit for bit, mapq too), under every entry of MODES; the same reads once, five times and 300
times in one batch at the defaults (other widenings, chunk counts and segments); the column-segment cases with their segments
pinned; the top-5 cases with secondary = 4 (and secondary_strips = 1 for the strip lengths) against tests/secondary_oracle.py; and
every call twice on one context, byte for byte.  tests/test_tie_cases_cpu.py shows what each case claims, without a GPU."""
import numpy as np
import pytest

import sigfish_amd as S
from tests import tie_cases as T
from tests.secondary_oracle import secondary_rows
from tests.test_gpu_parity import MODES, _aligner, assert_rows_equal
from tests.test_secondary_gpu import assert_sec_equal

pytestmark = pytest.mark.gpu

_want, _want_sec = {}, {}


def _model(case):
    names = [f"c{i}" for i in range(len(case.lens))]
    return S.RefModel(names, [n + 5 for n in case.lens], case.lens, case.offs, case.forward, case.reverse)


def _oref(O, case):
    return O.RefSynth([f"c{i}" for i in range(len(case.lens))], [n + 5 for n in case.lens], case.lens, case.offs, case.forward, case.reverse)


def expected(O, case):
    """the oracle's rows of the case's reads, computed once and shared"""
    if case.name not in _want:
        _want[case.name] = O.align_batch(case.q, case.q_off, _oref(O, case), case.flag, threads=8)
        _want[case.name].setflags(write=False)
    return _want[case.name]


def assert_claim(case, rows):
    """what the case claims of every read, on the rows themselves (the oracle's rows say the same: tests/test_tie_cases_cpu.py)"""
    c, s, col = case.winner
    assert (rows["rid"] == c).all() and (rows["strand"] == ord(s)).all(), (case.name, rows[:4])
    assert ((rows["pos_end"] if s == "+" else case.lens[c] - rows["pos_st"]) == col + (case.offs[c] if s == "+" else -case.offs[c])).all(), (case.name, rows[:4])
    if case.top_tie:
        assert np.array_equal(rows["score"].view(np.uint32), rows["score2"].view(np.uint32)), (case.name, rows[:4])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", T.NAMES)
def test_every_case_under_every_mode(oracle, name, mode):
    case = T.build(name)
    want = expected(oracle, case)
    with _aligner(_model(case), case.flag, mode) as al:
        got = al.align_db(case.q, case.q_off)
        again = al.align_db(case.q, case.q_off)  # buffers reused
    assert_rows_equal(got, want)
    assert_claim(case, got)
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("reps", T.REPS)
@pytest.mark.parametrize("name", T.NAMES)
def test_batch_sizes_at_defaults(oracle, name, reps):
    """every copy of a read gives the same row, the oracle's, whatever the planner makes of the batch size"""
    case = T.build(name)
    want = expected(oracle, case)
    q, q_off = T.repeated(case, reps)
    with S.Aligner(_model(case), case.flag) as al:
        got = al.align_db(q, q_off)
        again = al.align_db(q, q_off)
        prof = al.profile()
    n = len(want)
    for k in range(reps):
        assert got[k * n:(k + 1) * n].tobytes() == got[:n].tobytes(), (name, k)
    assert_rows_equal(got[:n], want)
    assert_claim(case, got)
    assert again.tobytes() == got.tobytes()
    if name in T.SPLIT and reps in case.real_split:  # the job list was really cut: fewer chunks than jobs (what the CPU file computes)
        assert 1 < prof["n_chunks"] < len(T.job_lens(case)), prof["n_chunks"]
    if name in T.SEGMENTED and reps == 1:
        assert prof["n_segments"] >= 3 and prof["segment_reruns"] == 0, prof


@pytest.mark.parametrize("warm", [4, 1])
@pytest.mark.parametrize("name", T.SEGMENTED)
def test_column_segments_pinned(oracle, name, warm):
    """lane_widening 4 with column_segments 2 / 3: the twins lie on either side of a hand-over (with one warm-up window too)"""
    case = T.build(name)
    want = expected(oracle, case)
    with S.Aligner(_model(case), case.flag) as al:
        for k, v in case.options.items():
            al.set_option(k, v)
        al.set_option("segment_warm_windows", warm)
        got = al.align_db(case.q, case.q_off)
        prof = al.profile()
        again = al.align_db(case.q, case.q_off)
    if warm == 4:
        assert prof["n_segments"] == case.options["column_segments"] and prof["segment_reruns"] == 0, prof
    else:  # a warm-up of one window may not verify at the hand-over: the batch is then walked again unsegmented, same rows
        assert prof["n_segments"] == case.options["column_segments"] or prof["segment_reruns"] == 1, prof
    assert_rows_equal(got, want)
    assert_claim(case, got)
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("reps", [1, 5])
@pytest.mark.parametrize("name", T.MANY)
def test_secondaries_of_the_many_tie_cases(oracle, name, reps):
    """secondary = 4: ranks 2..5 of the candidate list, the fifth the later of two tied candidates (row strips: secondary_strips)"""
    case = T.build(name)
    want = expected(oracle, case)
    if name not in _want_sec:
        _want_sec[name] = secondary_rows(oracle, case.q, case.q_off, _oref(oracle, case), case.flag)
    want_sec = _want_sec[name]
    q, q_off = T.repeated(case, reps)
    with S.Aligner(_model(case), case.flag) as al:
        al.set_secondary(4)
        if case.qlen > 2048:
            al.set_option("secondary_strips", 1)
        prim = al.align_db(q, q_off)
        sec = al.secondary_rows()
        prim2 = al.align_db(q, q_off)
        sec2 = al.secondary_rows()
    n = len(want)
    assert_rows_equal(prim[:n], want)
    assert_sec_equal(sec[:n], want_sec)
    for k in range(reps):
        assert prim[k * n:(k + 1) * n].tobytes() == prim[:n].tobytes() and sec[k * n:(k + 1) * n].tobytes() == sec[:n].tobytes(), (name, k)
    assert prim2.tobytes() == prim.tobytes() and sec2.tobytes() == sec.tobytes()
    for k, (c, s, col) in enumerate(case.top5[1:]):  # the claimed candidates, in the claimed order
        r = sec[:n, k]
        assert (r["valid"] == 1).all() and (r["rid"] == c).all() and (r["strand"] == ord(s)).all(), (name, k, r)
        assert ((r["pos_end"] if s == "+" else case.lens[c] - r["pos_st"]) == col + (case.offs[c] if s == "+" else -case.offs[c])).all(), (name, k, r)
