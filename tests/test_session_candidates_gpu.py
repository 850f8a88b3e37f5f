"""Session candidates on the GPU (sfa_session_candidates_config / sfa_session_candidates, sdtw_session.hpp): after EVERY call the
four candidates behind a slot's row equal the restatement of the reference's candidate list (tests/secondary_oracle.py) over the
slot's concatenated events -- every field, bit for bit, totals beyond 2048 events included -- and the rows of the session are the
bytes a twin session without candidates returns for the same chunks.  No tolerance anywhere."""
import numpy as np
import pytest

import sigfish_amd as S
from tests.secondary_oracle import secondary_rows, top5
from tests.test_session_gpu import _events, _oref, _small_ref
from tests.test_session_raw_gpu import SCALING, synth_signal
from tests.test_session_recal_gpu import RecalTwin
from tests.test_session_resweep_gpu import SweepTwin

pytestmark = pytest.mark.gpu

LENS = [300, 401]  # 401: no multiple of four, so the sweep's edge block runs
CTX = {"dna": 0, "rna_inv": S.RNA | S.INV}  # DNA: both strands, four jobs (the merge); RNA + INV: one strand
N_SLOTS = 12
FIELDS = ("rid", "pos_st", "pos_end", "strand", "mapq", "valid", "pad")


class Want:
    """The expected candidates of a slot: secondary_rows over its events so far, every distinct (events, count) once."""

    def __init__(self, O, ref, flag):
        self.O, self.ref, self.oref, self.flag, self.memo, self.lists = O, ref, _oref(O, ref), flag, {}, {}

    def cand(self, ev, n_sec=4):
        key = (ev.tobytes(), n_sec)
        if key not in self.memo:
            self.memo[key] = secondary_rows(self.O, ev, np.array([0, len(ev)], np.int64), self.oref, self.flag, n_sec)[0].copy()
        return self.memo[key]

    def aln(self, ev):
        key = ev.tobytes()
        if key not in self.lists:
            self.lists[key] = top5(self.O, ev, self.oref, self.flag)
        return self.lists[key]


_WANT = {}


def context(O, name, quant=True):
    """(ref, flag, Want) of a context, built once: quantised levels and events, so that ties occur"""
    if (name, quant) not in _WANT:
        flag = CTX[name]
        ref = _small_ref(np.random.default_rng(5 + len(name)), LENS, bool(flag & S.RNA), quant)
        _WANT[(name, quant)] = (ref, flag, Want(O, ref, flag))
    return _WANT[(name, quant)]


def assert_cand(got, want, starts, what):
    """every field of every row, valid or not; scores by their bits.  Without start columns the coordinate that needs one is -1"""
    w = want.copy()
    if not starts:
        v, plus = w["valid"] == 1, w["strand"] == ord("+")
        w["pos_st"][v & plus] = -1
        w["pos_end"][v & ~plus] = -1
    assert got.shape == w.shape, what
    for f in FIELDS:
        assert np.array_equal(got[f], w[f]), (what, f, np.argwhere(got[f] != w[f])[:8], got[f], w[f])
    for f in ("score", "score2"):
        assert np.array_equal(got[f].view(np.uint32), w[f].view(np.uint32)), (what, f, got[f], w[f])


def expected(want, sched, data, n_cand=4):
    """[call] -> (slots in order, [n, 4] expected candidates of EVERY slot of the schedule after that call, the event prefixes)"""
    slots = sorted(sched)
    used = {sl: 0 for sl in slots}
    out = []
    for c in range(max(len(v) for v in sched.values())):
        for sl in slots:
            if c < len(sched[sl]) and sched[sl][c] is not None:
                used[sl] += sched[sl][c]
        pre = [data[sl][:used[sl]] for sl in slots]
        out.append((slots, np.stack([want.cand(p, n_cand) for p in pre]), pre))
    return out


def coverage(want, exp):
    """what the oracle's lists of a schedule reach: equal scores inside a top 5, fewer than five finite candidates, two jobs"""
    seen = set()
    for _, _, pre in exp:
        for p in pre:
            if len(p) == 0:
                continue
            fin = [a for a in want.aln(p) if a[1] >= 0 and np.isfinite(a[0])]
            sc = [float(a[0]) for a in fin]
            if len(set(sc)) < len(sc):
                seen.add("tie")
            if len(fin) < 5:
                seen.add("short")
            if len({(a[1], a[4]) for a in fin}) >= 2:
                seen.add("two_jobs")
    return seen


def run(al, want, sched, data, starts, n_cand=4, exp=None):
    """the schedule on a session with candidates and on a twin without; after every call: rows byte-equal, score2 of the row is
    the best candidate's score, the candidates of every slot (named in the call or not) equal the oracle's"""
    exp = expected(want, sched, data, n_cand) if exp is None else exp
    used = {sl: 0 for sl in sched}
    with al.session(N_SLOTS, starts=starts, candidates=n_cand) as se, al.session(N_SLOTS, starts=starts) as twin:
        for c, (slots, want_c, _) in enumerate(exp):
            named = [sl for sl, v in sched.items() if c < len(v) and v[c] is not None]
            chunks = [data[sl][used[sl]:used[sl] + sched[sl][c]] for sl in named]
            ev_off = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
            ev = np.concatenate(chunks) if chunks else np.zeros(0, np.float32)
            rows, rows_twin = se.extend(named, ev, ev_off), twin.extend(named, ev, ev_off)
            for sl in named:
                used[sl] += sched[sl][c]
            assert rows.tobytes() == rows_twin.tobytes(), (c, named)
            mine = se.candidates(named)
            top = mine[:, 0]["valid"] == 1
            assert np.array_equal(rows["score2"][top].view(np.uint32), mine[:, 0]["score"][top].view(np.uint32)), (c, named)
            assert_cand(se.candidates(slots), want_c, starts, f"call {c}, named {named}")
        return se.lengths()


# a chunk length inside each of the six base shapes of kClassShapes, (4,16) (8,16) (16,16) (32,16) (32,32) (32,64): first as a
# slot's first chunk, then below its carried row; the short classes once more so that totals stay below the contigs (lists of
# five from several windows) and quantised scores tie
SHAPE_LENS = [40, 100, 200, 400, 700, 1500]
SHAPE_SCHED = {i: [n, n] for i, n in enumerate(SHAPE_LENS)}
SHAPE_SCHED.update({6: [7, 33, 64], 7: [None, 25, 65], 8: [129, None, 1], 9: [None, None, 257]})


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "nostart"])
@pytest.mark.parametrize("name", list(CTX))
def test_shapes_first_and_carried(oracle, name, starts):
    ref, flag, want = context(oracle, name)
    rng = np.random.default_rng(11)
    data = {sl: _events(rng, sum(x or 0 for x in v), True) for sl, v in SHAPE_SCHED.items()}
    exp = expected(want, SHAPE_SCHED, data)
    seen = coverage(want, exp)  # (about this test's own inputs, from the oracle's values, before anything is compared)
    assert seen >= ({"tie", "short", "two_jobs"} if name == "dna" else {"tie", "short"}), seen
    with S.Aligner(ref, flag) as al:
        full = run(al, want, SHAPE_SCHED, data, starts, exp=exp)
    assert full[5] == 3000 and full[4] == 1400


# chunks of different lengths that agree modulo R share a wave (MixedQuad): 61 & 57 & 33 & 1 and 64 & 60 & 56 & 52 on (4, 16),
# 256 & 144 on (16, 16), 128 & 72 on (8, 16), as first chunks and below carried rows; slots 8 .. 10 are left out of some calls
MIXED_SCHED = {0: [61, 64, 1], 1: [57, 60, 33], 2: [33, 56, 57], 3: [1, 52, 61], 4: [256, 144], 5: [144, 256], 6: [128, 72, 128], 7: [72, 128, 72],
               8: [50, None, None], 9: [None, 90, None], 10: [None, None, 30]}


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "nostart"])
def test_mixed_waves_and_slots_left_out(oracle, starts):
    ref, flag, want = context(oracle, "dna")
    rng = np.random.default_rng(12)
    data = {sl: _events(rng, sum(x or 0 for x in v), True) for sl, v in MIXED_SCHED.items()}
    with S.Aligner(ref, flag) as al:
        run(al, want, MIXED_SCHED, data, starts)


def test_short_lists(oracle):
    """totals above a fifth of the contigs: fewer than five windows exist on the one-strand context, the trailing ranks are
    valid = 0; and a session that keeps two candidates"""
    ref, flag, want = context(oracle, "rna_inv")
    rng = np.random.default_rng(13)
    sched = {0: [250], 1: [100, 110], 2: [301, 100], 3: [30, 40]}
    data = {sl: _events(rng, sum(v), True) for sl, v in sched.items()}
    exp = expected(want, sched, data)
    last = exp[-1][1]
    # (about this test's own inputs) 250 events: two windows per contig, four candidates; 401 events: one window per contig
    assert list(last[0]["valid"]) == [1, 1, 1, 0] and list(last[2]["valid"]) == [1, 0, 0, 0] and last[3]["valid"].all()
    with S.Aligner(ref, flag) as al:
        run(al, want, sched, data, True, exp=exp)
    ref, flag, want = context(oracle, "dna")
    exp2 = expected(want, sched, data, n_cand=2)
    assert all(not e[1]["valid"][:, 2:].any() and e[1]["valid"][:, :2].all() for e in exp2)
    with S.Aligner(ref, flag) as al:
        run(al, want, sched, data, True, n_cand=2, exp=exp2)


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "nostart"])
def test_long_chunk_and_growth_beyond_one_launch(oracle, starts):
    """a chunk of 2100 events runs as pieces of 2048 + 52 (the last piece's list counts), and a slot grows past 2048 events over
    several calls: the candidates stay valid -- a session has no SFA_MAX_QUERY cut-off"""
    ref, flag, want = context(oracle, "dna")
    rng = np.random.default_rng(14)
    sched = {0: [2100, 10], 1: [1000, 1000, 100], 2: [60, 2100], 3: [None, 70, 70]}
    data = {sl: _events(rng, sum(x or 0 for x in v), True) for sl, v in sched.items()}
    exp = expected(want, sched, data)
    assert exp[0][1][0]["valid"][:3].all() and exp[-1][1][1]["valid"][:3].all()  # (about this test's own inputs: four jobs, one window each)
    with S.Aligner(ref, flag) as al:
        full = run(al, want, sched, data, starts, exp=exp)
    assert list(full[:3]) == [2110, 2100, 2160]


def test_state(oracle):
    ref, flag, want = context(oracle, "dna")
    rng = np.random.default_rng(15)
    a, b = _events(rng, 120, True), _events(rng, 90, True)
    none = np.zeros(4, S.RESULT_DTYPE)
    none["rid"] = none["pos_st"] = none["pos_end"] = -1
    none["score"] = none["score2"] = np.inf
    empty = (np.zeros(0, np.float32), [0, 0])
    with S.Aligner(ref, flag) as al, al.session(4) as se:
        with pytest.raises(S.SfaError):  # nothing configured
            se.candidates([0])
        for n in (-1, 5):
            with pytest.raises(S.SfaError):
                se.configure_candidates(n)
        se.configure_candidates(4)
        for bad in ([4], [-1]):
            with pytest.raises(S.SfaError):
                se.candidates(bad)
        assert se.candidates([]).shape == (0, 4)
        assert_cand(se.candidates([0, 3]), np.stack([none, none]), True, "no events yet")
        se.extend([0, 2], np.concatenate([a[:70], b[:40]]), [0, 70, 110])
        with pytest.raises(S.SfaError):  # a slot is in use
            se.configure_candidates(2)
        assert_cand(se.candidates([2, 0, 1]), np.stack([want.cand(b[:40]), want.cand(a[:70]), none]), True, "first call")
        se.extend([0], *empty)  # an empty chunk: the stored candidates
        assert_cand(se.candidates([0]), want.cand(a[:70])[None], True, "empty chunk")
        se.reset([0])  # host-only: valid = 0 at once, then the list of the new read only
        assert_cand(se.candidates([0, 2]), np.stack([none, want.cand(b[:40])]), True, "after reset")
        se.extend([0], b[:55], [0, 55])
        assert_cand(se.candidates([0]), want.cand(b[:55])[None], True, "new read")
        nan = a.copy()
        nan[80] = np.nan
        se.extend([2, 0], np.concatenate([nan[70:120], b[55:90]]), [0, 50, 85])  # poisons slot 2, slot 0 beside it goes on
        assert_cand(se.candidates([2, 0]), np.stack([none, want.cand(b[:90])]), True, "poisoned")
        se.extend([2], a[:10], [0, 10])
        assert_cand(se.candidates([2]), none[None], True, "poisoned until reset")
        se.reset([2])
        se.extend([2], a[:10], [0, 10])
        assert_cand(se.candidates([2]), want.cand(a[:10])[None], True, "clean again")
        se.reset()
        se.configure_candidates(0)  # off again: the plain kernels, and nothing to ask for
        with pytest.raises(S.SfaError):
            se.candidates([0])
        got = se.extend([1], a[:70], [0, 70])
        with al.session(2) as plain:
            assert got.tobytes() == plain.extend([1], a[:70], [0, 70]).tobytes()


def _raw_run(al, want, twins, sigs, step, flag, resweep, shape, at, at_end, n_calls):
    """samples in: after every call the candidates are the oracle's for the twin's query -- the window's events as normalised --
    and the rows are those of a session without candidates"""
    slots = sorted(sigs)
    windows = {sl: [] for sl in slots}
    with al.session(len(slots), resweep=resweep, candidates=4) as se, al.session(len(slots), resweep=resweep) as plain:
        for s in (se, plain):
            s.configure_raw(*shape, recalibrate=at, at_end=at_end)
        for c in range(n_calls):
            named = [sl for sl in slots if (sl + c) % 4 != 3 and c * step[sl] < len(sigs[sl])]  # (a changing subset: the others keep theirs)
            if not named:
                continue
            chunks = [sigs[sl][c * step[sl]:(c + 1) * step[sl]] for sl in named]
            end = [(c + 1) * step[sl] >= len(sigs[sl]) for sl in named]
            raw_off = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
            args = (named, np.concatenate(chunks), raw_off, [SCALING] * len(named), end)
            rows, info = se.extend_raw(*args)
            rows_plain, info_plain = plain.extend_raw(*args)
            assert rows.tobytes() == rows_plain.tobytes() and info.tobytes() == info_plain.tobytes(), c
            for sl, chunk, e in zip(named, chunks, end):
                twins[sl].feed(chunk, e)
            qs = []
            for sl in slots:
                q = twins[sl].query_so_far()
                qs.append(np.zeros(0, np.float32) if q is None else np.ascontiguousarray(q, np.float32))
                windows[sl].append(twins[sl].window)
            assert list(se.lengths(slots)) == [len(q) for q in qs], c  # (the twin's query is the one the rows are of)
            assert_cand(se.candidates(slots), np.stack([want.cand(q) for q in qs]), True, f"call {c}")
            mine = se.candidates(named)
            top = mine[:, 0]["valid"] == 1
            assert np.array_equal(rows["score2"][top].view(np.uint32), mine[:, 0]["score"][top].view(np.uint32)), c
    return windows


def test_raw_recalibrating_session(oracle):
    """a session whose normalisation grows with the read (norm 25, doubling list): a recalibrated slot is swept again as a first
    chunk and its list follows that sweep"""
    ref, flag, want = context(oracle, "dna", quant=False)
    shape = (3, 25, 200)
    at = S.recal_double(25, 200)
    rng = np.random.default_rng(16)
    sigs = {sl: synth_signal(rng, n) for sl, n in enumerate([2600, 2600, 1500, 900, 2600, 2000, 300, 2600])}
    step = {sl: s for sl, s in enumerate([400, 333, 250, 450, 1300, 500, 100, 650])}
    twins = {sl: RecalTwin(False, shape, at, True) for sl in sigs}
    with S.Aligner(ref, flag) as al:
        windows = _raw_run(al, want, twins, sigs, step, flag, False, shape, at, True, 9)
    assert any(len(set(w) - {0}) >= 3 for w in windows.values()) and max(max(w) for w in windows.values()) == 200  # (about this test's own inputs)


def test_raw_resweep_session_rna(oracle):
    """direct RNA without INV: the query is the window's events reversed, swept only when the window changes; a call that leaves
    the window alone leaves the candidates as they were"""
    flag = S.RNA
    ref = _small_ref(np.random.default_rng(17), LENS, True, quant=False)
    want = Want(oracle, ref, flag)
    shape, at = (10, 25, 200), (50, 100, 200)
    rng = np.random.default_rng(18)
    sigs = {sl: synth_signal(rng, n) for sl, n in enumerate([7000, 7000, 3000, 5000, 700, 7000])}
    step = {sl: s for sl, s in enumerate([600, 500, 700, 1200, 350, 2400])}
    twins = {sl: SweepTwin(True, shape, at, True) for sl in sigs}
    with S.Aligner(ref, flag) as al:
        windows = _raw_run(al, want, twins, sigs, step, flag, True, shape, at, True, 15)
    grown = [w for w in windows.values() if len(set(w) - {0}) >= 2]
    stood = [w for w in windows.values() if any(a == b and a > 0 for a, b in zip(w, w[1:]))]
    assert grown and stood, windows  # (about this test's own inputs: windows that change, and calls that leave them alone)
