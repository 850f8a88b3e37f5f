"""Coverage caps of a session on the device (sfa_session_coverage_config / _add / _depth) against the numpy model of
tests/coverage_model.py: the depth tracks integer for integer after every call, the live count after every call, and the live
mask through machinery that exists already -- a second, fresh session is given set_targets(the model's open pieces), and the
classes of all slots of the two sessions are the same records, byte for byte, on the same carried rows.  Contigs of 31 .. 70
columns with non-zero offsets (mask words straddle jobs, a contig ends inside a word), 6 slots."""
import ctypes as C

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib
from tests import coverage_model as M
from tests.test_session_raw_gpu import SCALING, synth_signal

pytestmark = pytest.mark.gpu

LENS = [31, 33, 70, 45]
OFFS = [0, 7, 100, 3]
N_SLOTS = 6


def make_ref(rng, rna):
    arr = lambda n: (rng.integers(-6, 7, n) / 4).astype(np.float32)
    fw = [arr(n) for n in LENS]
    return S.RefModel([f"c{i}" for i in range(len(LENS))], [n + 5 for n in LENS], LENS, OFFS, fw, None if rna else [arr(n) for n in LENS])


def flag_of(rna):
    return (S.RNA | S.INV) if rna else 0


def whole(r):
    return (r, OFFS[r], OFFS[r] + LENS[r] + 1)


def offsets(chunks):
    return np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)


def feed(sessions, rng, slots, n):
    """the same n new events per slot into every session"""
    chunks = [(rng.integers(-6, 7, n) / 4).astype(np.float32) for _ in slots]
    for se in sessions:
        se.extend(slots, np.concatenate(chunks), offsets(chunks))


def check_depth(se, model, what):
    for c in range(len(LENS)):
        got = se.coverage(c)
        assert got.dtype == np.uint32 and len(got) == LENS[c] + 1 and np.array_equal(got.astype(np.int64), model.depth[c]), (what, c, got, model.depth[c])


def check_live(se, fresh, model, targets, slots, what):
    """the live mask of `se` is the base mask of the model's open pieces: counts, and the class records of every slot"""
    want = model.open_columns(targets)
    assert se.target_columns() == want, (what, se.target_columns(), want)
    got = se.classes(slots)
    pieces = model.open_list(targets)
    if not pieces:  # every on-target column is closed: an empty class, as the header defines it
        assert want == 0 and (got["on_rid"] == -1).all() and (got["on_pos_end"] == -1).all() and np.isposinf(got["on_score"]).all() and (got["on_strand"] == 0).all(), (what, got)
        live = got["valid"] == 1
        assert (got["off_rid"][live] >= 0).all() and np.isfinite(got["off_score"][live]).all()
        return got
    fresh.set_targets(pieces)
    assert fresh.target_columns() == want, what
    ref = fresh.classes(slots)
    assert got.tobytes() == ref.tobytes(), (what, got, ref)
    return got


ADDS = [("one-base intervals", [(2, 100, 101), (2, 151, 152), (2, 152, 153), (1, 38, 39), (0, 30, 31), (3, 20, 21)]),
        ("a whole contig", [whole(1)]),
        ("coordinate off and the last coordinate off + ref_len", [(2, 100, 103), (2, 168, 171), (3, 3, 4), (3, 48, 49), (0, 0, 1), (0, 31, 32)]),
        ("300 identical intervals", [(2, 120, 150)] * 300),
        ("two contigs interleaved", [(3, 5, 30), (1, 8, 20), (3, 20, 40), (1, 10, 39), (3, 5, 30), (1, 8, 20), (3, 47, 49)]),
        ("n = 0", []),
        ("below the offset", [(2, 0, 101), (3, 0, 3), (1, 0, 8)])]


@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna"])
def test_depth_is_exact_and_the_count_is_the_models(rna):
    rng = np.random.default_rng(3 + rna)
    ref = make_ref(rng, rna)
    strands = 1 if rna else 2
    targets = [whole(r) for r in range(4)]
    model = M.Coverage(LENS, OFFS, strands, 301)
    every = list(range(N_SLOTS))
    with S.Aligner(ref, flag_of(rna)) as al, al.session(N_SLOTS) as se, al.session(N_SLOTS) as fresh:
        feed((se, fresh), rng, every[1:], 40)  # (slot 0 stays empty)
        se.set_targets(targets)
        se.configure_coverage(301)
        assert se.target_columns() == strands * sum(LENS)
        check_depth(se, model, "zeroed")
        for name, iv in ADDS:
            n_open = se.add_coverage(iv)
            model.add(iv)
            check_depth(se, model, name)
            assert n_open == model.open_columns(targets) == se.target_columns(), (name, n_open)
        assert al.profile()["class_ms"] > 0
        # 300 copies under a cap of 301: every column is still open
        assert model.depth[2][20:50].min() == model.depth[2].max() == 300 and se.target_columns() == strands * sum(LENS)
        check_live(se, fresh, model, targets, every, "cap 301")
        # ... and the 301st copy closes exactly those 30 coordinates, on every strand
        n_open = se.add_coverage([(2, 120, 150)])
        model.add([(2, 120, 150)])
        assert n_open == model.open_columns(targets) == strands * sum(LENS) - strands * 30
        check_live(se, fresh, model, targets, every, "301 copies")


def words_bit(model, targets, strand, bit):
    """(contig, coordinate) of an on-target column of a `strand` job that sits at bit `bit` of its mask word, away from the job's ends"""
    base = model.base_mask(targets)
    for c, s, at in model.jobs:
        for j in range(2, model.rl[c] - 2):
            if s == strand and (at + j) % 32 == bit and base[at + j]:
                return c, M.place_col(s, j, model.rl[c], model.off[c])
    raise AssertionError("no such column")


@pytest.mark.parametrize("mode", ["dna", "rna", "dna_no_start", "dna_raw"])
def test_live_mask_through_a_fresh_session(mode):
    """after every step the classes of the capped session are those of a session that was GIVEN the model's open pieces as targets"""
    rna, raw, starts = mode == "rna", mode == "dna_raw", mode != "dna_no_start"
    rng = np.random.default_rng(11 + len(mode))
    ref = make_ref(rng, rna)
    strands = 1 if rna else 2
    targets = [whole(2), (3, 10, 40), (1, 7, 20), (0, 0, 5)]
    other = [whole(3), (2, 110, 160), (1, 30, 41)]
    every = list(range(N_SLOTS))
    slots = every[1:]  # (slot 0 stays empty)
    with S.Aligner(ref, flag_of(rna)) as al, al.session(N_SLOTS, starts=starts) as se, al.session(N_SLOTS, starts=starts) as fresh:
        if raw:
            sig = [synth_signal(rng, 2000) for _ in slots]
            for s in (se, fresh):
                s.configure_raw(3, 25, 70)
                s.extend_raw(slots, np.concatenate(sig), offsets(sig), [SCALING] * len(slots))
        else:
            feed((se, fresh), rng, slots, 35)
        se.set_targets(targets)
        fresh.set_targets(targets)
        plain = fresh.classes(every)  # a session without the feature: what the base mask answers
        assert plain["valid"][0] == 0 and (raw or (plain["valid"][1:] == 1).all())
        # ---- cap = 1 ----
        model = M.Coverage(LENS, OFFS, strands, 1)
        se.configure_coverage(1)
        assert se.classes(every).tobytes() == plain.tobytes() and se.target_columns() == fresh.target_columns()  # depth 0: live = base
        last = "+-"[strands - 1]
        steps = [[(2, 120, 121)], [(2, 100, 101), (2, 170, 171)], [(3, 0, 25), (1, 19, 30)], [],
                 [(c, x, x + 1) for c, x in (words_bit(model, targets, "+", 0), words_bit(model, targets, "+", 31), words_bit(model, targets, last, 0), words_bit(model, targets, last, 31))]]
        for k, iv in enumerate(steps):
            n_open = se.add_coverage(iv)
            model.add(iv)
            assert n_open == model.open_columns(targets), (mode, k)
            check_live(se, fresh, model, targets, every, (mode, "cap 1", k))
            if not raw:  # the rows move on between the steps; the mask does not depend on them
                feed((se, fresh), rng, slots, 5)
        # ---- set_targets again with other intervals: the depth is kept ----
        se.set_targets(other)
        assert se.target_columns() == model.open_columns(other)
        check_live(se, fresh, model, other, every, (mode, "other targets"))
        check_depth(se, model, (mode, "other targets"))
        # ---- every on-target column closed ----
        closing = [whole(r) for r in range(4)]
        assert se.add_coverage(closing) == 0
        model.add(closing)
        got = check_live(se, fresh, model, other, every, (mode, "all closed"))
        assert got["valid"][0] == 0 and (raw or (got["valid"][1:] == 1).all())
        # ---- cap 0: exactly the base-mask answers, and the calls that need a cap are refused again ----
        se.configure_coverage(0)
        fresh.set_targets(other)
        assert se.classes(every).tobytes() == fresh.classes(every).tobytes() and se.target_columns() == fresh.target_columns() > 0
        with pytest.raises(S.SfaError, match="no coverage cap"):
            se.add_coverage([(0, 0, 1)])
        # ---- cap = 2: depth cap - 1 is open and cap is closed, on the same coordinate; the depth starts from zero again ----
        model = M.Coverage(LENS, OFFS, strands, 2)
        se.configure_coverage(2)
        check_depth(se, model, "configured again")
        full = model.open_columns(other)
        for k in range(2):
            assert se.add_coverage([(2, 110, 140)]) == full - (strands * 30 if k else 0)
            model.add([(2, 110, 140)])
            check_live(se, fresh, model, other, every, (mode, "cap 2", k))
        assert int(model.depth[2][10]) == 2 and model.open_columns(other) == fresh.target_columns() == full - strands * 30


def test_spread_session_answers_as_the_plain_one():
    rng = np.random.default_rng(29)
    ref = make_ref(rng, False)
    targets = [whole(2), (3, 10, 40), (1, 7, 20)]
    model = M.Coverage(LENS, OFFS, 2, 2)
    order = [5, 0, 3, 1, 4]
    with S.Aligner(ref, 0) as one, S.Aligner(ref, 0, devices=[0, 0]) as many:
        with one.session(N_SLOTS) as plain, many.session(N_SLOTS, spread=True) as spread:
            feed((plain, spread), rng, list(range(1, N_SLOTS)), 45)
            for se in (plain, spread):
                se.set_targets(targets)
                se.configure_coverage(2)
            for k, iv in enumerate(([(2, 100, 140), (3, 0, 20)], [(2, 120, 171), (3, 15, 30), (1, 7, 8)], [], [whole(1)] * 2)):
                model.add(iv)
                a, b = plain.add_coverage(iv), spread.add_coverage(iv)
                assert a == b == model.open_columns(targets) == spread.target_columns(), (k, a, b)  # shard 0's count, not a sum
                check_depth(spread, model, ("spread", k))
                assert spread.classes(order).tobytes() == plain.classes(order).tobytes(), k
            with pytest.raises(S.SfaError, match="beyond"):
                spread.add_coverage([(1, 7, 50)])
            check_depth(spread, model, "after a refusal")
            spread.set_targets([])  # the cap goes with the targets
            with pytest.raises(S.SfaError, match="no coverage cap"):
                spread.coverage(0)
            with pytest.raises(S.SfaError, match="no targets"):
                spread.configure_coverage(2)


def test_refusals_by_message():
    rng = np.random.default_rng(31)
    ref = make_ref(rng, False)
    lib = _lib.load()
    u32p = C.POINTER(C.c_uint32)
    with S.Aligner(ref, 0) as al, al.session(2) as se:
        with pytest.raises(S.SfaError, match="no targets"):
            se.configure_coverage(3)
        se.configure_coverage(0)  # off is always allowed
        se.set_targets([whole(2)])
        for call, word in ((lambda: se.add_coverage([(2, 100, 101)]), "no coverage cap"), (lambda: se.coverage(2), "no coverage cap"),
                           (lambda: se.configure_coverage(-1), "cap must be 0"), (lambda: se.configure_coverage((1 << 30) + 1), "cap must be 0")):
            with pytest.raises(S.SfaError, match=word):
                call()
        se.configure_coverage(1 << 30)
        se.configure_coverage(4)
        se.add_coverage([(2, 100, 110)])
        before = [se.coverage(c) for c in range(4)]
        for iv, word in (((-1, 0, 1), "contig -1 out of range"), ((4, 0, 1), "contig 4 out of range"), ((2, -1, 4), "is negative"), ((2, 104, 104), "is empty"),
                         ((2, 100, 172), "lies beyond contig 2")):
            with pytest.raises(S.SfaError, match=word) as e:
                se.add_coverage([(2, 100, 101), iv])
            assert "sfa_session_coverage_add: target 1:" in str(e.value)  # coverage_list_error's own words
        with pytest.raises(S.SfaError, match="at most 1048576"):
            se.add_coverage(np.zeros((1 << 20) + 1, S.TARGET_DTYPE))
        with pytest.raises(S.SfaError, match="contig 4 out of range"):
            se.coverage(4)
        buf = np.zeros(200, np.uint32)
        for n in (70, 72, 0):  # contig 2 has 71 entries
            assert lib.sfa_session_coverage_depth(se._h, 2, buf.ctypes.data_as(u32p), n) != 0
            assert b"71 entries" in lib.sfa_last_error()
        assert lib.sfa_session_coverage_depth(se._h, 2, None, 71) != 0 and lib.sfa_session_coverage_depth(None, 2, buf.ctypes.data_as(u32p), 71) != 0
        assert lib.sfa_session_coverage_config(None, 1) != 0 and lib.sfa_session_coverage_add(None, None, 0, None) != 0
        assert lib.sfa_session_coverage_add(se._h, None, 1, None) != 0 and b"bad argument" in lib.sfa_last_error()
        assert (buf == 0).all()  # nothing was written by a refused call
        for c in range(4):  # ... nor to the tracks
            assert np.array_equal(se.coverage(c), before[c])
        assert int(before[2][:10].min()) == 1 and int(before[2].sum()) == 10
        se.set_targets([])  # n = 0 switches the cap off too
        with pytest.raises(S.SfaError, match="no coverage cap"):
            se.coverage(2)
        with al.session(2, resweep=True) as rs:
            with pytest.raises(S.SfaError, match="RESWEEP"):
                rs.set_targets([whole(2)])
            with pytest.raises(S.SfaError, match="no targets"):
                rs.configure_coverage(2)
