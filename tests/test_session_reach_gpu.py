"""Reach targets of a session on the device (sfa_session_targets_reach / sfa_session_reach_tables: reach_rules.hpp,
sdtw_session_reach.hpp) against the numpy model of tests/reach_model.py on the case table of tests/reach_cases.py: contigs of 31,
33, 95, 257 and 300 k-mers with non-zero offsets -- jobs start and end inside a mask word, a wave and a block, several jobs share
the first block -- for DNA (two strands) and RNA|INV (one).  The tables exactly; the classes against a numpy min-reduction of
Session.row under the model's mask; lead 0 / strand 0 against a set_targets session byte for byte; reads crafted to end inside a
lead-in; the live mask under a depth cap, which reads the depth of the anchor; switching between reach and plain targets; a
spread session; the refusals."""
import ctypes as C

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib
from tests import reach_cases as RC
from tests import reach_model as M
from tests import targets_oracle as T
from tests.test_session_raw_gpu import SCALING, synth_signal

pytestmark = pytest.mark.gpu

LENS, OFFS = RC.LENS, RC.OFFS
N_SLOTS = 6


def make_ref(rng, rna):
    arr = lambda n: (rng.integers(-6, 7, n) / 4).astype(np.float32)
    fw = [arr(n) for n in LENS]
    return S.RefModel([f"c{i}" for i in range(len(LENS))], [n + 5 for n in LENS], LENS, OFFS, fw, None if rna else [arr(n) for n in LENS])


def flag_of(rna):
    return (S.RNA | S.INV) if rna else 0


def offsets(chunks):
    return np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)


def feed(sessions, rng, slots, n):
    """the same n new events per slot into every session"""
    chunks = [(rng.integers(-6, 7, n) / 4).astype(np.float32) for _ in slots]
    for se in sessions:
        se.extend(slots, np.concatenate(chunks), offsets(chunks))


def slot_row(se, sl, strands):
    return np.concatenate([se.row(sl, r, s)[0] for r in range(len(LENS)) for s in "+-"[:strands]])


def check_tables(se, name, strands):
    mask, _, _, entry = RC.model_tables(name, strands)
    got_mask, got_anchor = se.reach_tables()
    assert got_mask.dtype == bool and got_anchor.dtype == np.int32 and len(got_mask) == len(got_anchor) == strands * sum(LENS)
    assert np.array_equal(got_mask, mask), (name, np.flatnonzero(got_mask != mask)[:8])
    assert np.array_equal(got_anchor.astype(np.int64), entry), (name, np.flatnonzero(got_anchor != entry)[:8])
    return mask


def check_classes(se, slots, mask, strands, what):
    """Session.classes against numpy over the rows under `mask`: lowest cost, then lowest column"""
    assert se.target_columns() == int(mask.sum()), what
    got = se.classes(slots)
    lens = se.lengths(slots)
    for i, sl in enumerate(slots):
        g = got[i]
        if lens[i] == 0:
            assert g["valid"] == 0 and np.isinf(g["on_score"]) and np.isinf(g["off_score"]) and g["on_rid"] == -1 and g["off_rid"] == -1, (what, sl, g)
            continue
        assert g["valid"] == 1 and g["n_events"] == lens[i], (what, sl, g)
        want = T.classes_of_rows(slot_row(se, sl, strands), mask, LENS, OFFS, strands)
        for side in ("on", "off"):
            assert np.float32(g[f"{side}_score"]).view(np.uint32) == np.float32(want[f"{side}_score"]).view(np.uint32), (what, sl, side, g, want)
            for f in ("rid", "pos_end", "strand"):
                assert int(g[f"{side}_{f}"]) == int(want[f"{side}_{f}"]), (what, sl, side, f, g, want)
    return got


@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna_inv"])
def test_tables_are_the_models_and_classes_read_them(rna):
    rng = np.random.default_rng(41 + rna)
    ref = make_ref(rng, rna)
    strands = 1 if rna else 2
    every = list(range(N_SLOTS))
    with S.Aligner(ref, flag_of(rna)) as al, al.session(N_SLOTS) as se:
        with pytest.raises(S.SfaError, match="no reach targets"):
            se.reach_tables()
        feed((se,), rng, every[1:], 40)  # (slot 0 stays empty)
        for name in RC.CASES:  # one list replaces the other
            se.set_reach_targets(RC.CASES[name])
            mask = check_tables(se, name, strands)
            got = check_classes(se, every, mask, strands, name)
            if not mask.any():  # the empty result: a '-' target without '-' jobs
                assert rna and (got["on_rid"] == -1).all() and np.isinf(got["on_score"]).all()
            feed((se,), rng, every[1:], 3)  # the rows move on; the tables do not depend on them
        se.set_reach_targets([])  # off: as set_targets([])
        assert se.target_columns() == 0
        with pytest.raises(S.SfaError, match="no targets"):
            se.classes([1])
        with pytest.raises(S.SfaError, match="no reach targets"):
            se.reach_tables()


@pytest.mark.parametrize("mode", ["dna_no_start", "dna_raw", "dna_raw_no_start", "rna_no_start"])
def test_classes_in_every_mode(mode):
    rna, raw, starts = mode.startswith("rna"), "raw" in mode, "no_start" not in mode
    rng = np.random.default_rng(50 + len(mode))
    ref = make_ref(rng, rna)
    strands = 1 if rna else 2
    every = list(range(N_SLOTS))
    with S.Aligner(ref, flag_of(rna)) as al, al.session(N_SLOTS, starts=starts) as se:
        if raw:
            sig = [synth_signal(rng, 2000) for _ in every[1:]]
            se.configure_raw(3, 25, 70)
            se.extend_raw(every[1:], np.concatenate(sig), offsets(sig), [SCALING] * len(sig))
        else:
            feed((se,), rng, every[1:], 35)
        for name in ("both strands", "overlapping lead-ins", "first and last coordinate", "a thousand"):
            se.set_reach_targets(RC.CASES[name])
            check_classes(se, every, check_tables(se, name, strands), strands, (mode, name))


@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna_inv"])
def test_lead_0_strand_0_is_set_targets(rna):
    rng = np.random.default_rng(43 + rna)
    ref = make_ref(rng, rna)
    strands = 1 if rna else 2
    plain = [(1, 12, 20), (1, 40, 46), (2, 0, 101), (3, 100, 150), (3, 140, 200), (4, 1300, 1301), (4, 1000, 1001), (0, 5, 37)]
    every = list(range(N_SLOTS))
    with S.Aligner(ref, flag_of(rna)) as al, al.session(N_SLOTS) as se, al.session(N_SLOTS) as twin:
        feed((se, twin), rng, every[1:], 40)
        se.set_reach_targets([(c, b, e, 0, None) for c, b, e in plain])
        twin.set_targets(plain)
        assert se.target_columns() == twin.target_columns() > 0
        assert se.classes(every).tobytes() == twin.classes(every).tobytes()
        mask, anchor = se.reach_tables()
        assert np.array_equal(mask, T.mask_of(plain, LENS, OFFS, strands))
        md = M.Reach(LENS, OFFS, strands)
        own = np.array([x - OFFS[c] for g, c, s, x in md.columns()])  # the anchor is the column's own coordinate
        assert np.array_equal(anchor[mask], own[mask]) and (anchor[~mask] == S.REACH_NONE).all()


def test_reads_that_end_inside_a_lead_in():
    """a '+' read and a '-' read whose events are the reference's own levels and end 30 bases in front of the target, in their own
    direction: cost 0 in a column the lead admits -- on target under reach, off target under set_targets of the same interval"""
    rng = np.random.default_rng(47)
    ref = make_ref(rng, False)
    c, b, e, lead = 4, 1100, 1150, 64
    plus_end, minus_end = 1070 - OFFS[c], LENS[c] - (1180 - OFFS[c])  # columns of coordinate 1070 on '+' and 1180 on '-'
    reads = [ref.forward[c][plus_end - 40:plus_end + 1], ref.reverse[c][minus_end - 40:minus_end + 1]]
    with S.Aligner(ref, 0) as al, al.session(2) as se, al.session(2) as twin:
        for s in (se, twin):
            s.extend([0, 1], np.concatenate(reads), offsets(reads))
        se.set_reach_targets([(c, b, e, lead, None)])
        twin.set_targets([(c, b, e)])
        got, plain = se.classes([0, 1]), twin.classes([0, 1])
        assert (got["on_score"] == 0).all() and (got["off_score"] > 0).all() and (got["on_rid"] == c).all()
        assert list(got["on_strand"]) == [ord("+"), ord("-")]
        assert b - lead <= got["on_pos_end"][0] < b and e <= got["on_pos_end"][1] < e + lead  # in front of the target, each in its direction
        assert (plain["off_score"] == 0).all() and (plain["on_score"] > 0).all()
        for k in range(2):
            assert S.target_decide(got[k], S.ENRICH, 10, 0.01) == "A" and S.target_decide(plain[k], S.ENRICH, 10, 0.01) == "U"
        # the lead of the other strand alone admits neither read's column
        se.set_reach_targets([(c, b, e, lead, "-")])
        assert se.classes([0])["on_score"][0] > 0 and se.classes([1])["on_score"][0] == 0
        se.set_reach_targets([(c, b, e, lead, "+")])
        assert se.classes([0])["on_score"][0] == 0 and se.classes([1])["on_score"][0] > 0


def check_depth(se, md, what):
    for c in range(len(LENS)):
        assert np.array_equal(se.coverage(c).astype(np.int64), md.depth[c]), (what, c)


@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna_inv"])
def test_the_cap_reads_the_depth_of_the_anchor(rna):
    rng = np.random.default_rng(53 + rna)
    ref = make_ref(rng, rna)
    strands = 1 if rna else 2
    targets = RC.CASES["both strands"] + RC.CASES["touching"] + RC.CASES["bodies below the offset"]
    other = RC.CASES["overlapping lead-ins"] + RC.CASES["one"]
    plain = [(3, 40, 90), (4, 1090, 1160)]
    every = list(range(N_SLOTS))
    cap = 2
    md = M.Reach(LENS, OFFS, strands)
    with S.Aligner(ref, flag_of(rna)) as al, al.session(N_SLOTS) as se:
        feed((se,), rng, every[1:], 40)
        se.set_reach_targets(targets)
        se.configure_coverage(cap)
        base, _ = md.entries(targets)
        check_classes(se, every, base, strands, "depth 0: live = base")
        # a target's first bases only; its whole body; a lead-in but not the body; each twice (cap - 1 is open, cap closed)
        steps = [[(3, 50, 53)], [(3, 50, 53)], [(4, 1100, 1150)], [(4, 1100, 1150)], [(4, 1036, 1100), (4, 1150, 1214)] * 2, [(2, 114, 120), (2, 120, 121)] * 2, [],
                 [(2, 100, 196)] * 2]
        before = int(base.sum())  # open columns after the step before
        for k, iv in enumerate(steps):
            n_open = se.add_coverage(iv)
            md.add(iv)
            live = md.live_mask(targets, cap)
            assert n_open == int(live.sum()), (k, n_open, int(live.sum()))
            check_classes(se, every, live, strands, ("step", k))
            check_depth(se, md, ("step", k))
            if k == 1:  # coordinates 50 .. 52 of contig 3 are closed, and with them the whole '+' lead-in 20 .. 49, whose anchor is 50; 53 .. 79 are open
                at = [a for c, s, a in md.jobs if (c, s) == (3, "+")][0]
                assert not live[at + 13:at + 46].any() and live[at + 46:at + 73].all() and int(base.sum()) - int(live.sum()) == 33 + (3 if strands == 2 else 0)
            if k == 4:  # covering the lead-ins of (4, 1100, 1150) changed nothing: they were closed with the body, and close nothing themselves
                assert n_open == before
            before = n_open
            feed((se,), rng, every[1:], 2)
        assert live[(md.entries(targets)[1] == M.BELOW_TRACK)].all()  # anchors below the track are never closed
        # ---- reach -> plain -> reach: the depth is kept, the live mask is derived again each time ----
        se.set_targets(plain)
        check_depth(se, md, "plain targets")
        with pytest.raises(S.SfaError, match="no reach targets"):
            se.reach_tables()
        mp = T.mask_of(plain, LENS, OFFS, strands)
        own = np.array([md.depth[c][x - OFFS[c]] < cap for g, c, s, x in md.columns()])  # a plain mask reads the column's own coordinate again
        check_classes(se, every, mp & own, strands, "plain targets")
        se.set_reach_targets(other)
        check_depth(se, md, "reach again")
        check_classes(se, every, md.live_mask(other, cap), strands, "reach again")
        assert np.array_equal(se.reach_tables()[0], md.entries(other)[0])  # (the base mask is kept beside the live one)
        # ---- cap off: the base mask answers; reach off: the cap goes with the targets ----
        se.configure_coverage(0)
        check_classes(se, every, md.entries(other)[0], strands, "cap off")
        se.configure_coverage(cap)
        se.set_reach_targets([])
        with pytest.raises(S.SfaError, match="no coverage cap"):
            se.coverage(0)


def test_spread_session_answers_as_the_plain_one():
    rng = np.random.default_rng(59)
    ref = make_ref(rng, False)
    order = [5, 0, 3, 1, 4]
    md = M.Reach(LENS, OFFS, 2)
    with S.Aligner(ref, 0) as one, S.Aligner(ref, 0, devices=[0, 0]) as many:
        with one.session(N_SLOTS) as plain, many.session(N_SLOTS, spread=True) as spread:
            feed((plain, spread), rng, list(range(1, N_SLOTS)), 45)
            for name in ("a thousand", "both strands"):
                for se in (plain, spread):
                    se.set_reach_targets(RC.CASES[name])
                check_tables(spread, name, 2)
                assert spread.target_columns() == plain.target_columns() == int(RC.model_tables(name, 2)[0].sum())
                assert spread.classes(order).tobytes() == plain.classes(order).tobytes(), name
            for se in (plain, spread):
                se.configure_coverage(1)
            for iv in ([(4, 1100, 1101)], [(3, 50, 80)]):
                md.add(iv)
                a, b = plain.add_coverage(iv), spread.add_coverage(iv)
                assert a == b == int(md.live_mask(RC.CASES["both strands"], 1).sum())
                assert spread.classes(order).tobytes() == plain.classes(order).tobytes()
            with pytest.raises(S.SfaError, match="lead -1 outside"):
                spread.set_reach_targets([(4, 1100, 1150, -1, None)])
            check_tables(spread, "both strands", 2)  # a refusal on every shard leaves every shard as it was
            spread.set_targets([(4, 1100, 1150)])
            with pytest.raises(S.SfaError, match="no reach targets"):
                spread.reach_tables()


def test_refusals_leave_the_session_as_it_was():
    rng = np.random.default_rng(61)
    ref = make_ref(rng, False)
    lib = _lib.load()
    with S.Aligner(ref, 0) as al, al.session(3) as se:
        feed((se,), rng, [0, 1, 2], 30)
        se.set_reach_targets(RC.CASES["both strands"])
        se.configure_coverage(3)
        se.add_coverage([(4, 1100, 1120)])
        depth = se.coverage(4)
        before = se.classes([0, 1, 2]).tobytes()
        good = (4, 1000, 1301, 1 << 30, "-")
        bad = [((-1, 0, 1, 0, None), "contig -1 out of range"), ((5, 0, 1, 0, None), "contig 5 out of range"), ((2, -1, 4, 0, None), "is negative"), ((2, 4, 4, 0, None), "is empty"),
               ((2, 100, 197, 0, None), "lies beyond contig 2"), ((2, 100, 110, -1, None), "lead -1 outside"), ((2, 100, 110, (1 << 30) + 1, None), "outside 0 .. 1073741824"),
               ((2, 100, 110, 3, "x"), "strand 120"), ((2, 100, 110, 3, 1), "strand 1 is none")]
        for t, word in bad:
            with pytest.raises(S.SfaError, match=word) as err:
                se.set_reach_targets([good, t])
            assert "sfa_session_targets_reach: target 1:" in str(err.value)
        padded = np.zeros(2, S.REACH_TARGET_DTYPE)
        padded[0] = padded[1] = (4, 1100, 1150, 5, 0, (0, 0, 0))
        padded["pad"][1][2] = 1
        with pytest.raises(S.SfaError, match="target 1: the padding is not zero"):
            se.set_reach_targets(padded)
        with pytest.raises(S.SfaError, match="at most 1048576"):
            se.set_reach_targets(np.zeros((1 << 20) + 1, S.REACH_TARGET_DTYPE))
        assert lib.sfa_session_targets_reach(None, None, 0) != 0 and lib.sfa_session_targets_reach(se._h, None, 2) != 0 and b"bad argument" in lib.sfa_last_error()
        # the tables, the classes and the depth are what they were
        check_tables(se, "both strands", 2)
        assert se.classes([0, 1, 2]).tobytes() == before and np.array_equal(se.coverage(4), depth)
        # sfa_session_reach_tables: sizes, and either pointer may be NULL
        cols = 2 * sum(LENS)
        words = (cols + 31) // 32 + 1
        m, a = np.zeros(words + 1, np.uint32), np.full(cols + 1, 7, np.int32)
        mp, ap = m.ctypes.data_as(C.POINTER(C.c_uint32)), a.ctypes.data_as(_lib.i32p)
        for nw, nc in ((words - 1, cols), (words + 1, cols), (words, cols - 1), (words, cols + 1), (0, 0)):
            assert lib.sfa_session_reach_tables(se._h, mp, nw, ap, nc) != 0
        assert not m.any() and (a == 7).all()  # nothing was written by a refused call
        assert lib.sfa_session_reach_tables(se._h, mp, words, None, 0) == 0 and lib.sfa_session_reach_tables(se._h, None, 0, ap, cols) == 0
        assert lib.sfa_session_reach_tables(se._h, None, 0, None, 0) == 0 and lib.sfa_session_reach_tables(None, mp, words, ap, cols) != 0
        assert m[words] == 0 and m[words - 1] == 0 and a[cols] == 7  # the spare word is zero; nothing behind the tables was touched
        assert np.array_equal(a[:cols].astype(np.int64), RC.model_tables("both strands", 2)[3])
        # the longest lead and a '-' target over a whole contig pass
        se.set_reach_targets([good])
        assert se.target_columns() == LENS[4]
        with al.session(2, resweep=True) as rs:
            with pytest.raises(S.SfaError, match="RESWEEP"):
                rs.set_reach_targets(RC.CASES["one"])
            with pytest.raises(S.SfaError, match="no reach targets"):
                rs.reach_tables()
