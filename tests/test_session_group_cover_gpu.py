"""Group caps of a session on the device (sfa_session_group_coverage_config / sfa_session_group_coverage, and the live label table
behind sfa_session_open_classes / sfa_session_group_bests) against the numpy model of tests/group_cover_model.py, by exact equality.
After every add: the depth tracks and the groups' records are the model's, integer for integer; and the live table is checked
through machinery that exists already -- a second, FRESH session is given the model's open pieces as its group targets, and
open_classes (every group open, and a bitmap with some closed) and group_bests of the two sessions are the same bytes on the same
carried rows.  Shapes are tests/class_shapes.py's where they fit (what a lane's quad of four columns, a wave of 256 and a block of
1024 columns meet there is said at each case)."""
import ctypes as C

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib
from tests import class_shapes as K
from tests import coverage_model as CM
from tests import group_cover_model as M
from tests.test_session_raw_gpu import SCALING, synth_signal

pytestmark = pytest.mark.gpu

SPAN = 1024  # columns of a block of either kernel: 256 lanes of four


def make_ref(rng, lens, rna):
    arr = lambda n: (rng.integers(-6, 7, n) / 4).astype(np.float32)
    offs = [(3 * r + 7 * (r % 2)) for r in range(len(lens))]
    fw = [arr(n) for n in lens]
    return S.RefModel([f"c{i}" for i in range(len(lens))], [n + 5 for n in lens], lens, offs, fw, None if rna else [arr(n) for n in lens]), offs


def flag_of(rna):
    return (S.RNA | S.INV) if rna else 0


def offsets(chunks):
    return np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)


def feed(sessions, rng, slots, n):
    """the same n new events per slot into every session"""
    chunks = [(rng.integers(-6, 7, n) / 4).astype(np.float32) for _ in slots]
    for se in sessions:
        se.extend(slots, np.concatenate(chunks), offsets(chunks))


def bitmap(n_groups, open_groups):
    w = np.zeros((n_groups + 31) // 32, np.uint32)
    for g in open_groups:
        w[g >> 5] |= np.uint32(1 << (g & 31))
    return w


def some_closed(n_groups):
    """every group open but those with id = 1 (mod 3); with one group: it is closed"""
    return bitmap(n_groups, [g for g in range(n_groups) if g % 3 != 1] if n_groups > 1 else [])


def check(se, fresh, model, slots, what, depth=True):
    """everything the capped session `se` answers against the model; the live table through `fresh`"""
    n_groups = model.n_groups
    if depth:
        for c in range(len(model.rl)):
            got = se.coverage(c)
            assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), model.depth[c]), (what, c)
    rec = se.group_coverage()
    assert rec.dtype == S.GROUP_COVER_DTYPE and rec.tobytes() == model.records().astype(S.GROUP_COVER_DTYPE).tobytes(), (what, rec, model.records())
    pieces = model.open_pieces()
    live = model.live_labels()
    assert (len(pieces) > 0) == bool((live != n_groups).any())
    if not pieces:  # every column is background: no group has a column, the ON class is empty as the open call documents
        got = se.open_classes(slots)
        ok = got["cls"]["valid"] == 1
        assert (got["on_group"] == -1).all() and (got["cls"]["on_rid"] == -1).all() and np.isposinf(got["cls"]["on_score"]).all(), (what, got)
        assert (got["off_group"][ok] == n_groups).all() and np.isfinite(got["cls"]["off_score"][ok]).all(), (what, got)
        bests, heads = se.group_bests(slots)
        assert (heads["best"][ok] == n_groups).all() and (heads["second"] == -1).all() and (bests["rid"][:, :n_groups] == -1).all(), (what, heads)
        return
    fresh.set_target_groups(pieces, n_groups)
    for bits in (None, some_closed(n_groups)):
        a, b = se.open_classes(slots, bits), fresh.open_classes(slots, bits)
        assert a.tobytes() == b.tobytes(), (what, bits, a, b)
    (ab, ah), (bb, bh) = se.group_bests(slots), fresh.group_bests(slots)
    assert ab.tobytes() == bb.tobytes() and ah.tobytes() == bh.tobytes(), (what, ah, bh)
    # a group without live columns has no column at all: its first went to "none", and nothing is placed in it
    gone = [g for g in range(n_groups) if not (live == g).any()]
    assert (ab["rid"][:, gone] == -1).all() and np.isposinf(ab["score"][:, gone]).all(), (what, gone)
    # ... and directly: under a bitmap that holds only a group whose every column is capped (while other groups still have live
    # columns) the ON class is empty and falls back as the open call documents -- the firsts come from the LIVE table
    capped_out = [g for g in gone if (model.base_labels() == g).any()]
    if capped_out:
        only = se.open_classes(slots, bitmap(n_groups, capped_out[:1]))
        ok = only["cls"]["valid"] == 1
        assert (only["on_group"] == -1).all() and (only["cls"]["on_rid"] == -1).all() and np.isposinf(only["cls"]["on_score"]).all(), (what, capped_out[0], only)
        assert (only["off_group"][ok] >= 0).all() and (only["cls"]["off_rid"][ok] >= 0).all(), (what, only)


def coords_of(model):
    """every (contig, coordinate) some column reports, contig after contig"""
    return [(c, model.off[c] + k) for c in range(len(model.rl)) for k in range(model.rl[c] + (model.strands - 1))]


def cyclic_targets(lens, offs, length, n_groups):
    """runs of `length` coordinates over every contig, groups 0 .. n_groups - 1 in turn, every fifth run left to the background"""
    out, k = [], 0
    for c, n in enumerate(lens):
        for a in range(0, n + 1, length):
            if k % 5 != 4:
                out.append((c, offs[c] + a, offs[c] + min(a + length, n + 1), k % n_groups))
            k += 1
    return out


def steps_for(lens, offs, cap):
    """adds that reach: intervals that overlap inside one call, a coordinate driven to exactly cap beside one at cap - 1, n = 0,
    the first and last coordinate of a contig, and at the end every coordinate of every contig closed"""
    last = len(lens) - 1
    n, o = lens[last], offs[last]
    mid = o + n // 2
    steps = [[(last, o, o + 1), (last, o + n, o + n + 1), (0, offs[0], offs[0] + 1)],
             [(last, mid, min(mid + 9, o + n + 1)), (last, max(mid - 3, o), mid + 1), (last, mid, mid + 1)] * max(cap - 1, 1),
             [],
             [(last, mid, mid + 1), (0, offs[0], offs[0] + lens[0] + 1)]]
    if n >= 8:  # the first quarter of the last contig and nothing of its last: a '-' job read the wrong way round closes the wrong end
        steps.append([(last, o + 1, o + n // 4 + 1)] * cap)
    steps.append([(c, offs[c], offs[c] + lens[c] + 1) for c in range(len(lens))] * cap)
    return steps


def run_case(rng, lens, rna, n_groups, targets_of, cap, n_slots=3, starts=True, raw=False, steps=None, events=20):
    ref, offs = make_ref(rng, lens, rna)
    strands = 1 if rna else 2
    targets = targets_of(lens, offs)
    model = M.GroupCover(lens, offs, strands, n_groups, targets, cap)
    every = list(range(n_slots))
    slots = every[1:]  # (slot 0 stays empty)
    with S.Aligner(ref, flag_of(rna)) as al, al.session(n_slots, starts=starts) as se, al.session(n_slots, starts=starts) as fresh:
        if raw:
            sig = [synth_signal(rng, 2000) for _ in slots]
            for s in (se, fresh):
                s.configure_raw(3, 25, 70)
                s.extend_raw(slots, np.concatenate(sig), offsets(sig), [SCALING] * len(slots))
        else:
            feed((se, fresh), rng, slots, events)
        se.set_target_groups(targets, n_groups)
        fresh.set_target_groups(targets, n_groups)
        plain = fresh.open_classes(every)
        se.configure_group_coverage(cap)
        assert se.open_classes(every).tobytes() == plain.tobytes()  # depth 0: the live table is the base table
        check(se, fresh, model, every, ("configured", lens))
        for k, iv in enumerate(steps if steps is not None else steps_for(lens, offs, cap)):
            se.add_coverage(iv)
            model.add(iv)
            check(se, fresh, model, every, (lens, n_groups, cap, k))
            if not raw and k < 2:  # the rows move on between the steps; the table does not depend on them
                feed((se, fresh), rng, slots, 3)
        assert al.profile()["class_ms"] > 0
    return model


# rows of 1 .. 7 columns: a quad that is the whole row, the last quad stored column by column
@pytest.mark.parametrize("shape", K.TINY, ids=[s.name for s in K.TINY])
def test_rows_shorter_than_two_quads(shape):
    rng = np.random.default_rng(sum(shape.lens))
    for cap in (1, 2):
        run_case(rng, shape.lens, True, 2, lambda lens, offs: [(0, offs[0], offs[0] + (lens[0] + 1) // 2, 1), (0, offs[0] + lens[0] // 2, offs[0] + lens[0] + 1, 0)], cap)


# odd totals and totals that are no multiple of 64 or 1024; jobs that begin at columns 37, 101, 166: inside a lane's quad (37 = 4 * 9 + 1);
# dna_930: a '-' job, whose depth reads descend, behind every '+' job
@pytest.mark.parametrize("shape", K.SMALL, ids=[s.name for s in K.SMALL])
def test_small_rows_at_every_alignment(shape):
    rng = np.random.default_rng(sum(shape.lens))
    model = run_case(rng, shape.lens, shape.rna, 7, lambda lens, offs: cyclic_targets(lens, offs, 5, 7), 3)
    assert model.total % 64 != 0 and any(at % 4 for _, _, at in model.jobs)


# every coordinate a group of its own (465 .. 469 groups), so that ONE wrong label anywhere in the live table changes an answer: the
# group of that column gains or loses its only column (one strand) or one of its two.  The columns behind a job's first -- 37, 101,
# 166: the second, second and third of their quads -- and the '-' columns, whose depth entries fall as the column rises, are what
# this is for; the adds close one end of a contig and not the other
@pytest.mark.parametrize("shape", K.SMALL, ids=[s.name for s in K.SMALL])
def test_every_column_its_own_group(shape):
    rng = np.random.default_rng(7 + sum(shape.lens))
    lens = shape.lens
    strands = 1 if shape.rna else 2
    n_coords = sum(n + strands - 1 for n in lens)
    assert n_coords <= 1023

    def each(lens, offs):
        cs = [(c, offs[c] + k) for c in range(len(lens)) for k in range(lens[c] + strands - 1)]
        return [(c, x, x + 1, g) for g, (c, x) in enumerate(cs)]

    offs = make_ref(np.random.default_rng(0), lens, shape.rna)[1]
    steps = [[(1, offs[1], offs[1] + 3), (2, offs[2], offs[2] + 2), (3, offs[3], offs[3] + 1)],  # the first coordinates of contigs 1 .. 3: the columns at the job starts
             [(3, offs[3] + 200, offs[3] + lens[3] + 1), (0, offs[0] + 30, offs[0] + 38)],      # the far end of two contigs only
             [(1, offs[1] + 1, offs[1] + 21)]]
    run_case(rng, lens, shape.rna, n_coords, each, 1, steps=steps, events=12)


@pytest.mark.parametrize("mode", ["no_start", "raw"])
def test_other_session_kinds(mode):
    shape = K.SMALL[4]  # dna_930
    rng = np.random.default_rng(17)
    run_case(rng, shape.lens, shape.rna, 4, lambda lens, offs: cyclic_targets(lens, offs, 9, 4), 2, starts=mode != "no_start", raw=mode == "raw")


# rows of more than one block: group 0 spans blocks (runs of 1500 coordinates, three groups in turn), jobs that begin inside a block
@pytest.mark.parametrize("shape", K.WIDE[2:], ids=[s.name for s in K.WIDE[2:]])
def test_rows_of_several_blocks(shape):
    rng = np.random.default_rng(sum(shape.lens))
    model = run_case(rng, shape.lens, shape.rna, 3, lambda lens, offs: cyclic_targets(lens, offs, 1500, 3), 2, events=8)
    assert model.total > 16 * SPAN and model.total % SPAN
    base = model.base_labels()
    assert len({c // SPAN for c in np.flatnonzero(base == 0)}) > 3  # the global merge: one entry from several blocks


# more than 64 blocks (513 of them), one group over nearly all of them
def test_a_row_of_more_than_64_blocks():
    shape = K.HUGE
    rng = np.random.default_rng(5)
    n = shape.lens[0]
    steps = [[(0, 3, 4), (0, 1024, 1030), (0, n - 1, n), (0, 200000, 200001)], [(0, 0, 300000)], [(0, 0, n + 1), (0, 250000, n + 1)]]
    model = run_case(rng, shape.lens, True, 3, lambda lens, offs: [(0, offs[0] + 2, offs[0] + 500000, 1), (0, offs[0] + 1000, offs[0] + 3000, 0), (0, offs[0] + 524000, offs[0] + 524302, 2)], 2,
                     n_slots=2, steps=steps, events=4)
    assert model.total > 64 * SPAN


# single-column groups, so that every entry of the LDS tables is used: 1101 columns (odd, two blocks, no multiple of 64)
@pytest.mark.parametrize("n_groups", [1, 32, 33, 1023])
def test_every_entry_of_the_tables(n_groups):
    rng = np.random.default_rng(n_groups)
    lens = [700, 401]

    def singles(lens, offs):
        cs = [(c, offs[c] + k) for c in range(2) for k in range(lens[c])]
        return [(c, x, x + 1, g) for g, (c, x) in enumerate(cs[30:30 + n_groups])]

    cap = 2
    offs = make_ref(np.random.default_rng(0), lens, True)[1]
    steps = [[(0, offs[0] + 30, offs[0] + 60)], [(0, offs[0] + 25, offs[0] + 50), (1, offs[1], offs[1] + 100)], [(0, offs[0], offs[0] + 701), (1, offs[1], offs[1] + 402)] * 2]
    model = run_case(rng, lens, True, n_groups, singles, cap, steps=steps, events=8)
    assert (model.records()["columns"][:n_groups] == 1).all() and (model.records()["capped"][:n_groups] == 1).all()


def test_both_caps_on_one_session_share_one_track():
    """the mask call follows the mask's cap, the label calls the group cap, over ONE depth track; either config(0) keeps the depth
    while the other cap is on, and the track goes when both are 0; set_target_groups again with a cap on"""
    shape = K.SMALL[4]  # dna_930
    lens = shape.lens
    rng = np.random.default_rng(23)
    ref, offs = make_ref(rng, lens, False)
    n_groups = 5
    targets = cyclic_targets(lens, offs, 11, n_groups)
    mask_targets = [(3, offs[3] + 10, offs[3] + 200), (1, offs[1], offs[1] + 65), (0, offs[0] + 5, offs[0] + 20)]
    gm = M.GroupCover(lens, offs, 2, n_groups, targets, 3)  # group cap 3
    mm = CM.Coverage(lens, offs, 2, 1)                      # mask cap 1
    every = [0, 1, 2]
    with S.Aligner(ref, 0) as al, al.session(3) as se, al.session(3) as fresh:
        feed((se, fresh), rng, every[1:], 30)
        se.set_target_groups(targets, n_groups)
        se.set_targets(mask_targets)
        se.configure_group_coverage(3)  # the group cap first: it allocates the track
        first = [(3, offs[3] + 50, offs[3] + 120), (3, offs[3] + 100, offs[3] + 150), (1, offs[1] + 2, offs[1] + 9)]
        se.add_coverage(first)
        gm.add(first)
        mm.add(first)
        check(se, fresh, gm, every, "group cap alone")
        assert se.target_columns() == int(mm.base_mask(mask_targets).sum())  # no mask cap: the mask's own columns
        se.configure_coverage(1)  # the mask's cap second: the depth is kept, and closes what it covers at once
        assert se.target_columns() == mm.open_columns(mask_targets) < int(mm.base_mask(mask_targets).sum())

        def mask_side(what):
            fresh.set_targets(mm.open_list(mask_targets))
            assert se.classes(every).tobytes() == fresh.classes(every).tobytes(), what
            assert se.target_columns() == mm.open_columns(mask_targets), what

        for k, iv in enumerate(([(3, offs[3] + 60, offs[3] + 110)], [(3, offs[3] + 60, offs[3] + 110), (0, offs[0], offs[0] + 38)])):
            n_open = se.add_coverage(iv)  # ONE add to the shared track; both derives in the call
            gm.add(iv)
            mm.add(iv)
            assert n_open == mm.open_columns(mask_targets)
            mask_side(("both", k))
            check(se, fresh, gm, every, ("both", k))
        assert int(gm.depth[3].max()) == 4 and 3 in gm.depth[3] and 2 in gm.depth[3]  # cap - 1 and cap side by side, and beyond
        # set_target_groups again with the cap on: a new base table, the live one from the kept depth
        other = cyclic_targets(lens, offs, 17, 3)
        se.set_target_groups(other, 3)
        gm = M.GroupCover(lens, offs, 2, 3, other, 3)
        for c in range(len(lens)):
            gm.depth[c][:] = mm.depth[c]
        check(se, fresh, gm, every, "groups again")
        # the mask's cap off: the depth stays for the group cap
        se.configure_coverage(0)
        fresh.set_targets(mask_targets)
        assert se.classes(every).tobytes() == fresh.classes(every).tobytes() and se.target_columns() == fresh.target_columns()
        check(se, fresh, gm, every, "mask cap off")
        se.set_targets([])  # ... and the mask itself off: still kept
        check(se, fresh, gm, every, "mask off")
        # the reverse: mask cap on again (depth kept), group cap off, depth still there
        se.set_targets(mask_targets)
        se.configure_coverage(1)
        mask_side("mask cap again")
        se.configure_group_coverage(0)
        with pytest.raises(S.SfaError, match="no group cap"):
            se.group_coverage()
        for c in range(len(lens)):
            assert np.array_equal(se.coverage(c).astype(np.int64), mm.depth[c])
        mask_side("group cap off")
        fresh.set_target_groups(other, 3)
        assert se.open_classes(every).tobytes() == fresh.open_classes(every).tobytes()  # the base table again
        # both 0: the track is freed; the next config starts from zero
        se.configure_coverage(0)
        with pytest.raises(S.SfaError, match="no coverage cap"):
            se.coverage(0)
        with pytest.raises(S.SfaError, match="no coverage cap"):
            se.add_coverage([(0, offs[0], offs[0] + 1)])
        se.configure_group_coverage(1)
        gm = M.GroupCover(lens, offs, 2, 3, other, 1)
        check(se, fresh, gm, every, "from zero")
        se.set_target_groups([], 1)  # n = 0 drops the group cap too
        with pytest.raises(S.SfaError, match="no coverage cap"):
            se.coverage(0)


def test_spread_session_answers_as_the_plain_one():
    shape = K.SPREAD  # 467 columns: odd
    lens = shape.lens
    rng = np.random.default_rng(29)
    ref, offs = make_ref(rng, lens, True)
    n_groups = 6
    targets = cyclic_targets(lens, offs, 13, n_groups)
    model = M.GroupCover(lens, offs, 1, n_groups, targets, 2)
    order = [5, 0, 3, 1, 4]
    with S.Aligner(ref, flag_of(True)) as one, S.Aligner(ref, flag_of(True), devices=[0, 0]) as many:
        with one.session(6) as plain, many.session(6, spread=True) as spread, one.session(6) as fresh:
            feed((plain, spread, fresh), rng, list(range(1, 6)), 30)
            with pytest.raises(S.SfaError, match="no groups"):
                spread.configure_group_coverage(2)
            for se in (plain, spread):
                se.set_target_groups(targets, n_groups)
                se.configure_group_coverage(2)
            for k, iv in enumerate(([(3, offs[3] + 10, offs[3] + 140), (0, offs[0], offs[0] + 20)], [(3, offs[3] + 100, offs[3] + 302), (1, offs[1], offs[1] + 1)], [], [(2, offs[2], offs[2] + 66)] * 2)):
                model.add(iv)
                plain.add_coverage(iv)
                spread.add_coverage(iv)
                check(spread, fresh, model, order, ("spread", k))
                assert spread.open_classes(order, some_closed(n_groups)).tobytes() == plain.open_classes(order, some_closed(n_groups)).tobytes(), k
                assert spread.group_coverage().tobytes() == plain.group_coverage().tobytes()
            spread.set_target_groups([], 1)
            with pytest.raises(S.SfaError, match="no group cap"):
                spread.group_coverage()


def test_refusals_by_message():
    rng = np.random.default_rng(31)
    lens = [31, 33, 70]
    ref, offs = make_ref(rng, lens, False)
    lib = _lib.load()
    gcp = C.POINTER(_lib.SfaGroupCover)
    with S.Aligner(ref, 0) as al, al.session(2) as se:
        with pytest.raises(S.SfaError, match="no groups"):
            se.configure_group_coverage(3)
        se.configure_group_coverage(0)  # off is always allowed
        se.set_targets([(2, offs[2], offs[2] + 71)])  # a mask is no substitute for groups
        with pytest.raises(S.SfaError, match="no groups"):
            se.configure_group_coverage(3)
        se.set_target_groups([(2, offs[2], offs[2] + 71, 0), (1, offs[1], offs[1] + 5, 2)], 3)
        for call, word in ((lambda: se.configure_group_coverage(-1), "cap must be 0"), (lambda: se.configure_group_coverage((1 << 30) + 1), "cap must be 0"),
                           (lambda: se.group_coverage(), "no group cap"), (lambda: se.add_coverage([(2, offs[2], offs[2] + 1)]), "no coverage cap"),
                           (lambda: se.coverage(2), "no coverage cap")):
            with pytest.raises(S.SfaError, match=word):
                call()
        se.configure_group_coverage(1 << 30)
        se.configure_group_coverage(4)
        se.add_coverage([(2, offs[2], offs[2] + 10)])
        before = se.group_coverage()
        assert before["depth_sum"][0] == 10 and before["columns"][0] == 70 and before["columns"][1] == 0 and before["depth_min"][1] == 2 ** 32 - 1
        out = np.frombuffer(np.full(8 * 32, 0x5A, np.uint8).tobytes(), S.GROUP_COVER_DTYPE).copy()
        for n in (3, 5, 0, -1):  # the session has 4 entries
            assert lib.sfa_session_group_coverage(se._h, out.ctypes.data_as(gcp), n) != 0
            assert b"4 entries" in lib.sfa_last_error()
        assert lib.sfa_session_group_coverage(se._h, None, 4) != 0 and lib.sfa_session_group_coverage(None, out.ctypes.data_as(gcp), 4) != 0
        assert lib.sfa_session_group_coverage_config(None, 1) != 0
        assert (out.view(np.uint8) == 0x5A).all()  # nothing was written by a refused call
        with pytest.raises(S.SfaError, match="beyond"):
            se.add_coverage([(2, offs[2], offs[2] + 72)])
        assert se.group_coverage().tobytes() == before.tobytes()  # ... nor to the tracks
        with al.session(2, resweep=True) as rs:
            with pytest.raises(S.SfaError, match="RESWEEP"):
                rs.set_target_groups([(2, offs[2], offs[2] + 71, 0)], 1)
            with pytest.raises(S.SfaError, match="no groups"):
                rs.configure_group_coverage(2)
