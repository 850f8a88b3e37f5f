"""sfa_session_group_bests against tests/group_oracle.py: numpy over the rows Session.row() reads back, scores bit for bit, contig,
coordinate and strand equal, heads equal.  The shapes are tests/class_shapes.py's (what they reach: tests/test_class_shapes_cpu.py):
rows at every alignment with heads and tails of 0 .. 3 columns, rows shorter than two quads, label changes at every seam of the walk
(inside a quad, between lanes, between waves, between a lane's quads 1024 columns apart, between parts), both reduction paths (one
label per wave, one label per column), n_groups of 1, 2, 64, 65 and 1023, entry 0 / background against sfa_session_classes, ties by
construction, entries whose every column costs +inf, entries without columns, a spread session, slot states, and one
replay(by_name=True) run against `sigfish-amd realtime --by-name`."""
import numpy as np
import pytest

import sigfish_amd as S
from tests import class_shapes as K
from tests import group_oracle as G
from tests import targets_oracle as T
from tests.test_session_class_edges_gpu import columns, flag_of, grow, last_row, strands_of
from tests.test_session_gpu import _events, _small_ref
from tests.test_session_raw_gpu import SCALING, synth_signal
from tests.test_session_targets_gpu import offsets, slot_row, whole

pytestmark = pytest.mark.gpu

CHUNKS = (7, 50)


def runs(ref, spans):
    """group targets for runs of columns [(lo, hi, group)] of a one-strand row"""
    return [(*t, g) for lo, hi, g in spans for t in columns(ref, lo, hi)]


def cyclic(ref, lo, hi, length, n):
    """runs of `length` columns over [lo, hi), groups 0 .. n - 1 in turn"""
    return runs(ref, [(a, min(a + length, hi), ((a - lo) // length) % n) for a in range(lo, hi, length)])


def rows_of(se, slots, ref, strands):
    lens = se.lengths(slots)
    return {sl: slot_row(se, sl, strands, ref.num_ref) for sl, n in zip(slots, lens) if n > 0}


def check_groups(se, slots, gt, n_groups, ref, strands, what, rows, label=None):
    """Session.group_bests of `slots` under the list `gt` against the oracle over `rows` (slot -> carried row); -> (bests, heads)"""
    se.set_target_groups(gt, n_groups)
    assert se.group_count() == n_groups, what
    if label is None:
        label = G.labels_of(gt, n_groups, ref.ref_lengths, ref.st_offset, strands)
    bests, heads = se.group_bests(slots)
    assert bests.shape == (len(slots), n_groups + 1) and heads.shape == (len(slots),)
    lens = se.lengths(slots)
    for i, sl in enumerate(slots):
        h = heads[i]
        if sl not in rows:
            assert lens[i] == 0 and h["valid"] == 0 and h["best"] == -1 and h["second"] == -1 and np.isinf(h["best_score"]) and np.isinf(h["second_score"]), (what, sl, h)
            assert np.isinf(bests[i]["score"]).all() and (bests[i]["rid"] == -1).all() and (bests[i]["pos_end"] == -1).all() and (bests[i]["strand"] == 0).all()
            continue
        want, head = G.entries_of_row(rows[sl], label, n_groups, ref.ref_lengths, ref.st_offset, strands)
        w = np.array([(s, r, p, st, (0, 0, 0)) for s, r, p, st, _ in want], S.GROUP_BEST_DTYPE)
        bad = np.flatnonzero((bests[i]["score"].view(np.uint32) != w["score"].view(np.uint32)) | (bests[i]["rid"] != w["rid"]) | (bests[i]["pos_end"] != w["pos_end"])
                             | (bests[i]["strand"] != w["strand"]))
        assert len(bad) == 0, (what, sl, bad[:5], bests[i][bad[:5]], w[bad[:5]])
        assert (bests[i]["pad"] == 0).all()
        assert h["valid"] == 1 and h["n_events"] == lens[i] and h["best"] == head["best"] and h["second"] == head["second"], (what, sl, h, head)
        assert np.float32(h["best_score"]).view(np.uint32) == np.float32(head["best_score"]).view(np.uint32), (what, sl, h, head)
        assert np.float32(h["second_score"]).view(np.uint32) == np.float32(head["second_score"]).view(np.uint32), (what, sl, h, head)
    return bests, heads


def check_sets(se, slots, sets, ref, strands, what, rows):
    out = {}
    for name, (gt, n_groups) in sets.items():
        out[name] = check_groups(se, slots, gt, n_groups, ref, strands, (what, name), rows)
    return out


# ---- rows at every alignment, label changes inside quads and between lanes, the overlap rule, the group counts ----
def small_sets(ref, shape):
    total = K.total_columns(shape)
    off, n = [int(x) for x in ref.st_offset], [int(x) for x in ref.ref_lengths]
    sets = {
        "one group over everything": ([(*whole(ref, r), 0) for r in range(ref.num_ref)], 1),
        "whole contigs, ids falling": ([(*whole(ref, r), ref.num_ref - 1 - r) for r in range(ref.num_ref)], ref.num_ref),
        # two and three groups over one stretch: the lowest id wins wherever they overlap; touching intervals; group 2 has no column
        "overlaps": ([(3, off[3] + 10, off[3] + 200, 3), (3, off[3] + 50, off[3] + 120, 1), (3, off[3] + 100, off[3] + 260, 0), (1, off[1] + 3, off[1] + 33, 4),
                      (1, off[1] + 33, off[1] + 40, 1), (0, off[0] + 36, off[0] + 38, 5)], 6),
    }
    if shape.rna:
        sets.update({
            # the three columns a head or a tail can have, each its own group
            "head and tail columns": (runs(ref, [(0, 1, 0), (1, 2, 1), (2, 3, 2), (total - 3, total - 2, 3), (total - 2, total - 1, 4), (total - 1, total, 5)]), 6),
            # runs of 5: the label changes at each of a quad's three inner positions and at quad ends, whatever the head is
            "runs of 5": (cyclic(ref, 0, total, 5, 7), 7),
            # runs of 4: between neighbouring lanes for head 0, inside the quads otherwise
            "runs of 4": (cyclic(ref, 0, total, 4, 3), 3),
            "two halves": (runs(ref, [(0, total // 2, 1), (total // 2, total, 0)]), 2),
            "64 runs": (cyclic(ref, 0, total, (total + 63) // 64, 64), 64),
            "65 runs": (cyclic(ref, 0, total, (total + 64) // 65, 65), 65),
            "every column its own, 1023": (runs(ref, [(c, c + 1, (7 * c) % total) for c in range(total)]), 1023),
        })
    return sets


@pytest.mark.parametrize("shape", K.SMALL, ids=[s.name for s in K.SMALL])
def test_rows_at_every_alignment(shape):
    rng = np.random.default_rng(61 + K.total_columns(shape))
    ref = _small_ref(rng, shape.lens, shape.rna)
    strands = strands_of(shape)
    sets = small_sets(ref, shape)
    order = list(range(shape.n_slots - 1, -1, -1))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        with pytest.raises(S.SfaError, match="no groups"):
            se.group_bests([0])
        assert se.group_count() == 0
        for step, n in enumerate(CHUNKS):
            grow(se, order, rng, n)
            rows = rows_of(se, order, ref, strands)
            got = check_sets(se, order, sets, ref, strands, (shape.name, step), rows)
            bests, heads = got["one group over everything"]
            assert (heads["best"] == 0).all() and (heads["second"] == -1).all() and np.isinf(heads["second_score"]).all() and (bests["rid"][:, 1] == -1).all()
            bests, heads = got["overlaps"]
            assert (bests["rid"][:, 2] == -1).all() and np.isinf(bests["score"][:, 2]).all() and (heads["best"] != 2).all() and (heads["second"] != 2).all()
        se.set_target_groups([], 1)
        assert se.group_count() == 0


@pytest.mark.parametrize("shape", K.TINY, ids=[s.name for s in K.TINY])
def test_tiny_rows(shape):
    n = shape.lens[0]
    rng = np.random.default_rng(67 + n)
    ref = _small_ref(rng, shape.lens, True)
    sets = {"every column its own": (runs(ref, [(c, c + 1, n - 1 - c) for c in range(n)]), n), "one group": ([(*whole(ref, 0), 0)], 1),
            "nothing in a group": ([(0, 0, int(ref.st_offset[0]), 0)], 2)}
    order = list(range(shape.n_slots - 1, -1, -1))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        for step, m in enumerate(CHUNKS):
            grow(se, order, rng, m)
            got = check_sets(se, order, sets, ref, 1, (shape.name, step), rows_of(se, order, ref, 1))
            bests, heads = got["every column its own"]
            assert (bests["pos_end"][:, :n] == int(ref.st_offset[0]) + np.arange(n)[::-1]).all() and (bests["rid"][:, n] == -1).all()
            bests, heads = got["nothing in a group"]
            assert (heads["best"] == 2).all() and (heads["second"] == -1).all()


# ---- rows of several parts: seams between waves, between a lane's quads, between parts ----
def wide_sets(ref, shape):
    total = K.total_columns(shape)
    off = [int(x) for x in ref.st_offset]
    sets = {"one group over everything": ([(*whole(ref, r), 0) for r in range(ref.num_ref)], 1)}
    if shape.rna:
        b = K.PART_COLUMNS
        sets.update({
            # a lane's quads are 1024 columns apart: with runs of 1024 every lane changes its label at every u
            "runs of 1024": (cyclic(ref, 0, total, 1024, 3), 3),
            # lanes 63 and 64 of a block meet at column head + 256: every column around it its own group
            "wave boundary": (runs(ref, [(c, c + 1, c - 250) for c in range(250, 264)] + [(0, 250, 15), (264, total, 14)]), 16),
            # the part boundary: columns 8191, 8192, 8193 .. 8196 each alone, a group that spans both parts underneath
            "part boundary": (runs(ref, [(c, c + 1, c - (b - 1)) for c in range(b - 1, b + 5)] + [(b - 200, b + 200, 6)]), 7),
            "a group in each part": (runs(ref, [(p * b + 3, min((p + 1) * b, total - 3), p) for p in range(K.class_parts(total)) if p * b + 3 < total - 3]), K.class_parts(total)),
            "last quads": (runs(ref, [(total - 40, total - 3, 0), (total - 3, total, 1)]), 2),
            "1023 runs": (cyclic(ref, 0, total, (total + 1022) // 1023, 1023), 1023),
        })
        if shape.name == "rna_8197":  # every lane flushes at every column, inside one part
            sets["1023 single columns"] = (runs(ref, [(100 + c, 101 + c, (5 * c) % 1023) for c in range(1023)]), 1023)
        if shape.name == "rna_16433":  # the last part has 12 quads: a group wholly inside it, whatever the head is
            sets["inside the last part"] = (runs(ref, [(2 * b + 3, total - 3, 1), (0, 2 * b + 3, 0)]), 2)
    else:  # dna_20006: column 8192 is column 4095 of (c0, '-'), coordinate off + 2; its neighbours 8191 and 8193 are off + 3, off + 1
        sets["part boundary"] = ([(0, off[0] + 1, off[0] + 2, 0), (0, off[0] + 2, off[0] + 3, 1), (0, off[0] + 3, off[0] + 4, 2), (0, off[0], off[0] + 200, 3),
                                  (2, off[2] + 100, off[2] + 300, 4), (1, off[1] + 5, off[1] + 4000, 5)], 6)
    return sets


@pytest.mark.parametrize("shape", K.WIDE, ids=[s.name for s in K.WIDE])
def test_rows_of_several_parts(shape):
    rng = np.random.default_rng(71 + K.total_columns(shape))
    ref = _small_ref(rng, shape.lens, shape.rna)
    strands = strands_of(shape)
    sets = wide_sets(ref, shape)
    if not shape.rna:  # what the DNA list claims about the boundary
        lab = G.labels_of(*sets["part boundary"], ref.ref_lengths, ref.st_offset, 2)
        assert [int(lab[c]) for c in (8190, 8191, 8192, 8193)] == [3, 2, 1, 0] and lab[8000] == 3 and lab[8194] == 6 and (lab[16384 + 3:] != 3).all() and (lab[16384 + 3:] == 4).any()
    order = list(range(shape.n_slots - 1, -1, -1))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        grow(se, order, rng, CHUNKS[1])
        check_sets(se, order, sets, ref, strands, shape.name, rows_of(se, order, ref, strands))


# ---- entry 0 and the background are the classes of the same intervals ----
def check_against_classes(se, slots, targets, what):
    se.set_targets(targets)  # (mask and labels side by side)
    se.set_target_groups([(*t, 0) for t in targets], 1)
    cls = se.classes(slots)
    bests, heads = se.group_bests(slots)
    for side, e in (("on", 0), ("off", 1)):
        assert np.array_equal(bests["score"][:, e].view(np.uint32), cls[f"{side}_score"].view(np.uint32)), (what, side)
        for f in ("rid", "pos_end", "strand"):
            assert np.array_equal(bests[f][:, e], cls[f"{side}_{f}"]), (what, side, f, bests[f][:, e], cls[f"{side}_{f}"])
    assert np.array_equal(heads["valid"], cls["valid"]) and np.array_equal(heads["n_events"], cls["n_events"]), what
    return cls


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "no_start"])
@pytest.mark.parametrize("shape", K.SMALL + K.WIDE[:1], ids=[s.name for s in K.SMALL + K.WIDE[:1]])
def test_one_group_is_the_on_class(shape, starts):
    rng = np.random.default_rng(73 + K.total_columns(shape))
    ref = _small_ref(rng, shape.lens, shape.rna)
    off = [int(x) for x in ref.st_offset]
    lists = {"scattered": [(ref.num_ref - 1, off[-1] + 10, off[-1] + 30), (1, off[1] + 3, off[1] + 33), (0, off[0] + 2, off[0] + 9), (1, off[1] + 20, off[1] + 50)],
             "everything": [whole(ref, r) for r in range(ref.num_ref)], "a contig": [whole(ref, 0)]}
    order = list(range(shape.n_slots - 1, -1, -1))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots, starts=starts) as se:
        grow(se, order[:-1], rng, CHUNKS[1])  # (slot 0 stays empty)
        for name, t in lists.items():
            cls = check_against_classes(se, order, t, (shape.name, name))
            assert cls["valid"][-1] == 0 and (cls["valid"][:-1] == 1).all()


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "no_start"])
def test_one_group_is_the_on_class_in_raw_mode(starts):
    lens = [37, 64, 65, 300]
    rng = np.random.default_rng(79)
    ref = _small_ref(rng, lens, False)
    targets = [(3, 200, 290), (3, 10, 40), (1, 3, 33), (3, 30, 64), (0, 36, 38)]
    with S.Aligner(ref, 0) as al, al.session(6, starts=starts) as se:
        se.configure_raw(3, 25, 70)
        sig = {sl: synth_signal(rng, 1000) for sl in range(5)}
        slots = list(range(5))  # (the last slot stays empty)
        for k in range(2):
            chunks = [sig[sl][500 * k:500 * (k + 1)] for sl in slots]
            se.extend_raw(slots, np.concatenate(chunks), offsets(chunks), [SCALING] * len(slots))
            cls = check_against_classes(se, list(range(6)), targets, ("raw", k))
            rows = rows_of(se, list(range(6)), ref, 2)
            check_groups(se, list(range(6)), [(*t, g % 3) for g, t in enumerate(targets)], 3, ref, 2, ("raw", k), rows)
        assert cls["valid"][5] == 0 and cls["valid"][:5].any()


# ---- ties by construction ----
@pytest.mark.parametrize("shape", [s for s in K.TIES if s.lens[0] in (4, 256, 8192)], ids=lambda s: s.name)
def test_ties(shape):
    """Reference [A, A, one k-mer] with two levels (tests/test_session_class_edges_gpu.py): columns j and |A| + j of a row are the
    same bits.  In one group the lower column wins; in two groups the scores are equal and the entry holding the lower column comes
    first, although it has the higher index."""
    n = shape.lens[0]
    rng = np.random.default_rng(83 + n)
    lv = lambda m: rng.choice(np.array([-0.5, 0.5], np.float32), m)
    a = lv(n)
    ref = S.RefModel(["c0", "c1", "c2"], [n + 5, n + 5, 6], shape.lens, [1, 2, 3], [a, a.copy(), lv(1)], None)
    order = list(range(shape.n_slots))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        grow(se, order, rng, CHUNKS[1], lv)
        rows = rows_of(se, order, ref, 1)
        n_top = 0
        for sl in order:
            row = rows[sl]
            assert np.array_equal(row[:n].view(np.uint32), row[n:2 * n].view(np.uint32)) and np.isfinite(row).all()
            js = sorted({int(np.argmin(row[:n])), 0, n - 1, n // 2})
            for j in js:
                one = runs(ref, [(j, j + 1, 0), (n + j, n + j + 1, 0)])
                bests, _ = check_groups(se, [sl], one, 1, ref, 1, (shape.name, sl, j, "one group"), rows)
                assert bests["rid"][0, 0] == 0 and bests["pos_end"][0, 0] == 1 + j
                two = runs(ref, [(j, j + 1, 1), (n + j, n + j + 1, 0)])
                bests, heads = check_groups(se, [sl], two, 2, ref, 1, (shape.name, sl, j, "two groups"), rows)
                assert bests["score"][0, 0].view(np.uint32) == bests["score"][0, 1].view(np.uint32) and bests["rid"][0, 1] == 0 and bests["rid"][0, 0] == 1
                if j == int(np.argmin(row[:n])) and row[2 * n] >= row[j]:  # column j is the first minimum of the whole row
                    assert heads["best"][0] == 1 and heads["best_score"][0] == row[j] == heads["second_score"][0]  # (the twin, or an equal column in front of it)
                    assert heads["second"][0] == (0 if row[j] < np.delete(row, [j, n + j]).min() else 2)
                    n_top += 1
        assert n_top >= 1 or n < 256  # (about this test's inputs: the single k-mer of contig 2 does not beat the best of |A| columns)


# ---- entries whose every column costs +inf, entries without columns ----
def test_entries_whose_every_column_costs_inf():
    shape = K.INF
    rng = np.random.default_rng(89)
    base = _small_ref(rng, shape.lens, True)
    fw = [x.copy() for x in base.forward]
    fw[2] = np.full(shape.lens[2], 3e38, np.float32)
    ref = S.RefModel(base.names, base.seq_lengths, base.ref_lengths, base.st_offset, fw, None)
    off = [int(x) for x in ref.st_offset]
    c2 = T.jobs_of(ref.ref_lengths, 1)[2][3]
    order = list(range(shape.n_slots - 1, -1, -1))
    sets = {"contig 2": ([(*whole(ref, 2), 0)], 1),
            "inside contig 2, an empty group, a finite group": (runs(ref, [(c2 + 5, c2 + 20, 0), (0, 30, 2)]), 3),
            "contig 2 and a column of contig 1": ([(*whole(ref, 2), 0), (1, off[1] + 63, off[1] + 64, 0)], 1)}
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        grow(se, order, rng, 9)
        rows = rows_of(se, order, ref, 1)
        for sl in order:
            assert np.isposinf(rows[sl][c2:c2 + 65]).all() and np.isfinite(np.delete(rows[sl], np.arange(c2, c2 + 65))).all()
        got = check_sets(se, order, sets, ref, 1, "inf", rows)
        bests, heads = got["contig 2"]  # +inf at the group's lowest column; the background is best, the group the runner-up
        assert np.isposinf(bests["score"][:, 0]).all() and (bests["rid"][:, 0] == 2).all() and (bests["pos_end"][:, 0] == off[2]).all() and (bests["strand"][:, 0] == ord("+")).all()
        assert (heads["best"] == 1).all() and (heads["second"] == 0).all() and np.isposinf(heads["second_score"]).all()
        for h in heads:  # a runner-up at +inf: any finite margin is met
            assert S.group_decide(h, 9, 1e30) == 1 == G.decide(h, 9, 1e30) and S.group_decide(h, 10, 0.0) is None and G.decide(h, 10, 0.0) is None
        bests, heads = got["inside contig 2, an empty group, a finite group"]
        assert np.isposinf(bests["score"][:, 0]).all() and (bests["pos_end"][:, 0] == off[2] + 5).all()
        assert np.isposinf(bests["score"][:, 1]).all() and (bests["rid"][:, 1] == -1).all() and (bests["pos_end"][:, 1] == -1).all() and (bests["strand"][:, 1] == 0).all()
        assert (heads["best"] != 1).all() and (heads["second"] != 1).all() and (heads["best"] != 0).all() and (heads["second"] != 0).all()
        bests, _ = got["contig 2 and a column of contig 1"]
        assert np.isfinite(bests["score"][:, 0]).all() and (bests["rid"][:, 0] == 1).all()
        for name in sets:  # decisions of the device's heads: the library's rule and the oracle's
            for h in got[name][1]:
                for margin in (0.0, 0.01, 0.5):
                    assert S.group_decide(h, 5, margin) == G.decide(h, 5, margin), (name, h, margin)


# ---- a spread session ----
def test_spread_session_on_rows_of_an_odd_width():
    shape = K.SPREAD
    rng = np.random.default_rng(97)
    ref = _small_ref(rng, shape.lens, True)
    sets = small_sets(ref, shape)
    order = [7, 0, 8, 1, 2, 6, 3]
    slots = list(range(1, shape.n_slots))  # (slot 0 stays empty)
    with S.Aligner(ref, flag_of(shape)) as one, S.Aligner(ref, flag_of(shape), devices=[0, 0]) as many:
        with one.session(shape.n_slots) as plain, many.session(shape.n_slots, spread=True) as spread:
            with pytest.raises(S.SfaError, match="no groups"):
                spread.group_bests([1])
            chunks = [_events(rng, CHUNKS[1], True) for _ in slots]
            for se in (plain, spread):
                se.extend(slots, np.concatenate(chunks), offsets(chunks))
            rows = rows_of(plain, order, ref, 1)
            for name, (gt, n_groups) in sets.items():
                spread.set_target_groups(gt, n_groups)
                assert spread.group_count() == n_groups
                bests, heads = check_groups(plain, order, gt, n_groups, ref, 1, ("plain", name), rows)
                got_b, got_h = spread.group_bests(order)
                assert got_b.tobytes() == bests.tobytes() and got_h.tobytes() == heads.tobytes(), name
            with pytest.raises(S.SfaError, match="twice|more than once"):
                spread.group_bests([1, 2, 1])
            assert many.profile()["class_ms"] > 0 and one.profile()["class_ms"] > 0


# ---- slot states and refusals ----
def test_slot_states_and_refusals():
    shape = K.SMALL[2]
    rng = np.random.default_rng(101)
    ref = _small_ref(rng, shape.lens, True)
    gt, n_groups = small_sets(ref, shape)["runs of 5"]
    with S.Aligner(ref, flag_of(shape)) as al:
        with al.session(shape.n_slots) as se:
            with pytest.raises(S.SfaError, match="no groups"):
                se.group_bests([0])
            grow(se, [1, 2, 3, 4], rng, 20)
            se.reset([2])
            rows = rows_of(se, [0, 1, 2, 3, 4], ref, 1)
            assert sorted(rows) == [1, 3, 4]
            _, heads = check_groups(se, [4, 0, 2, 1, 3], gt, n_groups, ref, 1, "states", rows)
            assert list(heads["valid"]) == [1, 0, 0, 1, 1]
            for bad, word in (([1, 3, 1], "twice|more than once"), ([9], "out of range"), ([-1], "out of range")):
                with pytest.raises(S.SfaError, match=word):
                    se.group_bests(bad)
            for bad, ng, word in (([(0, 1, 5, 7)], 7, "group"), ([(0, 1, 5, -1)], 7, "group"), ([(0, 1, 5, 0)], 0, "n_groups"), ([(0, 1, 5, 0)], 1024, "n_groups"),
                                  ([(4, 1, 5, 0)], 1, "contig"), ([(0, 5, 5, 0)], 1, "empty"), ([(0, 1, 500, 0)], 1, "beyond")):
                with pytest.raises(S.SfaError, match=word):
                    se.set_target_groups(bad, ng)
            assert se.group_count() == n_groups  # (a refused list leaves the table as it was)
            check_groups(se, [1], gt, n_groups, ref, 1, "after refusals", rows)
            se.set_target_groups([], 5)
            with pytest.raises(S.SfaError, match="no groups"):
                se.group_bests([1])
        with al.session(2, resweep=True) as rs:
            with pytest.raises(S.SfaError, match="RESWEEP"):
                rs.set_target_groups(gt, n_groups)


# ---- the real-time front ends: replay(by_name=True) and `sigfish-amd realtime --by-name` ----
def test_replay_by_name_and_the_binary(tmp_path):
    import os
    import subprocess

    from sigfish_amd import realtime, synth
    from tests.realtime_util import BIN, write_model
    from tests.test_session_raw_gpu import META

    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    k = 6
    model = write_model(tmp_path / "syn.model", k, synth.kmer_levels(k, 21))
    levels, _ = S.read_kmer_model(model)
    c0 = synth.random_sequence(905, 1)
    recs = [("c0", c0), ("c1", c0[300:605]), ("c2", synth.random_sequence(62, 3))]
    fasta, blow5, bed = (str(tmp_path / n) for n in ("ref.fa", "reads.blow5", "t.bed"))
    with open(fasta, "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in recs))
    reads = synth.make_dna_raw_reads(recs, levels, k, 12, seed=5, samples=(2000, 9000), kinds=("mapped", "mapped", "random", "mapped", "stalled", "flat"),
                                     meta={**META, "sampling_rate": 4000.0})
    synth.write_blow5(blow5, reads)
    with open(bed, "w") as f:
        f.write("# targets\ntrack name=t\nc0\t100\t400\tleft\nc1\t0\t301\trepeat\nc0\t400\t700\tright\nc0\t650\t800\tleft\n")
    ref = S.RefModel.from_fasta(fasta, levels, k, 0, 70)
    skip, norm, query, min_events, channels, chunk, margin = 3, 25, 70, 30, 4, 800, 0.05
    common = [BIN, "realtime", "--kmer-model", model, "--verbose", "0", "--channels", str(channels), "--chunk-samples", str(chunk), "-p", str(skip), "-q", str(query),
              "--norm-events", str(norm), "--min-events", str(min_events), "--targets", bed, "--enrich", "--margin", str(margin)]
    plain = subprocess.run(common + [fasta, blow5], capture_output=True, timeout=300)
    named = subprocess.run(common + ["--by-name", fasta, blow5], capture_output=True, timeout=300)
    assert plain.returncode == 0 and named.returncode == 0, (plain.stderr.decode(), named.stderr.decode())
    reads = list(S.Blow5File(blow5))
    gt, names = S.read_target_groups(bed, ref.names)
    assert names == ["left", "repeat", "right"] and list(gt["group"]) == [0, 1, 2, 0]
    targets = S.read_targets(bed, ref.names)
    lines, plain_lines, summary, accepted = [], [], {}, {}
    with S.Aligner(ref, 0) as al:
        without = list(realtime.replay(al, reads, channels, chunk, skip, norm, query, min_events, 61, targets=targets, mode=S.ENRICH, margin=margin))
        # a second session that takes the same chunks, asked at the decision tick: the tags recomputed from group_bests
        for item, base in zip(realtime.replay(al, reads, channels, chunk, skip, norm, query, min_events, 61, targets=(gt, names), by_name=True, mode=S.ENRICH, margin=margin,
                                              summary=summary), without):
            tick, ch, index, row, info, span, why, cls, action, head = item
            assert (tick, ch, index, why, base[8]) == (base[0], base[1], base[2], base[6], action) and cls.tobytes() == base[7].tobytes()  # decisions stay the class record's
            rid, _, raw = reads[index]
            line = realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why, target=(cls, S.ENRICH, min_events, margin), group=(head, names))
            old = realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why, target=(cls, S.ENRICH, min_events, margin))
            lines.append(line)
            plain_lines.append(old)
            if not line:
                assert head is None
                continue
            assert line.startswith(old[:-1] + "\ttg:Z:") and line.count("\t") == old.count("\t") + 2
            tg, gm = line.rstrip("\n").split("\t")[-2:]
            want_name = "*" if head["best"] == len(names) else names[int(head["best"])]
            assert tg == "tg:Z:" + want_name and head["valid"] == 1 and head["n_events"] == cls["n_events"]
            with np.errstate(all="ignore"):
                want_gm = (np.float64(head["second_score"] if head["second"] >= 0 else np.inf) - np.float64(head["best_score"])) / int(head["n_events"])
            assert gm == "gm:f:" + ("nan" if want_gm != want_gm else "%.4f" % want_gm)
            # groups and background together are every column, as the two classes are: the best of either is the row's minimum
            assert min(float(cls["on_score"]), float(cls["off_score"])) == float(head["best_score"])
            if action == "A":
                accepted[want_name] = accepted.get(want_name, 0) + 1
    assert plain.stdout.decode() == "".join(plain_lines) and named.stdout.decode() == "".join(lines)
    assert any(ln for ln in lines) and len(lines) == 12
    err = named.stderr.decode().splitlines()
    want_summary = realtime.format_group_summary(summary, names)
    assert "".join(ln + "\n" for ln in err[-len(names) - 1:]) == want_summary
    for name in names + ["*"]:
        assert f"group {name}: accepted {accepted.get(name, 0)} reads\n" in want_summary
    assert plain.stderr.decode().splitlines()[-1] + "\n" == realtime.format_summary(summary) == err[-len(names) - 2] + "\n"
