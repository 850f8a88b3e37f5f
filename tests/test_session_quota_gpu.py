"""sfa_session_open_classes against tests/quota_oracle.py: numpy over the rows Session.row() reads back, scores bit for bit, contig,
coordinate, strand and group equal.  The shapes are tests/class_shapes.py's (what they reach: tests/test_class_shapes_cpu.py): rows at
every alignment with heads and tails of 0 .. 3 columns, rows shorter than two quads, class changes at every seam of the walk (inside
a quad, between lanes, between waves, between a lane's quads 1024 columns apart, between parts, in the rows kernel's second round),
every group open against sfa_session_classes on the mask of the same intervals, every group closed, the word edges of the bitmap,
ties and +inf classes by construction, the overlap rule, a spread session, slot states, refusals with `out` untouched, and a batch
between two calls."""
import ctypes as C

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib
from tests import class_shapes as K
from tests import group_oracle as G
from tests import quota_oracle as Q
from tests import targets_oracle as T
from tests.test_session_class_edges_gpu import columns, flag_of, grow, strands_of
from tests.test_session_gpu import _events, _small_ref
from tests.test_session_raw_gpu import SCALING, synth_signal
from tests.test_session_targets_gpu import offsets, slot_row, whole

pytestmark = pytest.mark.gpu

CHUNK = 50
FIELDS = ("rid", "pos_end", "strand")


def runs(ref, spans):
    """group targets for runs of columns [(lo, hi, group)] of a one-strand row"""
    return [(*t, g) for lo, hi, g in spans for t in columns(ref, lo, hi)]


def span_labels(total, spans, n_groups):
    """the labels of runs(), without a pass per target: the lowest group over every column"""
    label = np.full(total, n_groups, np.int64)
    for lo, hi, g in spans:
        label[lo:hi] = np.minimum(label[lo:hi], g)
    return label


def cyclic(lo, hi, length, n):
    """spans of `length` columns over [lo, hi), groups 0 .. n - 1 in turn"""
    return [(a, min(a + length, hi), ((a - lo) // length) % n) for a in range(lo, hi, length)]


def rows_of(se, slots, ref, strands):
    lens = se.lengths(slots)
    return {sl: slot_row(se, sl, strands, ref.num_ref) for sl, n in zip(slots, lens) if n > 0}


def assert_none(rec, what):
    c = rec["cls"]
    assert c["valid"] == 0 and np.isposinf(c["on_score"]) and np.isposinf(c["off_score"]), (what, rec)
    assert c["on_rid"] == c["on_pos_end"] == c["off_rid"] == c["off_pos_end"] == rec["on_group"] == rec["off_group"] == -1 and c["on_strand"] == c["off_strand"] == 0, (what, rec)


def check_open(se, slots, n_groups, open_bits, label, ref, strands, what, rows):
    """Session.open_classes of `slots` under the bitmap against the oracle over `rows` (slot -> carried row); -> the records"""
    got = se.open_classes(slots, open_bits)
    assert got.dtype == S.OPEN_CLASS_DTYPE and got.shape == (len(slots),)
    lens = se.lengths(slots)
    for i, sl in enumerate(slots):
        if sl not in rows:
            assert_none(got[i], (what, sl))
            continue
        want = Q.record_of_row(rows[sl], label, n_groups, open_bits, ref.ref_lengths, ref.st_offset, strands)
        c = got[i]["cls"]
        for side in ("on", "off"):
            assert np.float32(c[f"{side}_score"]).view(np.uint32) == np.float32(want[f"{side}_score"]).view(np.uint32), (what, sl, side, got[i], want)
            for f in FIELDS:
                assert c[f"{side}_{f}"] == want[f"{side}_{f}"], (what, sl, side, f, got[i], want)
            assert got[i][f"{side}_group"] == want[f"{side}_group"], (what, sl, side, got[i], want)
        assert c["valid"] == 1 and c["n_events"] == lens[i] and (c["pad"] == 0).all(), (what, sl, got[i])
    return got


def check_case(se, slots, gt, n_groups, opens, ref, strands, what, rows, label=None):
    """one list of group targets under several bitmaps (lists of open groups, or None); -> {index of the bitmap: records}"""
    se.set_target_groups(gt, n_groups)
    if label is None:
        label = G.labels_of(gt, n_groups, ref.ref_lengths, ref.st_offset, strands)
    return [check_open(se, slots, n_groups, None if o is None else Q.bitmap(n_groups, o), label, ref, strands, (what, k), rows) for k, o in enumerate(opens)]


# ---- every group open: cls is the record of sfa_session_classes on the mask of the same intervals ----
def open_is_classes(se, slots, targets, n_groups, what):
    se.set_targets(targets)  # (mask and labels side by side)
    se.set_target_groups([(*t, k % n_groups) for k, t in enumerate(targets)], n_groups)
    cls = se.classes(slots)
    for bits in (None, Q.bitmap(n_groups, range(n_groups))):
        got = se.open_classes(slots, bits)
        assert got["cls"].tobytes() == cls.tobytes(), (what, got["cls"], cls)
        live = cls["valid"] == 1
        assert ((got["on_group"][live] < n_groups) & ((got["on_group"][live] >= 0) == (cls["on_rid"][live] >= 0))).all(), what
        assert ((got["off_group"][live] == n_groups) == (cls["off_rid"][live] >= 0)).all() and (got["on_group"][~live] == -1).all() and (got["off_group"][~live] == -1).all(), what
    return cls


def lists_of(ref):
    off, n = [int(x) for x in ref.st_offset], [int(x) for x in ref.ref_lengths]
    last = ref.num_ref - 1
    out = {"everything": [whole(ref, r) for r in range(ref.num_ref)], "a contig": [whole(ref, 0)], "first and last coordinates": [(0, off[0], off[0] + 1), (last, off[last] + n[last] - 1, off[last] + n[last] + 1)]}
    if n[last] > 60:
        out["scattered"] = [(last, off[last] + 10, off[last] + 30), (1, off[1] + 3, off[1] + 33), (0, off[0] + 2, off[0] + 9), (1, off[1] + 20, off[1] + 50)]
    return out


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "no_start"])
@pytest.mark.parametrize("shape", K.SMALL + K.TINY, ids=[s.name for s in K.SMALL + K.TINY])
def test_every_group_open_is_the_class_call(shape, starts):
    rng = np.random.default_rng(103 + K.total_columns(shape))
    ref = _small_ref(rng, shape.lens, shape.rna)
    order = list(range(shape.n_slots - 1, -1, -1))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots, starts=starts) as se:
        with pytest.raises(S.SfaError, match="no groups"):
            se.open_classes([0])
        grow(se, order[:-1], rng, CHUNK)  # (slot 0 stays empty)
        for name, t in lists_of(ref).items():
            for n_groups in (1, 3):
                cls = open_is_classes(se, order, t, n_groups, (shape.name, name, n_groups))
                assert cls["valid"][-1] == 0 and (cls["valid"][:-1] == 1).all()


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "no_start"])
def test_raw_mode(starts):
    lens = [37, 64, 65, 300]
    rng = np.random.default_rng(107)
    ref = _small_ref(rng, lens, False)
    targets = [(3, 200, 290), (3, 10, 40), (1, 3, 33), (3, 30, 64), (0, 36, 38)]
    gt = [(*t, g % 3) for g, t in enumerate(targets)]
    with S.Aligner(ref, 0) as al, al.session(6, starts=starts) as se:
        se.configure_raw(3, 25, 70)
        sig = {sl: synth_signal(rng, 1000) for sl in range(5)}
        slots = list(range(5))  # (the last slot stays empty)
        for k in range(2):
            chunks = [sig[sl][500 * k:500 * (k + 1)] for sl in slots]
            se.extend_raw(slots, np.concatenate(chunks), offsets(chunks), [SCALING] * len(slots))
            cls = open_is_classes(se, list(range(6)), targets, 3, ("raw", k))
            rows = rows_of(se, list(range(6)), ref, 2)
            got = check_case(se, list(range(6)), gt, 3, [None, [0, 2], [1], []], ref, 2, ("raw", k), rows)
        assert cls["valid"][5] == 0 and cls["valid"][:5].any() and (got[1]["cls"]["valid"][:5] == cls["valid"][:5]).all()


# ---- rows at every alignment: every group closed, a class change at every position of a quad, runs of 4 and 5, the overlap rule ----
@pytest.mark.parametrize("shape", K.SMALL + K.TINY, ids=[s.name for s in K.SMALL + K.TINY])
def test_rows_at_every_alignment(shape):
    total = K.total_columns(shape)
    rng = np.random.default_rng(109 + total)
    ref = _small_ref(rng, shape.lens, shape.rna)
    strands = strands_of(shape)
    order = list(range(shape.n_slots - 1, -1, -1))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        for step, n in enumerate((7, CHUNK)):
            grow(se, order, rng, n)
            rows = rows_of(se, order, ref, strands)
            what = (shape.name, step)
            # every group closed: the ON class is empty, OFF is the row's overall best (its first minimum)
            everything = [(*whole(ref, r), r % 2) for r in range(ref.num_ref)]
            got = check_case(se, order, everything, 2, [[], [0], [1], None], ref, strands, (what, "whole contigs"), rows)
            closed = got[0]
            assert (closed["cls"]["on_rid"] == -1).all() and np.isposinf(closed["cls"]["on_score"]).all() and (closed["on_group"] == -1).all() and (closed["cls"]["on_strand"] == 0).all()
            for i, sl in enumerate(order):
                c = int(np.argmin(rows[sl]))
                assert closed["cls"]["off_score"][i] == rows[sl][c] and (closed["cls"]["off_rid"][i], closed["cls"]["off_pos_end"][i]) == G.place(c, ref.ref_lengths, ref.st_offset, strands)[:2]
                assert closed["off_group"][i] == G.place(c, ref.ref_lengths, ref.st_offset, strands)[0] % 2
            assert (got[3]["cls"]["off_rid"] == -1).all() and (got[3]["off_group"] == -1).all()  # every column is in an open group: OFF is empty
            if not shape.rna:
                continue
            # every column its own group, the odd ones closed: the class changes at every position inside a quad
            each = [(c, c + 1, c) for c in range(total)]
            odd_closed = [g for g in range(total) if g % 2 == 0]
            got = check_case(se, order, runs(ref, each), total, [odd_closed, [g for g in range(total) if g % 2], None], ref, 1, (what, "every column its own"), rows,
                             label=span_labels(total, each, total))
            assert (got[0]["on_group"] % 2 == 0).all() and (got[0]["off_group"] % 2 == 1).all() or total < 2
            for length, n_groups, opens in ((4, 3, [[0], [1, 2], [1]]), (5, 7, [[0, 2, 4, 6], [3], [1, 5, 6]])):
                if total >= length:
                    spans = cyclic(0, total, length, n_groups)
                    check_case(se, order, runs(ref, spans), n_groups, opens, ref, 1, (what, "runs of", length), rows, label=span_labels(total, spans, n_groups))
            # the three columns a head or a tail can have, each its own group; one open at a time
            if total >= 8:
                spans = [(0, 1, 0), (1, 2, 1), (2, 3, 2), (total - 3, total - 2, 3), (total - 2, total - 1, 4), (total - 1, total, 5)]
                got = check_case(se, order, runs(ref, spans), 6, [[g] for g in range(6)] + [[0, 1, 2, 3, 4]], ref, 1, (what, "head and tail columns"), rows)
                for g in range(6):
                    assert (got[g]["on_group"] == g).all()


def test_the_overlap_rule():
    """a column covered by several groups follows the lowest id's bit only"""
    shape = K.SMALL[2]
    rng = np.random.default_rng(113)
    ref = _small_ref(rng, shape.lens, True)
    off = [int(x) for x in ref.st_offset]
    # groups 3 > 1 > 0 nested over contig 3; group 2 has no column; group 4 and 1 touch on contig 1
    gt = [(3, off[3] + 10, off[3] + 200, 3), (3, off[3] + 50, off[3] + 120, 1), (3, off[3] + 100, off[3] + 260, 0), (1, off[1] + 3, off[1] + 33, 4), (1, off[1] + 33, off[1] + 40, 1),
          (0, off[0] + 36, off[0] + 38, 5)]
    order = list(range(shape.n_slots))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        grow(se, order, rng, CHUNK)
        rows = rows_of(se, order, ref, 1)
        opens = [[3], [1], [0], [0, 1], [1, 3], [2], [3, 4, 5], [0, 1, 3, 4, 5]]
        got = check_case(se, order, gt, 6, opens, ref, 1, "overlaps", rows)
        label = G.labels_of(gt, 6, ref.ref_lengths, ref.st_offset, 1)
        at = T.jobs_of(ref.ref_lengths, 1)[3][3]
        assert [int(label[at + c]) for c in (9, 10, 49, 50, 99, 100, 259, 260)] == [6, 3, 3, 1, 1, 0, 0, 6]
        # only the lower id open: the winner lies where the lower id covers; only the higher open: never where the lower covers
        for k, o in enumerate(opens):
            on_cols = got[k]["cls"]["on_pos_end"][got[k]["cls"]["on_rid"] == 3] - off[3]
            assert all(int(label[at + c]) in o for c in on_cols)
        assert (got[5]["cls"]["on_rid"] == -1).all()  # the group without columns: an empty ON class


# ---- rows of several parts ----
@pytest.mark.parametrize("shape", [s for s in K.WIDE if s.rna], ids=lambda s: s.name)
def test_rows_of_several_parts(shape):
    total = K.total_columns(shape)
    rng = np.random.default_rng(127 + total)
    ref = _small_ref(rng, shape.lens, True)
    b = K.PART_COLUMNS
    order = list(range(shape.n_slots - 1, -1, -1))
    cases = {
        # a lane's quads are 1024 columns apart: with runs of 1024 every lane changes its class at every u
        "runs of 1024": (cyclic(0, total, 1024, 3), 3, [[0], [1], [0, 2]]),
        # lanes 63 and 64 of a block meet at column head + 256: every column around it its own group
        "lanes 63 / 64": ([(c, c + 1, c - 250) for c in range(250, 264)] + [(0, 250, 15), (264, total, 14)], 16, [[g for g in range(14) if g % 2], [g for g in range(14) if g % 2 == 0], [5, 6]]),
        # an open group that spans two parts, everything else closed or background
        "an open group over two parts": ([(b - 300, b + 300, 1), (0, b - 300, 0), (b + 300, total, 2)], 3, [[1], [0, 2]]),
        # the class changes at column 8192 - 1, 8192, 8192 + 1 (whatever the head is, these are the last and first quads of parts)
        "8192 +- 1": ([(0, b - 1, 0), (b - 1, b, 1), (b, b + 1, 2), (b + 1, b + 2, 3), (b + 2, total, 4)], 5, [[1], [2], [3], [0, 2, 4], [1, 3]]),
        "last quads": ([(total - 40, total - 3, 0), (total - 3, total, 1)], 2, [[0], [1]]),
    }
    if shape.name == "rna_16433":  # the last part has 12 quads: a closed group wholly inside it, whatever the head is
        cases["a closed group inside the last part"] = ([(2 * b + 3, total - 3, 1), (0, 2 * b + 3, 0)], 2, [[0], [1]])
        assert K.layout(total, 0).part_quads[-1] == 12
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        grow(se, order, rng, CHUNK)
        rows = rows_of(se, order, ref, 1)
        for name, (spans, n_groups, opens) in cases.items():
            got = check_case(se, order, runs(ref, spans), n_groups, opens, ref, 1, (shape.name, name), rows, label=span_labels(total, spans, n_groups))
            if name == "8192 +- 1":
                for k in range(3):  # one column is the whole ON class
                    assert (got[k]["cls"]["on_pos_end"] - int(ref.st_offset[0]) == b - 1 + k).all() or shape.lens[0] <= b + 1
            if name == "a closed group inside the last part":
                assert (got[0]["off_group"] == 1).all() and (got[1]["on_group"] == 1).all()


def test_dna_rows_of_several_parts():
    shape = K.WIDE[3]
    rng = np.random.default_rng(131)
    ref = _small_ref(rng, shape.lens, False)
    off = [int(x) for x in ref.st_offset]
    # column 8192 is column 4095 of (c0, '-'), coordinate off + 2; its neighbours 8191 and 8193 are off + 3, off + 1
    gt = [(0, off[0] + 1, off[0] + 2, 0), (0, off[0] + 2, off[0] + 3, 1), (0, off[0] + 3, off[0] + 4, 2), (0, off[0], off[0] + 200, 3), (2, off[2] + 100, off[2] + 300, 4),
          (1, off[1] + 5, off[1] + 4000, 5)]
    lab = G.labels_of(gt, 6, ref.ref_lengths, ref.st_offset, 2)
    assert [int(lab[c]) for c in (8190, 8191, 8192, 8193)] == [3, 2, 1, 0]
    order = list(range(shape.n_slots - 1, -1, -1))
    with S.Aligner(ref, 0) as al, al.session(shape.n_slots) as se:
        grow(se, order, rng, CHUNK)
        check_case(se, order, gt, 6, [[0], [1], [2], [3], [4, 5], [0, 2, 4]], ref, 2, shape.name, rows_of(se, order, ref, 2), label=lab)


def test_more_than_64_parts():
    """65 parts: the rows kernel's second round of 64.  The single open group holds only the row's last column"""
    shape = K.HUGE
    total = K.total_columns(shape)
    assert K.class_parts(total) == 65
    rng = np.random.default_rng(137)
    ref = _small_ref(rng, shape.lens, True)
    b64 = 64 * K.PART_COLUMNS
    cases = {"the last column": ([(total - 1, total, 0), (0, 100, 1)], 2, [[0], [1], []]),
             "inside part 64": ([(b64 + 3, total - 3, 0), (0, b64 + 3, 1)], 2, [[0], [1]]),
             "part 63 against part 64": ([(b64 - 5000, b64, 0), (b64, total, 1), (0, b64 - 5000, 2)], 3, [[0], [1], [0, 1]])}
    order = [3, 1, 0]
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        grow(se, order, rng, 7)
        rows = rows_of(se, order, ref, 1)
        for name, (spans, n_groups, opens) in cases.items():
            got = check_case(se, order, runs(ref, spans), n_groups, opens, ref, 1, (shape.name, name), rows, label=span_labels(total, spans, n_groups))
            if name == "the last column":
                assert (got[0]["cls"]["on_pos_end"] == int(ref.st_offset[0]) + total - 1).all() and (got[0]["on_group"] == 0).all()
            if name == "inside part 64":
                assert ((got[0]["cls"]["on_pos_end"] - int(ref.st_offset[0])) // K.PART_COLUMNS == 64).all()


# ---- the word edges of the bitmap ----
@pytest.mark.parametrize("n_groups", [32, 33, 65, 1023])
def test_word_edges_of_the_bitmap(n_groups):
    shape = K.WIDE[1]  # rna_8197
    total = K.total_columns(shape)
    rng = np.random.default_rng(139 + n_groups)
    ref = _small_ref(rng, shape.lens, True)
    length = total // n_groups  # every group has a run; what is left over is background
    spans = [(g * length, (g + 1) * length, g) for g in range(n_groups)]
    label = span_labels(total, spans, n_groups)
    edges = [g for g in (31, 32, 63, 64) if g < n_groups]
    order = [2, 1, 0]
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        grow(se, order, rng, CHUNK)
        rows = rows_of(se, order, ref, 1)
        opens = [[g] for g in edges] + [[h for h in range(n_groups) if h != g] for g in edges] + [[n_groups - 1], list(range(n_groups - 1))]
        got = check_case(se, order, runs(ref, spans), n_groups, opens, ref, 1, ("edges", n_groups), rows, label=label)
        for k, g in enumerate(edges):
            assert (got[k]["on_group"] == g).all() and (got[len(edges) + k]["on_group"] != g).all()
        # set bits at or above n_groups are ignored: the background stays closed
        bits = Q.bitmap(n_groups, [edges[0]])
        want = se.open_classes(order, bits)
        if n_groups % 32:
            bits[-1] |= np.uint32(~((1 << (n_groups % 32)) - 1) & 0xffffffff)
            assert se.open_classes(order, bits).tobytes() == want.tobytes()
        with pytest.raises(S.SfaError, match="words"):
            se.open_classes(order, np.zeros(len(bits) + 1, np.uint32))


# ---- ties by construction ----
@pytest.mark.parametrize("shape", [s for s in K.TIES if s.lens[0] in (4, 256, 8192)], ids=lambda s: s.name)
def test_ties(shape):
    """Reference [A, A, one k-mer] with two levels (tests/test_session_class_edges_gpu.py): columns j and |A| + j of a row are the
    same bits.  The twins in an open and a closed group: each class reports its own lowest column.  Both in open groups: the lower
    column wins and on_group is its group."""
    n = shape.lens[0]
    rng = np.random.default_rng(149 + n)
    lv = lambda m: rng.choice(np.array([-0.5, 0.5], np.float32), m)
    a = lv(n)
    ref = S.RefModel(["c0", "c1", "c2"], [n + 5, n + 5, 6], shape.lens, [1, 2, 3], [a, a.copy(), lv(1)], None)
    order = list(range(shape.n_slots))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        grow(se, order, rng, CHUNK, lv)
        rows = rows_of(se, order, ref, 1)
        for sl in order:
            row = rows[sl]
            assert np.array_equal(row[:n].view(np.uint32), row[n:2 * n].view(np.uint32)) and np.isfinite(row).all()
            for j in sorted({int(np.argmin(row[:n])), 0, n - 1, n // 2}):
                # the twins alone in their groups: group 1 holds the lower column
                spans = [(j, j + 1, 1), (n + j, n + j + 1, 0)]
                got = check_case(se, [sl], runs(ref, spans), 2, [[0], [1], [0, 1]], ref, 1, (shape.name, sl, j), rows)
                assert got[0]["cls"]["on_rid"][0] == 1 and got[0]["on_group"][0] == 0 and got[1]["cls"]["on_rid"][0] == 0 and got[1]["on_group"][0] == 1
                assert got[2]["cls"]["on_rid"][0] == 0 and got[2]["cls"]["on_pos_end"][0] == 1 + j and got[2]["on_group"][0] == 1  # both open: the lower column, its group
                # the two copies of A as two groups: equal minima in both classes, each class its own lowest column
                halves = [(0, n, 1), (n, 2 * n, 0)]
                got = check_case(se, [sl], runs(ref, halves), 2, [[0], [1], [0, 1]], ref, 1, (shape.name, sl, "halves"), rows)
                first = int(np.argmin(row[:n]))
                if row[2 * n] > row[first]:
                    assert got[0]["cls"]["on_score"][0] == got[0]["cls"]["off_score"][0] == row[first]
                    assert (got[0]["cls"]["on_rid"][0], got[0]["cls"]["on_pos_end"][0], got[0]["cls"]["off_rid"][0], got[0]["cls"]["off_pos_end"][0]) == (1, 2 + first, 0, 1 + first)
                    assert got[2]["on_group"][0] == 1 and got[2]["cls"]["on_rid"][0] == 0


# ---- classes whose every column costs +inf ----
def test_classes_whose_every_column_costs_inf():
    shape = K.INF
    rng = np.random.default_rng(151)
    base = _small_ref(rng, shape.lens, True)
    fw = [x.copy() for x in base.forward]
    fw[2] = np.full(shape.lens[2], 3e38, np.float32)
    ref = S.RefModel(base.names, base.seq_lengths, base.ref_lengths, base.st_offset, fw, None)
    off = [int(x) for x in ref.st_offset]
    c2 = T.jobs_of(ref.ref_lengths, 1)[2][3]
    order = list(range(shape.n_slots - 1, -1, -1))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        grow(se, order, rng, 9)
        rows = rows_of(se, order, ref, 1)
        for sl in order:
            assert np.isposinf(rows[sl][c2:c2 + 65]).all() and np.isfinite(np.delete(rows[sl], np.arange(c2, c2 + 65))).all()
        # group 0 inside contig 2 (+inf), group 1 without columns, group 2 finite
        spans = [(c2 + 5, c2 + 20, 0), (0, 30, 2)]
        got = check_case(se, order, runs(ref, spans), 3, [[0], [0, 1], [1], [0, 2], [2]], ref, 1, "inf", rows)
        for k in (0, 1):  # ON is +inf at the group's lowest column
            assert np.isposinf(got[k]["cls"]["on_score"]).all() and (got[k]["cls"]["on_rid"] == 2).all() and (got[k]["cls"]["on_pos_end"] == off[2] + 5).all() and (got[k]["on_group"] == 0).all()
            assert (got[k]["cls"]["on_strand"] == ord("+")).all()
        assert (got[2]["cls"]["on_rid"] == -1).all() and (got[2]["on_group"] == -1).all()
        assert np.isfinite(got[3]["cls"]["on_score"]).all() and (got[3]["on_group"] == 2).all()
        # contig 2 is everything that is closed: OFF is +inf at contig 2's first column
        everything = [(*whole(ref, r), r) for r in range(ref.num_ref)]
        got = check_case(se, order, everything, 4, [[0, 1, 3], [2]], ref, 1, "inf, whole contigs", rows)
        assert np.isposinf(got[0]["cls"]["off_score"]).all() and (got[0]["cls"]["off_pos_end"] == off[2]).all() and (got[0]["off_group"] == 2).all()
        assert np.isposinf(got[1]["cls"]["on_score"]).all() and (got[1]["cls"]["on_pos_end"] == off[2]).all() and (got[1]["on_group"] == 2).all()
        for rec in got[0]:  # an OFF class at +inf: on target by any finite margin
            assert S.target_decide(rec["cls"], S.ENRICH, 9, 1e30) == "A" and S.target_decide(rec["cls"], S.ENRICH, 10, 0.0) is None


# ---- a spread session ----
def test_spread_session_on_rows_of_an_odd_width():
    shape = K.SPREAD
    total = K.total_columns(shape)
    rng = np.random.default_rng(157)
    ref = _small_ref(rng, shape.lens, True)
    order = [7, 0, 8, 1, 2, 6, 3]
    slots = list(range(1, shape.n_slots))  # (slot 0 stays empty)
    spans = cyclic(0, total, 5, 40)
    with S.Aligner(ref, flag_of(shape)) as one, S.Aligner(ref, flag_of(shape), devices=[0, 0]) as many:
        with one.session(shape.n_slots) as plain, many.session(shape.n_slots, spread=True) as spread:
            with pytest.raises(S.SfaError, match="no groups"):
                spread.open_classes([1])
            chunks = [_events(rng, CHUNK, True) for _ in slots]
            for se in (plain, spread):
                se.extend(slots, np.concatenate(chunks), offsets(chunks))
            rows = rows_of(plain, order, ref, 1)
            spread.set_target_groups(runs(ref, spans), 40)
            opens = [None, [], [33], list(range(0, 40, 3)), list(range(32))]
            got = check_case(plain, order, runs(ref, spans), 40, opens, ref, 1, "plain", rows, label=span_labels(total, spans, 40))
            for o, want in zip(opens, got):
                assert spread.open_classes(order, None if o is None else Q.bitmap(40, o)).tobytes() == want.tobytes(), o
            with pytest.raises(S.SfaError, match="twice|more than once"):
                spread.open_classes([1, 2, 1])
            with pytest.raises(S.SfaError, match="words"):
                spread.open_classes([1, 2], np.zeros(1, np.uint32))
            with pytest.raises(S.SfaError, match="out of range"):
                spread.open_classes([1, 9])
            spread.open_classes(order)
            plain.open_classes(order)
            assert many.profile()["class_ms"] > 0 and one.profile()["class_ms"] > 0


# ---- slot states, refusals with `out` untouched, a batch between two calls ----
def raw_call(se, slots, bits, n_words, out):
    sl = np.ascontiguousarray(slots, np.int32)
    return se._L.sfa_session_open_classes(se._h, sl.ctypes.data_as(_lib.i32p), len(sl), None if bits is None else bits.ctypes.data_as(C.POINTER(C.c_uint32)), n_words,
                                          out.ctypes.data_as(C.c_void_p))


def test_slot_states_refusals_and_a_batch_in_between():
    shape = K.SMALL[2]
    total = K.total_columns(shape)
    rng = np.random.default_rng(163)
    ref = _small_ref(rng, shape.lens, True)
    spans = cyclic(0, total, 5, 7)
    gt, label = runs(ref, spans), span_labels(total, spans, 7)
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        marked = np.frombuffer(b"\xa5" * (3 * S.OPEN_CLASS_DTYPE.itemsize), S.OPEN_CLASS_DTYPE).copy()
        before = marked.tobytes()
        assert raw_call(se, [1, 2, 3], None, 0, marked) != 0 and marked.tobytes() == before  # no groups
        grow(se, [1, 2, 3, 4], rng, 20)
        se.reset([2])
        poison = np.full(5, np.nan, np.float32)
        se.extend([5], poison, offsets([poison]))
        rows = rows_of(se, [0, 1, 2, 3, 4], ref, 1)
        assert sorted(rows) == [1, 3, 4]
        got = check_case(se, [4, 0, 2, 5, 1, 3], gt, 7, [[0, 3, 6]], ref, 1, "states", rows)[0]
        assert list(got["cls"]["valid"]) == [1, 0, 0, 0, 1, 1]
        bits = Q.bitmap(7, [0, 3, 6])
        two = np.zeros(2, np.uint32)
        for slots, b, nw in (([1, 3, 1], bits, 1), ([1, 9, 3], bits, 1), ([-1, 1, 3], bits, 1), ([1, 3, 4], two, 2), ([1, 3, 4], bits, 0)):
            assert raw_call(se, slots, b, nw, marked) != 0 and marked.tobytes() == before, (slots, nw)
        for bad, b, word in (([1, 3, 1], None, "twice|more than once"), ([9], None, "out of range"), ([-1], None, "out of range"), ([1], two, "words")):
            with pytest.raises(S.SfaError, match=word):
                se.open_classes(bad, b)
        assert raw_call(se, [1, 3, 4], bits, 1, marked) == 0 and marked.tobytes() == got[[4, 5, 0]].tobytes()  # (and a call that is taken writes)
        # a batch on the same context between two calls changes nothing
        first = se.open_classes([1, 3, 4, 2], bits)
        q = _events(rng, 3 * 40, True)
        al.align_db(q, np.array([0, 40, 80, 120], np.int64))
        assert se.open_classes([1, 3, 4, 2], bits).tobytes() == first.tobytes() and first[:3].tobytes() == got[[4, 5, 0]].tobytes()
        check_open(se, [1, 3, 4], 7, bits, label, ref, 1, "after the batch", rows)
        se.set_target_groups([], 5)
        with pytest.raises(S.SfaError, match="no groups"):
            se.open_classes([1])
        # a new table: the lowest columns of the labels are looked for again (a class of +inf columns is not at hand here; the
        # records under the new table are the oracle's)
        spans2 = cyclic(0, total, 9, 4)
        check_case(se, [1, 3, 4], runs(ref, spans2), 4, [[1], [0, 2, 3]], ref, 1, "a second table", rows, label=span_labels(total, spans2, 4))
