"""sfa_session_classes at the rows the first tests do not reach (tests/test_session_targets_gpu.py: one aligned part, u == 0): rows
at every alignment with heads and tails of 0 .. 3 columns and mask shifts 29 .. 31, rows shorter than two quads, rows of several
parts (full, nearly empty and empty last parts, more than 64 of them), costs that tie across lanes, waves, a lane's eight quads and
parts, and classes whose every column costs +inf.  The shapes are tests/class_shapes.py's, and what they reach is asserted without
a GPU in tests/test_class_shapes_cpu.py.  The yardstick is check_classes of the first file: numpy over the rows Session.row() reads
back under tests/targets_oracle.py's mask, scores bit for bit, contig, coordinate and strand equal, after every extend call.
References have levels in quarters (or two levels), events likewise, so that equal costs are common."""
import numpy as np
import pytest

import sigfish_amd as S
from tests import class_shapes as K
from tests import targets_oracle as T
from tests.test_session_gpu import _events, _small_ref
from tests.test_session_targets_gpu import check_classes, offsets, slot_row, whole

pytestmark = pytest.mark.gpu

CHUNKS = (7, 50, 7)


def flag_of(shape):
    return (S.RNA | S.INV) if shape.rna else 0


def strands_of(shape):
    return 1 if shape.rna else 2


def columns(ref, lo, hi):
    """targets for the columns [lo, hi) of a one-strand row (the coordinate of column c of contig r is st_offset[r] + c)"""
    out = []
    for r, _, n, at in T.jobs_of(ref.ref_lengths, 1):
        a, b = max(lo, at), min(hi, at + n)
        if a < b:
            out.append((r, int(ref.st_offset[r]) + a - at, int(ref.st_offset[r]) + b - at))
    return out


def grow(se, slots, rng, n, make=None):
    chunks = [(make or (lambda m: _events(rng, m, True)))(n) for _ in slots]
    return se.extend(slots, np.concatenate(chunks), offsets(chunks))


def check_sets(se, slots, sets, ref, strands, what, wide=False):
    """check_classes under every target list of `sets` (name -> list, or (list, columns the mask must be) to pin the list down)"""
    out = {}
    for name, t in sets.items():
        t, cols = t if isinstance(t, tuple) else (t, None)
        mask = T.mask_of_wide(t, ref.ref_lengths, ref.st_offset, strands) if wide else T.mask_of(t, ref.ref_lengths, ref.st_offset, strands)
        if cols is not None:
            assert list(np.flatnonzero(mask)) == list(cols), (what, name)
        se.set_targets(t)
        out[name] = check_classes(se, slots, t, ref, strands, (what, name), mask=mask)
    return out


# ---- rows at every alignment ----
def edge_sets(ref, shape):
    off, n, total = [int(x) for x in ref.st_offset], [int(x) for x in ref.ref_lengths], K.total_columns(shape)
    sets = {
        # column 0 of the row, the last column of (c3, '+') (one strand: of the row), one column inside a quad, and with two strands
        # column 0 of (c1, '-')
        "first and last columns": [(0, off[0], off[0] + 1), (3, off[3] + n[3] - 1, off[3] + n[3]), (1, off[1] + n[1], off[1] + n[1] + 1), (2, off[2] + 1, off[2] + 2)],
        "everything": [whole(ref, r) for r in range(4)],
        "a contig": [whole(ref, 2)],
        "scattered, unsorted, overlapping": [(3, off[3] + 200, off[3] + 290), (3, off[3] + 10, off[3] + 40), (1, off[1] + 3, off[1] + 33), (3, off[3] + 30, off[3] + 64),
                                             (0, off[0] + 36, off[0] + 38)],
    }
    if shape.rna:  # the on class is the three columns a head or a tail can have, then one of them: the winner is the head's or tail's
        sets["head columns"] = (columns(ref, 0, 3), range(3))
        sets["tail columns"] = (columns(ref, total - 3, total), range(total - 3, total))
        sets["column 1"] = (columns(ref, 1, 2), [1])
        sets["last column but one"] = (columns(ref, total - 2, total - 1), [total - 2])
        sets["nothing"] = [(r, 0, off[r]) for r in range(4)]  # (st_offset is 1 .. 3: coordinates below it belong to no column)
    else:
        sets["both ends of the row"] = [(0, off[0], off[0] + 3), (3, off[3] + 1, off[3] + 4)]  # with (c0, '-') and (c3, '+') columns
    return sets


@pytest.mark.parametrize("shape", K.SMALL, ids=[s.name for s in K.SMALL])
def test_rows_at_every_alignment(shape):
    rng = np.random.default_rng(23 + K.total_columns(shape))
    ref = _small_ref(rng, shape.lens, shape.rna)
    strands = strands_of(shape)
    sets = edge_sets(ref, shape)
    order = list(range(shape.n_slots - 1, -1, -1))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        for step, n in enumerate(CHUNKS):
            grow(se, order, rng, n)
            got = check_sets(se, order, sets, ref, strands, (shape.name, step))
            assert all((g["valid"] == 1).all() for g in got.values())
            assert (got["everything"]["off_rid"] == -1).all() and np.isinf(got["everything"]["off_score"]).all()
            if shape.rna:
                assert (got["nothing"]["on_rid"] == -1).all() and np.isinf(got["nothing"]["on_score"]).all()
                assert (got["column 1"]["on_rid"] == 0).all() and (got["column 1"]["on_pos_end"] == int(ref.st_offset[0]) + 1).all()
                assert (got["last column but one"]["on_rid"] == 3).all()


# ---- rows shorter than two quads ----
@pytest.mark.parametrize("shape", K.TINY, ids=[s.name for s in K.TINY])
def test_tiny_rows(shape):
    """one contig of 1 .. 7 k-mers: a head that is the whole row, rows without a body, a tail without a body"""
    n = shape.lens[0]
    rng = np.random.default_rng(31 + n)
    ref = _small_ref(rng, shape.lens, True)
    sets = {"everything": [whole(ref, 0)], "nothing": [(0, 0, int(ref.st_offset[0]))]}
    for c in range(n):
        sets[f"column {c}"] = (columns(ref, c, c + 1), [c])
    if n > 2:
        sets["all but the ends"] = (columns(ref, 1, n - 1), range(1, n - 1))
    order = list(range(shape.n_slots - 1, -1, -1))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        for step, m in enumerate(CHUNKS):
            grow(se, order, rng, m)
            got = check_sets(se, order, sets, ref, 1, (shape.name, step))
            assert all((g["valid"] == 1).all() for g in got.values())
            for c in range(n):  # one column on target: it is the winner whatever it costs, and every other column is off target
                g = got[f"column {c}"]
                assert (g["on_pos_end"] == int(ref.st_offset[0]) + c).all() and ((g["off_rid"] == 0).all() if n > 1 else (g["off_rid"] == -1).all())


# ---- rows of several parts ----
def part_sets(ref, shape):
    """one interval inside every part in turn, the columns around every part boundary, everything"""
    total, strands = K.total_columns(shape), strands_of(shape)
    sets = {"everything": [whole(ref, r) for r in range(ref.num_ref)]}
    parts = K.class_parts(total)
    if shape.rna:
        for p in range(parts):
            lo, hi = K.part_interior(total, p)
            if lo < hi:
                sets[f"inside part {p}"] = (columns(ref, lo, hi), range(lo, hi))
        for p in range(1, parts):  # for a slot with a head of h columns part p begins at column p * 8192 + h
            b = p * K.PART_COLUMNS
            sets[f"boundary {p} - 1 .. + 1"] = (columns(ref, b - 1, b + 2), range(b - 1, b + 2))
            sets[f"boundary {p} + 2 .. + 4"] = (columns(ref, b + 2, b + 5), range(b + 2, b + 5))
            sets[f"column {b - 1}"] = (columns(ref, b - 1, b), [b - 1])
            sets[f"column {b}"] = (columns(ref, b, b + 1), [b])
        sets["last quads"] = (columns(ref, total - 9, total), range(total - 9, total))
    else:  # two strands: contig r is inside part r on both (class_shapes.WIDE), a few columns away from its ends
        for r in range(ref.num_ref):
            t = [(r, int(ref.st_offset[r]) + 4, int(ref.st_offset[r]) + int(ref.ref_lengths[r]) - 3)]
            cols = np.flatnonzero(T.mask_of_wide(t, ref.ref_lengths, ref.st_offset, strands))
            lo, hi = K.part_interior(total, r)
            assert len(cols) > 0 and lo <= cols[0] and cols[-1] < hi
            sets[f"inside part {r}"] = t
        sets["contig ends"] = [(r, int(ref.st_offset[r]), int(ref.st_offset[r]) + 2) for r in range(ref.num_ref)]  # columns on either side of boundaries
    return sets


@pytest.mark.parametrize("shape", K.WIDE, ids=[s.name for s in K.WIDE])
def test_rows_of_several_parts(shape):
    rng = np.random.default_rng(41 + K.total_columns(shape))
    ref = _small_ref(rng, shape.lens, shape.rna)
    strands = strands_of(shape)
    sets = part_sets(ref, shape)
    # (8197 columns: part 1 has one quad or none, no column of it is a body column of every slot; the boundary sets are its)
    assert sum(name.startswith("inside part") for name in sets) == K.class_parts(K.total_columns(shape)) - (shape.name == "rna_8197") >= 1
    order = list(range(shape.n_slots - 1, -1, -1))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        for step, n in enumerate(CHUNKS[:2]):
            grow(se, order, rng, n)
            got = check_sets(se, order, sets, ref, strands, (shape.name, step), wide=True)
            assert all((g["valid"] == 1).all() for g in got.values())


def test_more_than_64_parts():
    """524 301 columns, 65 parts: the rows kernel merges part 64 in a lane's second round.  The on class is confined to parts 0, 1,
    63 and 64 in turn (the oracle's argmin runs over the class's columns only)."""
    shape = K.HUGE
    total = K.total_columns(shape)
    rng = np.random.default_rng(43)
    ref = _small_ref(rng, shape.lens, True)
    sets = {"everything": [whole(ref, 0)]}
    for p in (0, 1, 63, 64):
        lo, hi = K.part_interior(total, p)
        sets[f"inside part {p}"] = (columns(ref, lo, hi), range(lo, hi))
    b = 64 * K.PART_COLUMNS
    sets["boundary 64 - 1 .. + 1"] = (columns(ref, b - 1, b + 2), range(b - 1, b + 2))
    sets["last quads"] = (columns(ref, total - 9, total), range(total - 9, total))
    order = list(range(shape.n_slots - 1, -1, -1))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        for step, n in enumerate(CHUNKS[:2]):
            grow(se, order, rng, n)
            got = check_sets(se, order, sets, ref, 1, (shape.name, step), wide=True)
            assert all((g["valid"] == 1).all() for g in got.values())
            for p in (0, 1, 63, 64):  # (said once more: the on-target winner is a column of that part)
                assert ((got[f"inside part {p}"]["on_pos_end"] - int(ref.st_offset[0])) // K.PART_COLUMNS == p).all()


# ---- ties by construction ----
@pytest.mark.parametrize("shape", K.TIES, ids=[s.name for s in K.TIES])
def test_ties_across_lanes_waves_quads_and_parts(shape):
    """Reference [A, A, one k-mer], two levels: contig 1's levels are contig 0's, and a column's cost depends on the levels up to its
    own and on the events only, so column j and column |A| + j of a slot's row are the same bits.  The on class is exactly these two
    columns: the lower one must win.  Where the twin sits: tests/test_class_shapes_cpu.py."""
    n = shape.lens[0]
    rng = np.random.default_rng(47 + n)
    lv = lambda m: rng.choice(np.array([-0.5, 0.5], np.float32), m)
    a = lv(n)
    ref = S.RefModel(["c0", "c1", "c2"], [n + 5, n + 5, 6], shape.lens, [1, 2, 3], [a, a.copy(), lv(1)], None)
    js = sorted({0, 1, 2, 3, n // 2 + 1, n - 2, n - 1} & set(range(n)))
    sets = {f"columns {j} and {n + j}": ([(0, 1 + j, 2 + j), (1, 2 + j, 3 + j)], [j, n + j]) for j in js}
    order = list(range(shape.n_slots))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        for step, m in enumerate(CHUNKS[:2]):
            grow(se, order, rng, m, lv)
            for sl in order:  # the inputs really tie
                row = slot_row(se, sl, 1, 3)
                assert np.array_equal(row[:n].view(np.uint32), row[n:2 * n].view(np.uint32)) and np.isfinite(row).all(), (shape.name, step, sl)
            got = check_sets(se, order, sets, ref, 1, (shape.name, step), wide=n >= 1024)
            for j in js:  # (check_classes has compared these with numpy's first minimum; said once more)
                g = got[f"columns {j} and {n + j}"]
                assert (g["on_rid"] == 0).all() and (g["on_pos_end"] == 1 + j).all() and (g["valid"] == 1).all(), (shape.name, step, j)


# ---- classes whose every column costs +inf ----
def last_row(events, levels):
    """the subsequence DTW's last row in numpy, float32 cell by cell: |x - y| + min(up, diagonal, left), row 0 starts anywhere"""
    prev = None
    inf = np.float32(np.inf)
    with np.errstate(over="ignore"):
        for x in np.asarray(events, np.float32):
            d = np.abs(x - np.asarray(levels, np.float32))
            cur = np.empty_like(d)
            for j in range(len(d)):
                m = np.float32(0) if prev is None else min(prev[j], prev[j - 1] if j else inf, cur[j - 1] if j else inf)
                cur[j] = d[j] + m
            prev = cur
    return prev


def test_classes_whose_every_column_costs_inf():
    """Contig 2's levels are 3e38: a cell costs about 3e38 (finite), two of them overflow, so from the second event on every
    column of contig 2 costs +inf -- never NaN, nothing is subtracted from an infinity -- while the other contigs stay finite.  No
    column is less than the initial +inf of a partial minimum, and the record names the lowest column of the class."""
    shape = K.INF
    rng = np.random.default_rng(53)
    base = _small_ref(rng, shape.lens, True)
    fw = [x.copy() for x in base.forward]
    fw[2] = np.full(shape.lens[2], 3e38, np.float32)
    ref = S.RefModel(base.names, base.seq_lengths, base.ref_lengths, base.st_offset, fw, None)
    off = [int(x) for x in ref.st_offset]
    data = {sl: _events(rng, 9, True) for sl in range(shape.n_slots)}
    # on the CPU first: finite after one event, +inf and no NaN from the second on; the other contigs finite
    for sl in data:
        one, two, nine = (last_row(data[sl][:m], fw[2]) for m in (1, 2, 9))
        assert np.isfinite(one).all() and (one > 2.9e38).all() and np.isposinf(two).all() and np.isposinf(nine).all()
        assert np.isfinite(last_row(data[sl], fw[1])).all()
    c2 = T.jobs_of(ref.ref_lengths, 1)[2][3]
    sets = {"contig 2": [whole(ref, 2)], "all but contig 2": [whole(ref, r) for r in (0, 1, 3)], "inside contig 2": (columns(ref, c2 + 5, c2 + 20), range(c2 + 5, c2 + 20)),
            "all but inside contig 2": [whole(ref, r) for r in (0, 1, 3)] + columns(ref, c2, c2 + 5) + columns(ref, c2 + 20, c2 + 65),
            "contig 2 and a column of contig 1": [whole(ref, 2), (1, off[1] + 63, off[1] + 64)], "everything": [whole(ref, r) for r in range(4)]}
    order = list(range(shape.n_slots - 1, -1, -1))
    with S.Aligner(ref, flag_of(shape)) as al, al.session(shape.n_slots) as se:
        used = 0
        for step, m in enumerate((1, 1, 7)):
            chunks = [data[sl][used:used + m] for sl in order]
            se.extend(order, np.concatenate(chunks), offsets(chunks))
            used += m
            for sl in order:  # the device's row of contig 2 is the CPU's
                assert np.array_equal(se.row(sl, 2, "+")[0].view(np.uint32), last_row(data[sl][:used], fw[2]).view(np.uint32)), (step, sl)
            got = check_sets(se, order, sets, ref, 1, ("inf", step))
            assert all((g["valid"] == 1).all() and (g["n_events"] == used).all() for g in got.values())
            on, off_side, inside, outside = got["contig 2"], got["all but contig 2"], got["inside contig 2"], got["all but inside contig 2"]
            if step == 0:
                assert np.isfinite(on["on_score"]).all() and (on["on_score"] > 2.9e38).all()
                continue
            # the class's lowest column: column 0 of contig 2 (coordinate st_offset), or column 5 of it
            for g, side, other, coord in ((on, "on", "off", off[2]), (off_side, "off", "on", off[2]), (inside, "on", "off", off[2] + 5), (outside, "off", "on", off[2] + 5)):
                assert np.isposinf(g[f"{side}_score"]).all() and (g[f"{side}_rid"] == 2).all() and (g[f"{side}_pos_end"] == coord).all(), (step, side, g)
                assert (g[f"{side}_strand"] == ord("+")).all() and np.isfinite(g[f"{other}_score"]).all() and (g[f"{other}_rid"] != 2).all(), (step, side, g)
            assert np.isfinite(got["contig 2 and a column of contig 1"]["on_score"]).all() and (got["contig 2 and a column of contig 1"]["on_rid"] == 1).all()
            # the decision (target_rules.hpp: target_class_of): +inf on target against a finite cost off target is off target at every
            # margin, and the other way round; below min_events there is none
            for rec in on:
                assert S.target_decide(rec, S.ENRICH, used, 0.0) == "U" and S.target_decide(rec, S.DEPLETE, used, 1e30) == "A"
                assert S.target_decide(rec, S.ENRICH, used + 1, 0.0) is None
            for rec in off_side:
                assert S.target_decide(rec, S.ENRICH, used, 1e30) == "A" and S.target_decide(rec, S.DEPLETE, used, 0.0) == "U"


# ---- a spread session ----
def test_spread_session_on_rows_of_an_odd_width():
    """global slot i is slot i // 2 of sub-session i % 2: its row begins at another alignment there, and the answers are the same bytes"""
    shape = K.SPREAD
    total = K.total_columns(shape)
    rng = np.random.default_rng(59)
    ref = _small_ref(rng, shape.lens, True)
    sets = edge_sets(ref, shape)
    order = [7, 0, 8, 1, 2, 6, 3]
    assert total % 2 == 1 and sum(K.layout(total, i).offset != K.layout(total, i // 2).offset for i in order) >= 4
    slots = list(range(1, shape.n_slots))  # (slot 0 stays empty)
    with S.Aligner(ref, flag_of(shape)) as one, S.Aligner(ref, flag_of(shape), devices=[0, 0]) as many:
        with one.session(shape.n_slots) as plain, many.session(shape.n_slots, spread=True) as spread:
            for step, n in enumerate(CHUNKS[:2]):
                chunks = [_events(rng, n, True) for _ in slots]
                for se in (plain, spread):
                    se.extend(slots, np.concatenate(chunks), offsets(chunks))
                for name, t in sets.items():
                    t = t[0] if isinstance(t, tuple) else t
                    for se in (plain, spread):
                        se.set_targets(t)
                    assert spread.target_columns() == plain.target_columns()
                    want = check_classes(plain, order, t, ref, 1, ("plain", name, step))
                    assert spread.classes(order).tobytes() == want.tobytes(), (name, step)
            assert many.profile()["class_ms"] > 0 and one.profile()["class_ms"] > 0
