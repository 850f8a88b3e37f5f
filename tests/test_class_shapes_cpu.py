"""What the shapes of tests/class_shapes.py reach in the two kernels of sdtw_session_class.hpp, from the documented layout alone
(no GPU, no library call): the claims tests/test_session_class_edges_gpu.py rests on are asserted here, so a shape table that stops
reaching a head, a mask shift, a `u` or a part fails in this file."""
import numpy as np

from tests import class_shapes as K
from tests import targets_oracle as T


def layouts(shape):
    total = K.total_columns(shape)
    return [K.layout(total, sl) for sl in range(shape.n_slots)]


def test_the_layout_function_on_rows_worked_out_by_hand():
    # 466 columns, slot 1: 466 words behind a boundary = 2 (mod 4), two head columns, 116 quads, no tail
    assert K.layout(466, 1) == K.Layout(2, 2, 116, 0, 1, [116], {2, 6, 10, 14, 18, 22, 26, 30})
    assert K.layout(466, 2)[:4] == (0, 0, 116, 2)
    # one column in slot 1 of one-column rows: the head would be 3 columns but the row ends first
    assert K.layout(1, 1)[:4] == (1, 1, 0, 0) and K.layout(1, 0)[:4] == (0, 0, 0, 1)
    assert K.layout(5, 1)[:4] == (1, 3, 0, 2) and K.layout(7, 3)[:4] == (1, 3, 1, 0)
    # parts count total / 4 quads, whatever the head takes away
    assert K.class_parts(8192) == 1 and K.class_parts(8195) == 1 and K.class_parts(8196) == 2 and K.class_parts(3) == 1
    assert K.layout(8197, 1).part_quads == [2048, 0] and K.layout(8197, 0).part_quads == [2048, 1]
    assert K.us_of(0) == set() and K.us_of(256) == {0} and K.us_of(257) == {0, 1} and K.us_of(2048) == set(range(8))
    assert K.waves_of(12) == {0} and K.waves_of(64) == {0} and K.waves_of(65) == {0, 1} and K.waves_of(193) == {0, 1, 2, 3}
    assert K.seat(466, 1, 1) == ("head", 1) and K.seat(466, 2, 465) == ("tail", 65) and K.seat(466, 1, 2) == ("body", 0, 0, 0, 0)
    assert K.seat(16385, 0, 8192 + 4 * 300) == ("body", 1, 1, 0, 44)


def test_what_the_existing_shapes_reach():
    """tests/test_session_targets_gpu.py: 932 columns (DNA) and 466 (RNA), 9 slots -- what its docstring says"""
    dna, rna = [K.layout(932, sl) for sl in range(9)], [K.layout(466, sl) for sl in range(9)]
    assert {x.offset for x in dna} == {0} and {(x.head, x.tail) for x in dna} == {(0, 0)}
    assert {x.offset for x in rna} == {0, 2} and {(x.head, x.tail) for x in rna} == {(0, 2), (2, 0)}
    for x in dna + rna:
        assert x.parts == 1 and K.us_of(x.part_quads[0]) == {0} and not x.shifts & {29, 31}
    assert 30 in rna[1].shifts


def test_small_shapes_reach_every_alignment():
    pairs, heads, tails, shifts, head_tail = set(), set(), set(), set(), set()
    for shape in K.SMALL:
        total = K.total_columns(shape)
        for x in layouts(shape):
            pairs.add((x.offset, total % 4))
            heads.add(x.head)
            tails.add(x.tail)
            head_tail.add((x.head, x.tail))
            shifts |= x.shifts
            assert x.parts == 1 and x.nq > 64  # (a body in more than one wave; parts and `u` are the wide shapes')
    # every pair that exists: an even total cannot put a row at an odd offset (11 of the 16 combinations)
    assert pairs == K.reachable_pairs() and len(pairs) == 11
    assert {o for o, _ in pairs} == {0, 1, 2, 3} and {t for _, t in pairs} == {0, 1, 2, 3}
    assert heads == {0, 1, 2, 3} and tails == {0, 1, 2, 3}
    assert head_tail == {((4 - o) % 4, (t - (4 - o)) % 4) for o, t in K.reachable_pairs()} and len(head_tail) == 11
    assert {29, 30, 31} <= shifts
    assert [K.total_columns(s) for s in K.SMALL] == [465, 466, 467, 468, 930]
    assert not K.SMALL[4].rna and K.total_columns(K.SMALL[4]) % 4 == 2


def test_tiny_shapes_have_rows_without_a_body():
    seen = set()
    for shape in K.TINY:
        for x in layouts(shape):
            assert x.parts == 1 and x.nq <= 1 and x.head + 4 * x.nq + x.tail == K.total_columns(shape)
            seen.add(("whole row is head", x.head == K.total_columns(shape) and x.head > 0))
            seen.add(("no body", x.nq == 0))
            seen.add(("tail, no body", x.nq == 0 and x.tail > 0))
            seen.add(("head and tail, no body", x.nq == 0 and x.tail > 0 and x.head > 0))
            seen.add(("one quad between head and tail", x.nq == 1 and x.head > 0 and x.tail > 0))
    assert all((name, True) in seen for name, _ in seen), sorted(seen)
    assert [K.total_columns(s) for s in K.TINY] == [1, 2, 3, 5, 6, 7]


def test_wide_shapes_reach_every_u_wave_and_kind_of_last_part():
    by = {s.name: layouts(s) for s in K.WIDE}
    a, b, c, d = by["rna_16385"], by["rna_8197"], by["rna_16433"], by["dna_20006"]
    assert a[0].part_quads == [2048, 2048] and a[0].head == 0 and a[0].tail == 1  # a full last part
    assert [x.nq for x in a] == [4096, 4095, 4095, 4096, 4096] and {x.head for x in a} == {0, 1, 2, 3}  # (head 1 leaves 16384 columns)
    assert b[0].part_quads == [2048, 1] and b[1].head == 3 and b[1].part_quads == [2048, 0]  # an empty last part
    assert c[0].parts == 3 and c[0].part_quads == [2048, 2048, 12] and K.waves_of(12) == {0}  # under 64 quads: waves 1..3 have nothing
    assert d[0].parts == 3 and {x.offset for x in d} == {0, 2} and 64 < d[0].part_quads[2] < 2048
    for x in a + b + c + d:
        assert K.us_of(x.part_quads[0]) == set(range(8)) and K.waves_of(x.part_quads[0]) == {0, 1, 2, 3}
        assert x.part_quads[0] == 2048 and sum(x.part_quads) == x.nq
    # a last part that stops inside a lane's eight quads
    assert K.us_of(d[0].part_quads[2]) == {0, 1, 2, 3} and K.us_of(a[1].part_quads[1]) == set(range(8)) and a[1].part_quads[1] == 2047
    # the intervals the GPU test confines the on class with lie in one part for every slot
    for shape in K.WIDE + [K.HUGE]:
        total = K.total_columns(shape)
        for p in range(K.class_parts(total)):
            lo, hi = K.part_interior(total, p)
            if lo >= hi:
                continue
            for sl in range(shape.n_slots):
                assert {K.seat(total, sl, g)[:2] for g in (lo, hi - 1)} == {("body", p)}, (shape.name, p, sl)


def test_huge_shape_has_more_than_64_parts():
    x = layouts(K.HUGE)
    assert all(y.parts == 65 for y in x) and {y.head for y in x} == {0, 1, 2, 3}
    assert x[0].part_quads[63:] == [2048, 3] and x[1].part_quads[64] == 2  # (part 64 is the second round of lane 0 in the rows kernel)
    assert all(K.part_interior(K.total_columns(K.HUGE), p)[0] < K.part_interior(K.total_columns(K.HUGE), p)[1] for p in (0, 1, 63, 64))


def test_where_the_twin_of_a_tied_column_sits():
    """reference [A, A, one k-mer]: the twin of column j is column |A| + j, |A| / 4 quads further"""
    want = {4: "next lane", 256: "next wave", 1024: "next u", 8192: "next part"}
    for shape in K.TIES:
        n, total = shape.lens[0], K.total_columns(shape)
        seen = set()
        for sl in range(shape.n_slots):
            for j in range(n):
                a, b = K.seat(total, sl, j), K.seat(total, sl, n + j)
                if a[0] != "body" or b[0] != "body":
                    seen.add(f"{a[0]} and {b[0]}")
                    continue
                _, pa, ua, wa, la = a
                _, pb, ub, wb, lb = b
                if (pb, ub, wb, lb) == (pa, ua, wa, la + 1):
                    seen.add("next lane")
                elif (pb, ub, lb) == (pa, ua, la) and wb == wa + 1:
                    seen.add("next wave")
                elif (pb, wb, lb) == (pa, wa, la) and ub == ua + 1:
                    seen.add("next u")
                elif (ub, wb, lb) == (ua, wa, la) and pb == pa + 1:
                    seen.add("next part")
                else:
                    seen.add("other")
        assert want[n] in seen, (shape.name, seen)
        assert total % 4 == 1 and "head and body" in seen, (shape.name, seen)  # (the twin of a head column is a body column)
        assert K.seat(total, 0, 0) == ("body", 0, 0, 0, 0) and K.seat(total, 1, 0) == ("head", 0)


def test_vectorised_mask_is_the_per_column_one():
    lens, offs = [1, 31, 32, 33, 64, 65, 300], [0, 7, 0, 100, 3, 0, 1000]
    lists = [[], [(r, offs[r], offs[r] + lens[r] + 1) for r in range(7)], [(6, 1200, 1260), (6, 1010, 1040), (3, 105, 120), (0, 0, 2), (4, 34, 36), (3, 0, 100)]]
    for strands in (1, 2):
        for t in lists:
            assert np.array_equal(T.mask_of_wide(t, lens, offs, strands), T.mask_of(t, lens, offs, strands)), (strands, t)
    assert T.mask_of_wide(lists[2], lens, offs, 2).any()
