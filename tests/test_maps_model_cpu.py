"""The numpy model of an event map (tests/maps_model.py) against the host routine sfa_r2qevent_map (band_traceback + path_to_pairs,
host/sam.cpp) on every row of tests/map_bands.py -- bands the caller wrote, not the aligner -- and on aligner-shaped rows; and
what the table claims to reach, asserted here so that it holds before tests/test_event_maps_bands_gpu.py runs on a device.
Maps are integers and the costs behind them the same float32 operations: every comparison is exact."""
import numpy as np
import pytest

import sigfish_amd as S
from oracle import oracle as O
from tests import map_bands as B
from tests import maps_model as M

ALL = [(n, v) for n in B.CASES for v in B.VARIANTS]


def host_map(ref, flag, x, row):
    """sfa_r2qevent_map of one row for the events x (event order); None where it refuses (no complete map)"""
    ev = np.zeros(len(x), S.EVENT_DTYPE)
    ev["mean"] = x
    j = int(row["rid"])
    y = ref.forward[j] if row["strand"] == ord("+") else ref.reverse[j]
    try:
        return S.r2qevent_map(row, ev, 0, len(x), y, int(ref.st_offset[j]), flag)
    except S.SfaError:
        return None


def assert_same(got, want, what):
    if want is None:
        assert got is None, what  # the host routine must have raised
    else:
        assert got is not None and got.dtype == np.int32 and np.array_equal(got, want), (what, None if got is None else got[:6], want[:6])


def assert_is_an_alignment(mp, qlen, what):
    """a complete map read as an alignment: the columns that hold query rows hold them in order, without a gap, from 0 to qlen - 1"""
    held = mp[mp[:, 0] >= 0]
    assert (mp[mp[:, 0] < 0] == -1).all() and (held[:, 0] <= held[:, 1]).all(), what
    assert held[0, 0] == 0 and held[-1, 1] == qlen - 1, what
    assert (np.diff(held[:, 1]) >= 0).all(), what
    # the next column that holds rows starts one row on (a column entered without advancing in the query has lost that point)
    assert (held[1:, 0] - held[:-1, 1] == 1).all(), what
    assert mp[0, 0] == 0, what  # the path's first column is never blank


@pytest.mark.parametrize("name,variant", ALL)
def test_model_equals_host_routine(name, variant):
    case, b = B.CASES[name], B.build(name, variant)
    ref = B.ref_model(b)
    want = B.model_maps(name, variant)
    for k, band in enumerate(case.bands):
        x = b.q[b.q_off[band.read]:b.q_off[band.read + 1]]
        assert_same(host_map(ref, case.flag, x, b.rows[k]), want[k], (name, variant, k, band))
        if want[k] is not None:
            assert len(want[k]) == band.m
            assert_is_an_alignment(want[k], len(x), (name, variant, k, band))


@pytest.mark.parametrize("name", ["array_edges_dna", "no_map_between_maps", "rna_reversed", "rna_invert", "rna_dtw_std", "forty_rows_one_read"])
@pytest.mark.parametrize("variant", B.VARIANTS)
def test_aligner_shaped_rows(name, variant):
    """rows as the aligner reports them (the CPU oracle's, over the case's reference and queries): band of the optimum"""
    case, b = B.CASES[name], B.build(name, variant)
    ref = B.ref_model(b)
    rows = O.align_batch(b.q, b.q_off, O.RefSynth(b.names, b.seq_lengths, b.ref_lengths, b.st_offset, b.forward, b.reverse), case.flag, threads=4)
    n_maps = 0
    for i, row in enumerate(rows):
        assert row["valid"] and row["rid"] >= 0
        x = b.q[b.q_off[i]:b.q_off[i + 1]]
        want = M.row_map(row, x, b.forward, b.reverse, b.st_offset, bool(case.flag & S.RNA), bool(case.flag & S.INV), bool(case.flag & S.DTW))
        assert_same(host_map(ref, case.flag, x, row), want, (name, variant, i, row))
        if want is not None:
            n_maps += 1
            assert_is_an_alignment(want, len(x), (name, variant, i))
    # pos_st is the column in which the aligner's own walk left query row 0, so the band's walk ends there too unless the band's
    # first column, which continues from above only, changes a tie on the way; on these inputs (fixed seeds) it never does, with
    # --dtw-std either: every row has its map
    assert n_maps == len(rows)


def test_rows_report_their_bands():
    """the row <-> columns conversion, on hand-worked figures (src/sigfish.c:971-975): '-' flips about rlen, not rlen - 1"""
    assert M.row_positions(0, 1499, True, 1500, 0) == (0, 1499) and M.row_positions(0, 1499, False, 1500, 0) == (1, 1500)
    assert M.row_positions(10, 19, False, 100, 3) == (84, 93) and M.row_columns(84, 93, False, 100, 3) == (10, 19)
    assert M.row_columns(13, 22, True, 100, 3) == (10, 19)
    for name in B.CASES:
        case, b = B.CASES[name], B.build(name, "quantised")
        assert (b.rows["valid"] == 1).all() and len(b.rows) == len(b.read_of_row) == len(case.bands)
        for k, band in enumerate(case.bands):
            plus = band.strand == "+"
            assert M.row_columns(int(b.rows["pos_st"][k]), int(b.rows["pos_end"][k]), plus, case.lens[band.contig], case.offs[band.contig]) == \
                (band.col_st, band.col_st + band.m - 1)


# ---- what the table reaches ----

@pytest.mark.parametrize("name,variant", ALL)
def test_planted_rows_have_maps_and_random_ones_none(name, variant):
    case = B.CASES[name]
    maps = B.model_maps(name, variant)
    planted = [k for k, band in enumerate(case.bands) if band.planted]
    random = [k for k, band in enumerate(case.bands) if not band.planted]
    assert planted and 4 * sum(maps[k] is not None for k in planted) >= 3 * len(planted), (name, variant)
    if random:
        assert all(case.bands[k].m >= case.qlens[case.bands[k].read] for k in random)
        assert 4 * sum(maps[k] is None for k in random) >= 3 * len(random), (name, variant)
        # ... and each such row stands between planted ones
        assert all(0 < k < len(case.bands) - 1 for k in random)
    if name == "no_map_between_maps":
        assert len(random) >= 12 and any(case.bands[k + 1].planted and case.bands[k - 1].planted for k in random)


def test_every_class_has_its_widths_and_step_residues():
    seen = {}
    for name in B.TABLE:
        for band in B.CASES[name].bands:
            q = B.CASES[name].qlens[band.read]
            seen.setdefault(B.shape_of(q), set()).add((q, band.m))
    assert set(seen) == {(R, L) for R, L, _ in B.CLASSES}
    lo = 0
    for R, L, most in B.CLASSES:
        pairs = seen[(R, L)]
        for q in (x for x in B.EDGE_QLENS if lo < x <= most):
            for m in (1, 2, 3, 4, 5, 7, 8, L - 1, L, L + 1, max(q // 2, 1), q, min(2 * q, 2100)):
                assert (q, m) in pairs, (R, L, q, m)
        assert {(m + L - 1) % 4 for _, m in pairs} == {0, 1, 2, 3}, (R, L)
        lo = most
    # a wave runs max(m) + L - 1 steps in groups of four, m over the 64 / L rows it holds: rows of a case reach their class's launch in
    # input order (one slice under the default budget), 64 / L to a wave.  Every remainder, per class, as a wave's step count
    steps = {}
    for name in B.TABLE:
        case, by_class = B.CASES[name], {}
        for band in case.bands:
            by_class.setdefault(B.shape_of(case.qlens[band.read]), []).append(band.m)
        for (R, L), ms in by_class.items():
            for w in range(0, len(ms), 64 // L):
                steps.setdefault((R, L), set()).add((max(ms[w:w + 64 // L]) + L - 1) % 4)
    assert all(steps[(R, L)] == {0, 1, 2, 3} for R, L, _ in B.CLASSES), steps
    assert {q for q in B.EDGE_QLENS} == {q for ps in seen.values() for q, _ in ps if q in B.EDGE_QLENS}
    # the largest single fill
    assert max(q * m for ps in seen.values() for q, m in ps) == 2048 * 2100


def test_mixed_waves_hold_what_they_claim():
    for name, counts in (("mixed_one_row", (1, 1, 1)), ("mixed_block_less_one", (15, 7, 3)), ("mixed_block", (16, 8, 4)), ("mixed_block_plus_one", (17, 9, 5))):
        case = B.CASES[name]
        by_class = {}
        for band in case.bands:
            by_class.setdefault(B.shape_of(case.qlens[band.read]), []).append(band.m)
        for (R, L), n in zip(((4, 16), (32, 16), (32, 32), (32, 64)), (counts[0], counts[0], counts[1], counts[2])):
            ms = by_class[(R, L)]
            assert len(ms) == n and n in (1, B.per_block(L) - 1, B.per_block(L), B.per_block(L) + 1)
            if n >= 4:  # the slots of the first wave (L = 64: the first waves), in launch order
                assert (ms[0], ms[2]) == ((1, 3) if L != 32 else (1, 1)) and min(ms[1], ms[3]) > 10 * ms[2]
        sizes = sorted(B.row_bytes(case.qlens[band.read], band.m) for band in case.bands)
        assert len(sizes) == 1 or sizes[-1] > sizes[-2] or name == "mixed_one_row"


def test_array_edges_are_edges():
    case = B.CASES["array_edges_dna"]
    ends = {(band.contig, band.strand) for band in case.bands if band.col_st + band.m == case.lens[band.contig]}
    begins = {(band.contig, band.strand) for band in case.bands if band.col_st == 0}
    last = len(case.lens) - 1
    assert {(last, "+"), (last, "-"), (2, "+"), (2, "-")} <= ends and {(2, "+"), (2, "-"), (last, "+"), (last, "-")} <= begins
    assert any(band.col_st == 0 and band.m == case.lens[band.contig] for band in case.bands)  # a contig as short as its band
    assert case.offs[2] != 0 and case.offs[last] != 0
    case = B.CASES["forty_rows_one_read"]
    of_read_1 = [band for band in case.bands if band.read == 1]
    assert len(of_read_1) == 40 and len(set(of_read_1)) == 39 and len({(b.contig, b.strand, b.col_st) for b in of_read_1}) == 39
    for name in ("rna_reversed",):  # a reversed query whose length is no multiple of the rows per lane
        assert sum(q % B.shape_of(q)[0] != 0 for q in B.CASES[name].qlens) >= 5
    for name in B.STRIPS:
        case = B.CASES[name]
        assert all(q > B.MAX_QUERY for q in case.qlens)
        assert all(band.m <= 65 or (band.m, case.qlens[band.read]) == (2049, 2049) for band in case.bands)
    assert set(B.CASES["strips_dna"].qlens) == {2049, 4096, 4097, 6145}
    assert {band.m for band in B.CASES["strips_dna"].bands} == {1, 2, 5, 63, 64, 65, 2049}


@pytest.mark.parametrize("variant", B.VARIANTS)
def test_dtw_std_bands_depend_on_their_prefix(variant):
    """--dtw-std: the running sum of the columns in front of a band shifts every cost of the band, so it shows in a map only through
    rounding.  The bands behind a spike are built so that it does: without the last column in front of the band (its level replaced
    by the query's first event, which adds exactly 0) the model gives another map behind every HUGE spike and behind some SPIKE."""
    case, b = B.CASES["rna_dtw_std"], B.build("rna_dtw_std", variant)
    maps = B.model_maps("rna_dtw_std", variant)
    assert {band.col_st for band in case.bands} == {0, 1, 2, 300}
    differs = {B.SPIKE: 0, B.HUGE: 0}
    for contig, strand, col, level in case.spikes:
        k = next(i for i, band in enumerate(case.bands) if band.contig == contig)
        band = case.bands[k]
        assert band.col_st == col + 1 and maps[k] is not None
        x = M.dp_query(b.q[b.q_off[band.read]:b.q_off[band.read + 1]], True, False)
        y = b.forward[contig].copy()
        y[col] = x[0]
        other = M.band_map(x, y, band.col_st, band.col_st + band.m - 1, True)
        d = other is None or not np.array_equal(other, maps[k])
        assert d or level != B.HUGE, (variant, band)
        differs[level] += d
    assert differs[B.SPIKE] >= 2 and differs[B.HUGE] == 9, differs


def sequential_row0(x0, y, upto):
    """row 0 of --dtw-std up to column `upto` of the array as the kernel's loop adds it up: |x0 - y[0]|, then one float32 addition
    per column, in order.  Plain Python over numpy scalars: no cumsum, no reduction whose order numpy chooses"""
    acc = np.float32(abs(np.float32(x0) - y[0]))
    out = [acc]
    for j in range(1, upto + 1):
        acc = np.float32(np.float32(abs(np.float32(x0) - y[j])) + acc)
        out.append(acc)
    return out


@pytest.mark.parametrize("variant", B.VARIANTS)
@pytest.mark.parametrize("name", ["rna_dtw_std", "strips_rna_dtw_std"])
def test_dtw_std_row_0_is_the_sequential_sum(name, variant):
    """every --dtw-std band of the table: the model's row 0, all m columns of it, is the sequential float32 sum from column 0 of the
    array -- the columns in front of the band included --, and |x0 - y0| itself where the band begins at column 0"""
    case, b = B.CASES[name], B.build(name, variant)
    assert case.flag & B.DTW
    col_sts, order_shows = set(), 0
    for band in case.bands:
        x = M.dp_query(b.q[b.q_off[band.read]:b.q_off[band.read + 1]], True, False)
        y = b.forward[band.contig]
        en = band.col_st + band.m - 1
        S_ = M.band_costs(x, y, band.col_st, en, True)
        want = sequential_row0(x[0], y, en)
        got = [S_[j, 0] for j in range(band.m)]
        assert all(type(g) is np.float32 for g in got) and got == want[band.col_st:], (name, variant, band)
        if band.col_st == 0:
            assert got[0] == np.float32(abs(x[0] - y[0]))
        col_sts.add(band.col_st)
        # (about the inputs) a sum whose value shows the order it was added up in: it is not the float64 sum rounded once
        exact = np.abs(np.float64(x[0]) - y[:en + 1].astype(np.float64)).cumsum()
        order_shows += any(np.float32(e) != w for e, w in zip(exact[band.col_st:], want[band.col_st:]))
    assert col_sts >= ({0, 1, 2, 300} if name == "rna_dtw_std" else {2})
    if variant == "normal":
        assert order_shows >= len(case.bands) // 2, order_shows
