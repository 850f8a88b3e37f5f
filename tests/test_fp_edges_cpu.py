"""The cases of tests/fp_edges.py are what they claim, from the oracle alone (no GPU): every score of denormal_all is a non-zero
denormal (so the oracle build itself does not flush), denormal_crossing has scores on both sides of 2^-126, an exact power of two
scales the scores and nothing else, 2^-120 does not, absorbed has ties and winners a float64 accumulator would not give, signed_zero
has scores of +0 with both divisions by zero in its mapq, near_top reaches the last binades of fp32 -- and a 5 x 12 matrix of
denormals is recomputed by a float32 DP written out below, bit for bit."""
import numpy as np
import pytest

from tests import fp_edges as F

STRIP_ROWS = 2048  # a query beyond this many events is filled in row strips of at most this many rows ("row strips")

_rows = {}


def rows_of(O, name):
    if name not in _rows:
        case = F.build(name)
        _rows[name] = O.align_batch(case.q, case.q_off, F.oracle_ref(O, case), case.flag, threads=8)
        _rows[name].setflags(write=False)
    return _rows[name]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def names_of(family):
    return [n for n in F.NAMES if F.family_of(n) == family]


def test_the_case_list():
    assert [f for f in F.FAMILIES if not names_of(f)] == []
    assert {F.build(n).mode for n in F.NAMES} == {"dna", "rna", "rna_inv", "rna_std"}
    assert {f for f in F.FAMILIES} == {F.family_of(n) for n in F.NAMES if F.build(n).mode == "dna"}  # every family on both strands
    for n in F.NAMES:
        c = F.build(n)
        qlens = list(np.diff(c.q_off))
        assert c.family == F.family_of(n)
        assert set(qlens) == {1, 64, 250, 257, 600, 1100, 2100} and 8 <= len(qlens) <= 16, n
        assert c.lens == [701, 1503] and min(c.lens) < 1100 and max(c.lens) < 2100, n
        assert (c.reverse is not None) == (c.mode == "dna") and (c.mode == "dna" or min(c.offs) > 0), n
        assert F.bound(c) < F.FLT_MAX / 2, n  # every cell finite by construction
        if c.mode == "dna":
            assert {s for _, s, _ in c.origin} == {"+", "-"} and {s for (_, s, _), q in zip(c.origin, qlens) if q > STRIP_ROWS} == {"+", "-"}, n


def test_windows_and_strips():
    """every strand has two or more last-row windows for the reads of up to 600 events (a window is as long as the query,
    src/sigfish.c:891-901; the longer reads have one or two, and a single partial one on the short contig), and the reads of 2100
    events take two row strips"""
    for n in F.NAMES:
        c = F.build(n)
        for q in np.diff(c.q_off):
            for rlen in c.lens:
                assert F.windows(rlen, int(q)) >= 2 or q > 600, (n, q, rlen)
        assert F.windows(c.lens[1], 1100) == 2 and F.windows(c.lens[0], 1100) == 1
        assert sorted({-(-int(q) // STRIP_ROWS) for q in np.diff(c.q_off)}) == [1, 2]


@pytest.mark.parametrize("name", names_of("denormal_all"))
def test_denormal_all_scores_are_non_zero_denormals(oracle, name):
    r = rows_of(oracle, name)
    assert (r["valid"] == 1).all()
    for f in ("score", "score2"):
        assert (r[f] > 0).all() and (r[f] < np.float32(F.MIN_NORMAL)).all(), (f, r[f])
        assert ((bits(r[f]) >> 23) == 0).all()  # exponent field 0
    # the arithmetic is exact: a score is its integer number of units of 2^-149, and the planted noise alone costs that many
    assert (bits(r["score"]) >= 1).all() and (bits(r["score"]) < 2100 * 25).all()


@pytest.mark.parametrize("name", names_of("denormal_crossing"))
def test_denormal_crossing_has_scores_on_both_sides(oracle, name):
    case, r = F.build(name), rows_of(oracle, name)
    assert (r["valid"] == 1).all() and (r["score"] > 0).all()
    tiny = np.float32(F.MIN_NORMAL)
    c, s, y = F.jobs(case)[0]
    if case.flag & F.DTW:
        # --dtw-std: one candidate per contig, the sum of a path through all of it -- every score is normal; the crossing lies
        # inside each matrix, where row 0 is a running sum that begins as a denormal
        assert (r["score"] >= tiny).all()
        row0 = oracle.std_dtw(F.dp_query(case, 1), y)[0]
        assert 0 < row0[0] < tiny <= row0[-1] and (np.diff(row0) >= 0).all()
        return
    assert (r["score"] < tiny).any() and (r["score"] >= tiny).any(), r["score"]
    # ... and inside one matrix: the last row of the read of one event is what query row 0 of a longer read looks like
    i = list(np.diff(case.q_off)).index(1)
    row0 = oracle.last_row(F.events_of(case, i), y, case.flag)[0]
    assert (row0 < tiny).mean() > 0.5 and (row0 > 0).any()
    long_row = oracle.last_row(F.events_of(case, 1), y, case.flag)[0]
    assert (long_row >= tiny).all()


@pytest.mark.parametrize("k,mode", [(60, "dna"), (-60, "dna"), (100, "dna"), (100, "rna_std")])
def test_an_exact_power_of_two_scales_the_scores_and_nothing_else(oracle, k, mode):
    name = f"pow2_scaled_{'m' if k < 0 else 'p'}{abs(k)}_{mode}"
    base, got = rows_of(oracle, f"ordinary_{mode}"), rows_of(oracle, name)
    assert (base["valid"] == 1).all()
    for f in ("valid", "rid", "strand", "pos_st", "pos_end", "mapq"):
        assert np.array_equal(got[f], base[f]), (name, f)
    for f in ("score", "score2"):
        want = (base[f].astype(np.float64) * 2.0 ** k).astype(np.float32)
        assert np.isfinite(want).all() and (want >= np.float32(F.MIN_NORMAL)).all()
        assert np.array_equal(bits(got[f]), bits(want)), (name, f)


@pytest.mark.parametrize("mode", ["dna", "rna"])
def test_two_to_the_minus_120_does_not(oracle, mode):
    """inputs and costs below 2^-126 have fewer bits than the base has: the scores are not 2^-120 times the scores of the base (those
    that stay above 2^-126 may be: a difference of two floats is exact even where it is a denormal), which is why this family
    cannot be replaced by the property above"""
    base, got = rows_of(oracle, f"ordinary_{mode}"), rows_of(oracle, f"pow2_scaled_m120_{mode}")
    assert (got["valid"] == 1).all() and (got["score"] > 0).all()
    differ = got["score"].astype(np.float64) * 2.0 ** 120 != base["score"].astype(np.float64)  # (exact in float64 either way)
    print(mode, "reads whose score is not 2^-120 x the score of the base:", np.flatnonzero(differ), "of", len(got))
    assert differ.any() and (got["score"][differ] < np.float32(F.MIN_NORMAL)).all()
    assert np.allclose(got["score"].astype(np.float64) * 2.0 ** 120, base["score"], rtol=1e-3)  # (still the same alignment problem)


def _winner_in(case, i, dtype):
    """(contig, strand, last-row column) of the reference's winner had every sum been made in `dtype`: windows of qlen columns,
    the first strict minimum of each, a later candidate wins an exact tie (oracle/sdtw_oracle.c: scan_windows, top_offer)"""
    x = F.dp_query(case, i)
    best = None
    for c, s, y in F.jobs(case):
        last = F.last_row_of(x, y, dtype)
        for w in range(0, len(y), len(x)):
            col = w + int(np.argmin(last[w:w + len(x)]))
            if best is None or not (last[col] > best[0]):
                best = (last[col], c, s, col)
    return best[1:]


def _winner_of_row(case, r):
    c, s = int(r["rid"]), chr(r["strand"])
    off = case.offs[c]
    return (c, s, int(r["pos_end"]) - off if s == "+" else case.lens[c] - (int(r["pos_st"]) - off))


@pytest.mark.parametrize("name", names_of("absorbed"))
def test_absorbed_has_ties_and_winners_a_wider_sum_would_not_give(oracle, name):
    case, r = F.build(name), rows_of(oracle, name)
    assert (r["valid"] == 1).all() and (r["score"] > 2.0 ** 19).all()
    tie = bits(r["score"]) == bits(r["score2"])
    long_enough = np.diff(case.q_off) > F.ABSORB_ROWS
    assert (r["score"][long_enough] >= 2.0 ** 23).all() and (r["score"][long_enough] == np.round(r["score"][long_enough])).all()  # fp32 counts in ones here
    assert tie.any(), r["score"]
    changed = []
    for i in np.flatnonzero(np.diff(case.q_off) <= 600):
        assert _winner_in(case, i, np.float32) == _winner_of_row(case, r[i]), (name, i)  # (the restatement above is the oracle's rule)
        if _winner_in(case, i, np.float64) != _winner_of_row(case, r[i]):
            changed.append(int(i))
    print(name, "ties", np.flatnonzero(tie), "winner differs under float64 for reads", changed)
    assert changed


@pytest.mark.parametrize("name", names_of("signed_zero"))
def test_signed_zero_scores_are_plus_zero_and_mapq_divides_by_zero(oracle, name):
    case, r = F.build(name), rows_of(oracle, name)
    assert (r["valid"] == 1).all()
    zero = r["score"] == 0
    assert (bits(r["score"][zero]) == 0).all() and (bits(r["score2"][r["score2"] == 0]) == 0).all()  # +0, never -0
    both = zero & (r["score2"] == 0)   # 0 / 0
    one = zero & (r["score2"] > 0)     # x / 0
    rest = ~zero
    assert both.sum() >= 3 and one.any() and rest.sum() == 2, (r["score"], r["score2"])
    assert (r["mapq"][both] == 0).all() and [oracle.mapq(0.0, float(x)) for x in r["score2"][one]] == list(r["mapq"][one])
    assert (r["score"][rest] == np.round(r["score"][rest])).all()


@pytest.mark.parametrize("name", names_of("near_top"))
def test_near_top_reaches_the_last_binades(oracle, name):
    case, r = F.build(name), rows_of(oracle, name)
    assert F.FLT_MAX / 8 < F.bound(case) < F.FLT_MAX / 2
    assert (r["valid"] == 1).all() and np.isfinite(r["score"]).all() and np.isfinite(r["score2"]).all()
    i = int(np.argmax(np.diff(case.q_off)))
    worst = max(float(cost.max()) for _, _, cost, _ in oracle.last_rows(F.events_of(case, i), F.oracle_ref(oracle, case), case.flag))
    print(name, "largest score", r["score2"].max(), "largest last-row cell", worst, "bound", F.bound(case))
    assert np.isfinite(worst) and worst > F.FLT_MAX / 64   # a last-row cell within six binades of the top
    assert r["score2"].max() > 2.0 ** 120


def test_a_matrix_of_denormals_recomputed_here(oracle):
    """q = 5 against 12 columns, small integers x 2^-149: the recurrence written out in np.float32 (src/cdtw.c:170-190) gives the
    oracle's matrix and row bit for bit, so the oracle neither flushes denormals nor sums in a wider type"""
    rng = np.random.default_rng(5)
    unit = np.float64(2.0 ** -149)
    x = (rng.integers(-9, 10, 5) * unit).astype(np.float32)
    y = (rng.integers(-9, 10, 12) * unit).astype(np.float32)
    C = np.zeros((5, 12), np.float32)
    for j in range(12):
        C[0, j] = np.abs(x[0] - y[j])
    for i in range(1, 5):
        C[i, 0] = np.abs(x[i] - y[0]) + C[i - 1, 0]
        for j in range(1, 12):
            C[i, j] = np.abs(x[i] - y[j]) + min(C[i - 1, j], C[i - 1, j - 1], C[i, j - 1])
    assert C.dtype == np.float32 and (C[-1] > 0).all() and (C < np.float32(F.MIN_NORMAL)).all()
    assert np.array_equal(bits(C), np.rint(C.astype(np.float64) / unit).astype(np.uint32))  # whole numbers of units: nothing was rounded
    assert np.array_equal(bits(oracle.subsequence(x, y)), bits(C))
    ref = oracle.RefSynth(["c0"], [17], [12], [0], [y], [y[::-1].copy()])
    row = oracle.align_batch(x, np.array([0, 5], np.int64), ref, 0)[0]
    last_rv = oracle.last_row(x, y[::-1].copy(), 0)[0]
    cands = [C[-1, :5].min(), C[-1, 5:10].min(), C[-1, 10:].min(), last_rv[:5].min(), last_rv[5:10].min(), last_rv[10:].min()]
    assert bits(row["score"]) == bits(min(cands)) and row["valid"] == 1
    assert np.array_equal(bits(F.last_row_of(x, y, np.float32)), bits(C[-1]))  # (the anti-diagonal DP of fp_edges.py, in float32)
