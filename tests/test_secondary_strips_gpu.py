"""Secondary mappings of reads beyond 2048 events (option "secondary_strips": the row strips keep every (read, job)'s list of its 5
best windows, a merge ranks them, pass 2 traces ranks 1..4) against the restatement of the reference's candidate list
(tests/secondary_oracle.py).  Rows are compared exactly: valid flags, integer fields, scores bit for bit.  Every test that switches
the option on also compares the primaries byte for byte with a run without it.

Candidates per read.  A DNA read of q events over contigs of r columns has 2 * sum(ceil(r / q)) candidates.  For the contigs
[6200, 2300, 900] of test_shapes that is 14 at q = 2049 and 8 at q = 4097: every long read there has all four secondaries, for
every seed (checked with the oracle alone for the two seeds used, generator seeds 4201 and 4202: 8 of 8 long reads have four valid
rows, none fewer).  Fewer than four occur on the reference [900] (two candidates, one secondary) of the case `few_windows`, again
for both seeds; test_shapes asserts the first property on the contigs above and the second on that case.  With the quarter-quantised
values of seed 4201 two of the long reads have equal scores among their five candidates (the oracle alone; 4200 has none): the
order of equals is update_aln's, the later candidate first."""
import numpy as np
import pytest

import sigfish_amd as S
from tests.secondary_oracle import secondary_rows
from tests.util import device_lists

pytestmark = pytest.mark.gpu


def _arr(rng, n, quant):
    return (rng.integers(-6, 7, n) / 4).astype(np.float32) if quant else rng.normal(size=n).astype(np.float32)


def _small_ref(rng, lens, rna, quant=True):
    fw = [_arr(rng, n, quant) for n in lens]
    rv = None if rna else [_arr(rng, n, quant) for n in lens]
    return S.RefModel([f"c{i}" for i in range(len(lens))], [n + 5 for n in lens], lens,
                      rng.integers(0, 3, len(lens)) if rna else [0] * len(lens), fw, rv)


def _oref(O, ref):
    return O.RefSynth(ref.names, ref.seq_lengths, ref.ref_lengths, ref.st_offset, ref.forward, ref.reverse)


def _batch(rng, qlens, quant=True):
    q_off = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int64)
    return _arr(rng, int(q_off[-1]), quant), q_off


def assert_sec_equal(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got["valid"], want["valid"]), np.argwhere(got["valid"] != want["valid"])[:8]
    v = want["valid"] == 1
    for f in ("rid", "strand", "pos_st", "pos_end", "mapq"):
        assert np.array_equal(got[f][v], want[f][v]), (f, np.argwhere((got[f] != want[f]) & v)[:8])
    assert np.array_equal(got["score"][v].view(np.uint32), want["score"][v].view(np.uint32))
    assert np.array_equal(got["score2"][v].view(np.uint32), want["score2"][v].view(np.uint32))


def _run(al, q, q_off, n_sec=4):
    """(primaries without secondaries, primaries with, secondaries) of one batch, the option on"""
    al.set_secondary(0)
    base = al.align_db(q, q_off)
    al.set_secondary(n_sec)
    al.set_option("secondary_strips", 1)
    prim = al.align_db(q, q_off)
    return base, prim, al.secondary_rows()


LONG = [2049, 2560, 2561, 3072, 3073, 3585, 4096, 4097]  # 2 strips at R = 20, 20 | 24, 24 | 28, 32; 2 | 3 strips
SHORT = [250, 64, 2048]
_expected = {}  # the oracle's rows of a (case, seed), computed once


def _shapes_case(oracle, case, seed):
    lens = {"contigs": [6200, 2300, 900], "few_windows": [900]}[case]
    rng = np.random.default_rng(4201 + seed)
    quant = seed == 0  # quarter-quantised values: equal scores occur, the tie order decides
    ref = _small_ref(rng, lens, False, quant)
    qlens = np.array(LONG + SHORT if case == "contigs" else [2049, 250, 4097])
    rng.shuffle(qlens)
    q, q_off = _batch(rng, qlens, quant)
    key = (case, seed)
    if key not in _expected:
        _expected[key] = secondary_rows(oracle, q, q_off, _oref(oracle, ref), 0)
    return ref, qlens, q, q_off, _expected[key]


@pytest.mark.parametrize("seed", [0, 1], ids=["quantised", "normal"])
@pytest.mark.parametrize("case", ["contigs", "few_windows"])
def test_shapes(oracle, case, seed):
    ref, qlens, q, q_off, want = _shapes_case(oracle, case, seed)
    with S.Aligner(ref, 0) as al:
        base, prim, sec = _run(al, q, q_off)
    assert prim.tobytes() == base.tobytes()
    assert_sec_equal(sec, want)
    n_valid = sec["valid"][qlens > 2048].sum(axis=1)
    if case == "contigs":
        assert (n_valid == 4).any()
        if seed == 0:  # (about this test's own input) equal scores inside a list do occur
            lists = np.concatenate([prim["score"][:, None], sec["score"]], axis=1)[qlens > 2048]
            assert any(len(set(r)) < 5 for r in lists)
    else:
        assert (n_valid < 4).all() and (n_valid > 0).all()


RNA_CASES = {
    "rna": (S.RNA, [2500, 1400, 300, 900, 2200]),
    "rna_inv": (S.RNA | S.INV, [2500, 1400, 300, 900, 2200]),
    "rna_std": (S.RNA | S.DTW, [2500, 1400, 300, 900, 2200, 600]),
}


@pytest.mark.parametrize("case", list(RNA_CASES))
def test_rna(oracle, case):
    flag, lens = RNA_CASES[case]
    rng = np.random.default_rng(77 + len(case))
    ref = _small_ref(rng, lens, True)
    q, q_off = _batch(rng, [2100, 250, 4100])
    with S.Aligner(ref, flag) as al:
        base, prim, sec = _run(al, q, q_off)
    assert prim.tobytes() == base.tobytes()
    want = secondary_rows(oracle, q, q_off, _oref(oracle, ref), flag)
    assert_sec_equal(sec, want)
    assert sec["valid"][[0, 2]].all()  # five contigs or more: every rank has a candidate


def test_option_semantics(oracle):
    rng = np.random.default_rng(31)
    ref = _small_ref(rng, [5000, 900], False)
    q, q_off = _batch(rng, [250, 2100, 64, 3000])
    long = [1, 3]
    with S.Aligner(ref, 0) as al:
        for bad in (-1, 2, 5):
            with pytest.raises(S.SfaError):
                al.set_option("secondary_strips", bad)
        base, prim, sec2 = _run(al, q, q_off, n_sec=2)
        assert prim.tobytes() == base.tobytes()
        assert_sec_equal(sec2, secondary_rows(oracle, q, q_off, _oref(oracle, ref), 0, n_sec=2))
        assert sec2["valid"][long][:, :2].all() and not sec2["valid"][:, 2:].any()
        al.set_secondary(4)
        prim4 = al.align_db(q, q_off)
        sec4 = al.secondary_rows()
        want = secondary_rows(oracle, q, q_off, _oref(oracle, ref), 0)
        assert_sec_equal(sec4, want)
        v = sec4["valid"][:, 0] == 1
        assert v[long].all()
        assert np.array_equal(sec4["score"][v, 0].view(np.uint32), prim4["score2"][v].view(np.uint32))  # rank 1 is the primary's runner-up
        al.set_option("secondary_strips", 0)  # ... and back: the long reads have none again, in the same context
        prim0 = al.align_db(q, q_off)
        sec0 = al.secondary_rows()
    assert prim4.tobytes() == base.tobytes() and prim0.tobytes() == base.tobytes()
    assert not sec0["valid"][long].any()
    want[long] = sec0[long]
    assert_sec_equal(sec0, want)


def test_groups_on_two_scratch_sets(oracle):
    """A checkpoint budget that holds two reads per set of scratch: six long reads run as three groups alternating between the two
    sets and streams, each group's ranks traced before the next group of its set overwrites the boundary rows and checkpoints."""
    rng = np.random.default_rng(41)
    ref = _small_ref(rng, [2600, 700], False)
    qlens = [2049, 3000, 250, 4097, 2500, 3585, 2100]
    q, q_off = _batch(rng, qlens)
    # one read's scratch (sfa_plan.hpp, plan_long_groups) at the longest query's 3 strips, T = 512: 2 boundary rows of both strands'
    # padded columns, and 3 strips x ((rlen - 1) >> 9) checkpoint records of 33 x 64 floats per strand
    pad = lambda n: (n + 256 + 3) & ~3
    per_read = 4 * 2 * 2 * (pad(2600) + pad(700)) + 4 * 33 * 64 * 3 * 2 * ((2599 >> 9) + (699 >> 9))
    with S.Aligner(ref, 0) as al:
        base, prim, sec = _run(al, q, q_off)
        al.set_option("ckpt_interval", 512)
        al.set_option("ckpt_budget_bytes", 4 * per_read)  # two sets of two reads
        prim_small = al.align_db(q, q_off)
        sec_small = al.secondary_rows()
    assert prim.tobytes() == base.tobytes() and prim_small.tobytes() == base.tobytes()
    assert_sec_equal(sec, secondary_rows(oracle, q, q_off, _oref(oracle, ref), 0))
    assert sec_small.tobytes() == sec.tobytes()


def test_non_finite_long_read(oracle):
    rng = np.random.default_rng(51)
    ref = _small_ref(rng, [2600, 700], False)
    q, q_off = _batch(rng, [2100, 3000, 250, 2500])
    with S.Aligner(ref, 0) as al:
        _, _, clean = _run(al, q, q_off)
        q2 = q.copy()
        q2[q_off[1] + 1234] = np.nan
        base, prim, sec = _run(al, q2, q_off)
    assert prim.tobytes() == base.tobytes() and not prim["valid"][1]
    assert not sec["valid"][1].any()
    keep = [0, 2, 3]
    assert sec[keep].tobytes() == clean[keep].tobytes()
    # (about this test's own input: 2 x (2 + 1) windows for the reads of 2100 and 2500 events, 2 x (1 + 1) for the one of 3000)
    assert clean["valid"][[0, 3]].all() and list(clean["valid"][1]) == [1, 1, 1, 0]
    assert_sec_equal(clean, secondary_rows(oracle, q, q_off, _oref(oracle, ref), 0))


def test_entry_points(oracle):
    rng = np.random.default_rng(61)
    ref = _small_ref(rng, [2600, 700], False)
    qlens = np.array([250, 2100, 64, 3000])
    q, q_off = _batch(rng, qlens)
    want = secondary_rows(oracle, q, q_off, _oref(oracle, ref), 0)
    assert want["valid"][1].all() and list(want["valid"][3]) == [1, 1, 1, 0]  # (this test's own input: 6 and 4 windows)
    with S.Aligner(ref, 0) as al:
        base = al.align_db(q, q_off)
        al.set_secondary(4)
        al.set_option("secondary_strips", 1)
        al.submit(q, q_off)
        assert al.wait().tobytes() == base.tobytes()
        assert_sec_equal(al.secondary_rows(), want)
        tables = []
        for i in range(len(qlens)):
            ev = np.zeros(int(qlens[i]) + 3, S.EVENT_DTYPE)
            ev["mean"][3:] = q[q_off[i]:q_off[i + 1]]
            tables.append(ev)
        rows = al.align_events(tables, [3] * len(qlens), [3 + int(x) for x in qlens])
        assert rows.tobytes() == base.tobytes()
        assert_sec_equal(al.secondary_rows(), want)


@pytest.mark.parametrize("devs", device_lists())
def test_two_shards(oracle, devs):
    if len(devs) < 2:
        pytest.skip("one device list entry")
    rng = np.random.default_rng(71)
    ref = _small_ref(rng, [2600, 700], False)
    qlens = [2100, 250, 3000, 64, 2049, 600, 2500]
    q, q_off = _batch(rng, qlens)
    with S.Aligner(ref, 0) as al:
        base = al.align_db(q, q_off)
    with S.Aligner(ref, 0, devices=devs) as al:
        al.set_secondary(4)
        al.set_option("secondary_strips", 1)
        prim = al.align_db(q, q_off)
        sec = al.secondary_rows()
    assert prim.tobytes() == base.tobytes()
    assert_sec_equal(sec, secondary_rows(oracle, q, q_off, _oref(oracle, ref), 0))


def _host_map(ref, flag, q, q_off, read, row):
    x = q[q_off[read]:q_off[read + 1]]
    ev = np.zeros(len(x), S.EVENT_DTYPE)
    ev["mean"] = x
    j = int(row["rid"])
    y = ref.forward[j] if row["strand"] == ord("+") else ref.reverse[j]
    try:
        return S.r2qevent_map(row, ev, 0, len(x), y, int(ref.st_offset[j]), flag)
    except S.SfaError:
        return None


@pytest.mark.parametrize("flag", [0, S.RNA], ids=["dna", "rna"])
def test_event_maps_of_long_secondaries(flag):
    """sfa_event_maps over the rows of secondary_rows(), long reads included: in row strips on the device ("map_strips" 1) and from
    the host routine inside the call (0), both the bytes of sfa_r2qevent_map per row."""
    rng = np.random.default_rng(81 + flag)
    ref = _small_ref(rng, [2600, 700, 1500, 400, 2200], bool(flag & S.RNA))
    qlens = [2100, 250, 3000]
    q, q_off = _batch(rng, qlens)
    with S.Aligner(ref, flag) as al:
        al.set_secondary(4)
        al.set_option("secondary_strips", 1)
        al.align_db(q, q_off)
        sec = al.secondary_rows()
        assert sec["valid"][[0, 2]].all()
        rows, ror = sec.reshape(-1), np.repeat(np.arange(len(qlens), dtype=np.int32), 4)
        n_long_rows = int(sec["valid"][[0, 2]].sum())
        got = {}
        for on in (1, 0):
            al.set_option("map_strips", on)
            got[on] = al.event_maps(rows, ror)
            assert al.maps_on_host == (0 if on else n_long_rows)
    n_maps = 0
    for k, row in enumerate(rows):
        want = _host_map(ref, flag, q, q_off, int(ror[k]), row) if row["valid"] else None
        for on in (1, 0):
            if want is None:
                assert len(got[on][k]) == 0, (on, k)
            else:
                assert got[on][k].dtype == np.int32 and got[on][k].tobytes() == want.tobytes(), (on, k)
        n_maps += want is not None
    assert n_maps >= 8
