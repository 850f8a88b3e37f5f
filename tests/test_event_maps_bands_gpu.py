"""The band fill and walk kernels behind sfa_event_maps and sfa_session_event_maps (sdtw_path.hpp) at bands the test chooses:
the rows of tests/map_bands.py -- widths of 1 to 2100 columns at every class's edges, widths of 1 and 1700 side by side in a
wave, waves with idle slots, bands at both ends of their arrays, --dtw-std bands behind a prefix that decides their ties, one read
named by 40 rows, rows without a complete map between rows that have one, row strips -- put on queries that an align call left
resident (its own rows are ignored).  Every map must equal the map of the numpy model tests/maps_model.py, which
tests/test_maps_model_cpu.py holds against the host routine: integers from the same float32 operations, so equality is exact.
maps_on_host == 0 wherever the device is to take every row: the in-call host routine cannot stand in for a kernel."""
import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import synth
from tests import map_bands as B
from tests import maps_model as M
from tests import test_session_maps_gpu as T

pytestmark = pytest.mark.gpu

NONE = np.iinfo(np.int32).min  # what Session.event_maps leaves where the library wrote nothing


def assert_maps(got, want, what):
    assert len(got) == len(want), what
    for k, w in enumerate(want):
        if w is None:
            assert len(got[k]) == 0, (what, k, got[k][:4])
        else:
            assert got[k].dtype == np.int32 and got[k].shape == w.shape and np.array_equal(got[k], w), (what, k, got[k][:6], w[:6])


def run(name, variant, options=()):
    """the case's rows through Aligner.event_maps, twice -> (maps, maps_on_host, maps of the second call)"""
    case, b = B.CASES[name], B.build(name, variant)
    with S.Aligner(B.ref_model(b), case.flag) as al:
        for key, value in options:
            al.set_option(key, value)
        al.align_db(b.q, b.q_off)  # the queries are resident now; what it aligned them to does not matter
        maps = al.event_maps(b.rows, b.read_of_row)
        on_host = al.maps_on_host
        again = al.event_maps(b.rows, b.read_of_row)
        assert al.maps_on_host == on_host
    return maps, on_host, again


@pytest.mark.parametrize("variant", B.VARIANTS)
@pytest.mark.parametrize("name", B.TABLE)
def test_bands(name, variant):
    maps, on_host, again = run(name, variant)
    assert on_host == 0
    assert_maps(maps, B.model_maps(name, variant), (name, variant))
    assert_maps(again, B.model_maps(name, variant), (name, variant, "second call"))


@pytest.mark.parametrize("variant", B.VARIANTS)
@pytest.mark.parametrize("name", B.STRIPS)
def test_strips(name, variant):
    maps, on_host, again = run(name, variant, (("map_strips", 1),))
    assert on_host == 0
    assert_maps(maps, B.model_maps(name, variant), (name, variant))
    assert_maps(again, B.model_maps(name, variant), (name, variant, "second call"))


@pytest.mark.parametrize("variant", B.VARIANTS)
def test_two_budgets(variant):
    """a budget between the moves of the widest row and of the second widest: exactly the rows above it go to the host routine, the
    others through in several slices, and every map is the one the default budget gave"""
    name = "mixed_block_plus_one"
    case = B.CASES[name]
    sizes = [B.row_bytes(case.qlens[band.read], band.m) for band in case.bands]
    top = sorted(sizes)
    budget = (top[-2] + top[-1]) // 2
    above = sum(s > budget for s in sizes)
    assert above == 1 and sum(sizes) - top[-1] > 2 * budget  # (about the case: one row above, the rest in three slices or more)
    full, on_host, _ = run(name, variant)
    assert on_host == 0
    small, on_host, again = run(name, variant, (("map_scratch_bytes", budget),))
    assert on_host == above
    assert_maps(small, B.model_maps(name, variant), (name, variant, budget))
    assert all(np.array_equal(a, b) for a, b in zip(full, small)) and all(np.array_equal(a, b) for a, b in zip(small, again))


def session_maps(pairs, off):
    out = []
    for k in range(len(off) - 1):
        m = pairs[off[k]:off[k + 1]]
        out.append(np.zeros((0, 2), np.int32) if len(m) and (m == NONE).all() else m)
    return out


@pytest.mark.parametrize("variant", B.VARIANTS)
def test_event_mode_session(variant):
    """slots of 60, 300, 700 and 1500 kept events -- four classes --, extended once; the crafted rows of the mixed-widths case name
    every slot many times, and those of the no-map case leave rows unwritten between written ones"""
    for name in ("mixed_block_plus_one", "no_map_between_maps"):
        case, b = B.CASES[name], B.build(name, variant)
        n = len(case.qlens)
        with S.Aligner(B.ref_model(b), case.flag) as al, al.session(n, keep_events=max(case.qlens)) as se:
            se.extend(list(range(n)), b.q, b.q_off)
            pairs, off, on_host = se.event_maps(b.rows, b.read_of_row)
            again, off2, _ = se.event_maps(b.rows, b.read_of_row)
        assert on_host == 0 and np.array_equal(off, S.map_offsets(b.rows)) and np.array_equal(off, off2)
        assert_maps(session_maps(pairs, off), B.model_maps(name, variant), (name, variant))
        assert again.tobytes() == pairs.tobytes()
        assert np.bincount(b.read_of_row).min() >= 2


def test_raw_mode_slot():
    """one raw-mode slot: its query is what the device normalised from its own events.  Around the row the session reports, bands of
    1 .. 17 columns that end where it ends, halves of it, the band itself and wider ones that begin in front of it"""
    k = 6
    levels = synth.kmer_levels(k, 21)
    recs = [("c0", synth.random_sequence(1405, 1)), ("c1", synth.random_sequence(305, 3))]
    ref = S.RefModel.from_records(recs, levels, k, 0, 250)
    sig = synth.make_dna_raw_reads(recs[:1], levels, k, 1, seed=8, samples=(9000, 9000), meta=T.META)[0][5]
    skip, norm, query = 3, 25, 600
    with S.Aligner(ref, 0) as al, al.session(1) as se:
        se.configure_raw(skip, norm, query)
        rows, info = se.extend_raw([0], sig, [0, len(sig)], [T.SCALE], [True])
        assert rows["valid"][0] and rows["rid"][0] >= 0
        q = int(info["q_events"][0])
        x = T.normalised(se.events(0), skip, q, info["norm_mean"][0], info["norm_sd"][0])["mean"][skip:skip + q].copy()
        j, plus = int(rows["rid"][0]), rows["strand"][0] == ord("+")
        y = ref.forward[j] if plus else ref.reverse[j]
        st, en = M.row_columns(int(rows["pos_st"][0]), int(rows["pos_end"][0]), plus, len(y), int(ref.st_offset[j]))
        bands = [(en - m + 1, en) for m in (1, 2, 3, 4, 5, 7, 8, 15, 16, 17, (en - st) // 2, 3 * (en - st) // 4) if en - m + 1 >= 0]
        bands += [(st, en), (st, en), (max(st - 9, 0), en), (st + 5, en), (st, min(en + 40, len(y) - 1)), (0, min(q // 2, len(y) - 1))]
        crafted = np.repeat(rows, len(bands))
        for i, (a, z) in enumerate(bands):
            crafted["pos_st"][i], crafted["pos_end"][i] = M.row_positions(a, z, plus, len(y), int(ref.st_offset[j]))
        pairs, off, on_host = se.event_maps(crafted, [0] * len(bands))
        again, _, _ = se.event_maps(crafted, [0] * len(bands))
    assert on_host == 0 and again.tobytes() == pairs.tobytes()
    want = [M.band_map(x, y, a, z, False) for a, z in bands]
    assert want[12] is not None and sum(w is not None for w in want) >= 8 and q > 256  # (about the inputs)
    assert_maps(session_maps(pairs, off), want, ("raw slot", q, st, en))
