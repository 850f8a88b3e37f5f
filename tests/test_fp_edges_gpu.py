"""The fp32 edge cases of tests/fp_edges.py through every alignment route: align_db under every entry of MODES and with pinned column
segments, the strip reads alone under strips_backoff, secondaries, event maps, sessions fed in chunks (rows after every chunk, the
carried row read back) and the class route over a target.  Everything is compared bit for bit -- scores and carried costs as uint32
views, the rest as integers -- with oracle.align_batch, tests/secondary_oracle.py, tests/maps_model.py, oracle.last_rows and
tests/targets_oracle.py; there is no tolerance anywhere.  tests/test_fp_edges_cpu.py shows without a GPU that each case reaches the
range it is named after (denormal costs, the crossing to normal, the last binades, absorbed terms, signed zeros)."""
import numpy as np
import pytest

import sigfish_amd as S
from tests import fp_edges as F
from tests import maps_model as M
from tests import targets_oracle as T
from tests.secondary_oracle import secondary_rows
from tests.test_gpu_parity import MODES, assert_rows_equal
from tests.test_secondary_gpu import assert_sec_equal
from tests.test_session_gpu import Oracle, assert_rows

pytestmark = pytest.mark.gpu

ROUTES = dict(MODES, segments_warm1={"column_segments": 6, "segment_warm_windows": 1})
STRIP_READS = [i for i, n in enumerate(F.QLENS) if n > 2048]
SESSION_READS = [i for i, n in enumerate(F.QLENS) if n in (250, 600)]
CHUNKS = (33, 1, 64)  # ... and the rest
SECONDARY = [n for n in F.NAMES if F.family_of(n) in ("denormal_all", "absorbed", "signed_zero")]
MAPS = [n for n in F.NAMES if F.family_of(n) in ("denormal_all", "absorbed")]
SESSIONS = [n for n in F.NAMES if F.family_of(n) in ("denormal_all", "denormal_crossing", "near_top") and F.build(n).mode in ("dna", "rna_inv")]

_want, _want_sec = {}, {}


def expected(O, case):
    """the oracle's rows of the case's reads, computed once and shared"""
    if case.name not in _want:
        _want[case.name] = O.align_batch(case.q, case.q_off, F.oracle_ref(O, case), case.flag, threads=8)
        _want[case.name].setflags(write=False)
    return _want[case.name]


def aligner(case, options):
    al = S.Aligner(F.model(case), case.flag)
    for k, v in options.items():
        al.set_option(k, v)
    return al


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", F.NAMES)
def test_every_case_under_every_route(oracle, name, route):
    """the rows equal the oracle's whether or not a column segment verified (segment_reruns may move, the rows may not)"""
    case = F.build(name)
    want = expected(oracle, case)
    assert (want["valid"] == 1).all()
    with aligner(case, ROUTES[route]) as al:
        got = al.align_db(case.q, case.q_off)
        again = al.align_db(case.q, case.q_off)  # buffers reused
        assert al.profile()["non_finite_reads"] == 0
    assert_rows_equal(got, want)
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("name", F.NAMES)
def test_strip_reads_alone_with_every_strip_backing_off(oracle, name):
    """a batch of nothing but the reads of 2100 events, pass 2 of every strip with no head start"""
    case = F.build(name)
    want = expected(oracle, case)[STRIP_READS]
    q, q_off = F.subset(case, STRIP_READS)
    with aligner(case, MODES["strips_backoff"]) as al:
        got = al.align_db(q, q_off)
    assert_rows_equal(got, want)


@pytest.mark.parametrize("name", SECONDARY)
def test_secondaries(oracle, name):
    """secondary = 4 (secondary_strips for the reads of 2100 events): ranks 2 .. 5 of the candidate list, ordered on float bits"""
    case = F.build(name)
    want = expected(oracle, case)
    if name not in _want_sec:
        _want_sec[name] = secondary_rows(oracle, case.q, case.q_off, F.oracle_ref(oracle, case), case.flag)
    with aligner(case, {}) as al:
        al.set_secondary(4)
        al.set_option("secondary_strips", 1)
        prim = al.align_db(case.q, case.q_off)
        sec = al.secondary_rows()
    assert_rows_equal(prim, want)
    assert_sec_equal(sec, _want_sec[name])
    many = 1 if case.flag & F.DTW else 4  # --dtw-std: one candidate per contig, two contigs
    assert (sec["valid"][np.diff(case.q_off) <= 250, :many] == 1).all()  # (about the inputs: the list is full where windows are many)


@pytest.mark.parametrize("name", MAPS)
def test_event_maps(oracle, name):
    """sfa_event_maps of the primaries, every row on the device (map_strips for the reads of 2100 events), against the numpy model"""
    case = F.build(name)
    want = expected(oracle, case)
    with aligner(case, {"map_strips": 1}) as al:
        rows = al.align_db(case.q, case.q_off)
        maps = al.event_maps()
        on_host = al.maps_on_host
    assert_rows_equal(rows, want)
    assert on_host == 0 and len(maps) == len(want)
    rna, inv, std = bool(case.flag & F.RNA), bool(case.flag & F.INV), bool(case.flag & F.DTW)
    complete = 0
    for i, row in enumerate(want):
        model = M.row_map(row, F.events_of(case, i), case.forward, case.reverse, case.offs, rna, inv, std)
        if model is None:
            assert len(maps[i]) == 0, (name, i)
            continue
        complete += 1
        assert maps[i].dtype == np.int32 and maps[i].shape == model.shape and np.array_equal(maps[i], model), (name, i, maps[i][:6], model[:6])
    assert complete >= len(want) - 1, (name, complete)  # (about the inputs: the rows have maps)


def _feed(se, case, orc, after_chunk, starts=True):
    """the reads of 250 and 600 events into slots 0 .. 3, in chunks of 33, 1, 64 events and the rest; after every chunk the slots'
    rows equal align_batch on the prefixes"""
    data = [F.events_of(case, i) for i in SESSION_READS]
    slots = list(range(len(data)))
    used = 0
    for n in CHUNKS + (max(len(x) for x in data),):
        named = [sl for sl in slots if len(data[sl]) > used]
        chunks = [data[sl][used:used + n] for sl in named]
        off = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
        got = se.extend(named, np.concatenate(chunks), off)
        used += n
        prefixes = [data[sl][:used] for sl in named]
        assert_rows(got, orc.rows(prefixes), starts, (case.name, used))
        assert list(se.lengths(named)) == [len(p) for p in prefixes]
        after_chunk(named, prefixes)
    assert used >= 600


@pytest.mark.parametrize("name", SESSIONS)
def test_sessions_in_chunks(oracle, name):
    """... and the carried row of every (slot, contig, strand) read back is the oracle's last row: costs as bits, start columns too"""
    case = F.build(name)
    orc = Oracle(oracle, F.model(case), case.flag)

    def carried(named, prefixes):
        for sl, p in zip(named, prefixes):
            for contig, strand, cost, start in oracle.last_rows(p, orc.oref, case.flag):
                gc, gs = se.row(sl, contig, strand)
                assert np.array_equal(gc.view(np.uint32), cost.view(np.uint32)), (name, sl, len(p), contig, strand)
                assert np.array_equal(gs, start), (name, sl, len(p), contig, strand)

    with aligner(case, {}) as al, al.session(len(SESSION_READS)) as se:
        _feed(se, case, orc, carried)
        whole = se.extend(list(range(len(SESSION_READS))), np.zeros(0, np.float32), np.zeros(len(SESSION_READS) + 1, np.int64))
    assert_rows(whole, expected(oracle, case)[SESSION_READS], True, name)


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "no_start"])
def test_session_classes_on_denormal_costs(oracle, starts):
    """the class route (a u64 key of cost bits and column): with the second contig as the target, the best on-target and
    off-target column of every slot equal tests/targets_oracle.py over the ORACLE's last rows, after every chunk"""
    case = F.of_family("denormal_all")
    ref = F.model(case)
    orc = Oracle(oracle, ref, case.flag)
    targets = [(1, int(ref.st_offset[1]), int(ref.st_offset[1]) + int(ref.ref_lengths[1]) + 1)]
    mask = T.mask_of_wide(targets, ref.ref_lengths, ref.st_offset, 2)
    assert mask.sum() == 2 * case.lens[1] and not mask[:2 * case.lens[0]].any()

    def classes(named, prefixes):
        got = se.classes(named)
        for g, p in zip(got, prefixes):
            row = np.concatenate([cost for _, _, cost, _ in oracle.last_rows(p, orc.oref, case.flag)])
            assert (row > 0).all() and (row < np.float32(F.MIN_NORMAL)).all()  # (about the inputs: every key holds a denormal)
            want = T.classes_of_rows(row, mask, ref.ref_lengths, ref.st_offset, 2)
            assert g["valid"] == 1 and g["n_events"] == len(p)
            for side in ("on", "off"):
                assert np.float32(g[f"{side}_score"]).view(np.uint32) == np.float32(want[f"{side}_score"]).view(np.uint32), (len(p), side, g, want)
                for f in ("rid", "pos_end", "strand"):
                    assert int(g[f"{side}_{f}"]) == int(want[f"{side}_{f}"]), (len(p), side, f, g, want)

    with aligner(case, {}) as al, al.session(len(SESSION_READS), starts=starts) as se:
        se.set_targets(targets)
        assert se.target_columns() == int(mask.sum())
        _feed(se, case, orc, classes, starts)
