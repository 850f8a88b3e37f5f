"""The event detection kernels (sigfish_amd/csrc/events_kernels.hpp) at their own edges, seen whole: through the testing hook
sfa_detect_events_device every read's complete event table, both t-statistics and the kernel that produced each read's sums and
peaks come back, and are held against the host twin (S.detect_events) and the model of tests/events_model.py.  The inputs
(tests/events_edge_cases.py) sit on every tile, block, chunk and list boundary the kernels have, for both chemistries;
tests/test_events_edges_cpu.py shows without a GPU that they do, and which route every read has to take."""
import numpy as np
import pytest

import sigfish_amd as S
from tests import events_edge_cases as E
from tests import events_model as M

pytestmark = pytest.mark.gpu

CHEM = [pytest.param(False, id="dna"), pytest.param(True, id="rna")]


def _ref(rna):
    rng = np.random.default_rng(11)
    lens = [700, 350]
    fw = [rng.normal(size=n).astype(np.float32) for n in lens]
    rv = None if rna else [rng.normal(size=n).astype(np.float32) for n in lens]
    return S.RefModel([f"c{i}" for i in range(len(lens))], [n + 5 for n in lens], lens, [0] * len(lens), fw, rv)


def _aligner(rna):
    return S.Aligner(_ref(rna), S.RNA if rna else 0)


def _first_difference(got, want):
    """-> None, or text naming the first event at which the two tables differ"""
    if len(got) != len(want):
        return f"{len(got)} events, expected {len(want)}"
    for f in ("start", "length", "mean", "stdv"):
        a, b = got[f], want[f]
        eq = (a == b) if f == "start" else ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b)))
        if not eq.all():
            e = int(np.argmin(eq))
            return f"event {e}: {f} {a[e]!r}, expected {b[e]!r} (event {got[e]}, expected {want[e]})"
    return None


def _check_tables(batch, tables, want, routes, what):
    for i, ((name, raw, _), got, ev) in enumerate(zip(batch, tables, want)):
        diff = _first_difference(got, ev)
        assert diff is None, f"{what}: read {i} ({name}, {len(raw)} samples, route {routes[i]}): {diff}"


@pytest.mark.parametrize("rna", CHEM)
def test_batch_a_whole_tables_statistics_and_routes(rna):
    batch, model, want = E.batch_a(rna), E.model_a(rna), E.host_a(rna)
    raw, off, sc = E.pack(batch)
    with _aligner(rna) as al:
        tables, routes, t1, t2 = al.detect_events_device(raw, off, sc, tstats=True)
    assert [len(t) for t in tables] == [len(ev) for ev in want]   # n_events
    _check_tables(batch, tables, want, routes, "batch (a)")
    for i, ((name, r, _), m) in enumerate(zip(batch, model)):
        for f, t in (("t1", t1), ("t2", t2)):
            got = t[off[i]:off[i + 1]]
            assert E.same_bits(got, m[f]), f"read {i} ({name}): {f} differs first at sample {int(np.argmax(got.view(np.uint32) != m[f].view(np.uint32)))}"
    # which kernel took which read
    seq_peaks = (routes & 2) != 0
    seq_prefix = (routes & 1) != 0
    names = [b[0] for b in batch]
    acc = np.array([m["spec"][0] for m in model])
    why = np.array([m["spec"][1] for m in model])
    exact = np.array([m["cert"][0] for m in model])
    assert np.array_equal(seq_peaks, ~acc), [(names[i], why[i], int(routes[i])) for i in np.nonzero(seq_peaks == acc)[0]]
    assert np.array_equal(seq_prefix, ~exact), [(names[i], int(routes[i])) for i in np.nonzero(seq_prefix == exact)[0]]
    assert np.sum(~seq_peaks) >= 20 and not seq_peaks[32:64].any()
    assert np.sum(seq_peaks & (why == "list")) >= 2 and np.sum(seq_peaks & (why == "nosync")) >= 2
    assert np.array_equal(seq_peaks & (why == "range"), np.array([E.chunk(len(b[1])) < 24 or E.chunk(len(b[1])) > 288 for b in batch]))
    assert seq_prefix.any() and not seq_prefix.all()


@pytest.mark.parametrize("rna", CHEM)
def test_batch_a_is_the_same_under_every_ev_parallel(rna):
    batch, want = E.batch_a(rna), E.host_a(rna)
    raw, off, sc = E.pack(batch)
    seen = {}
    with _aligner(rna) as al:
        for opt in (3, 2, 1, 0):
            al.set_option("ev_parallel", opt)
            tables, routes, t1, t2 = al.detect_events_device(raw, off, sc, tstats=True)
            _check_tables(batch, tables, want, routes, f"ev_parallel {opt}")
            seen[opt] = (tables, t1.tobytes(), t2.tobytes())
            assert np.all(routes & 1) == (not opt & 1) and np.all(routes & 2) == (not opt & 2), (opt, routes)
    for opt in (2, 1, 0):   # byte for byte (field by field: the records have four bytes of padding)
        assert seen[opt][1:] == seen[3][1:], opt
        for i, (a, b) in enumerate(zip(seen[opt][0], seen[3][0])):
            assert all(a[f].tobytes() == b[f].tobytes() for f in ("start", "length", "mean", "stdv")), (opt, i, batch[i][0])


@pytest.mark.parametrize("rna", CHEM)
def test_one_read_alone(rna):
    batch = E.batch_b(rna)
    raw, off, sc = E.pack(batch)
    want = [E.host_events(r, s, rna) for _, r, s in batch]
    with _aligner(rna) as al:
        tables, routes = al.detect_events_device(raw, off, sc)
    _check_tables(batch, tables, want, routes, "batch (b)")
    assert routes[0] == 2   # exact sums; lane 63 of the speculative picker holds two samples and meets nothing


@pytest.mark.parametrize("rna", CHEM)
def test_8192_reads_are_offered_to_the_speculative_picker_and_8193_are_not(rna):
    big = E.batch_c(rna, 8193)
    want = {}
    for name, r, s in big:   # most reads are the same 40 samples: one host run per distinct read
        if (name, len(r)) not in want:
            want[(name, len(r))] = E.host_events(r, s, rna)
    got = {}
    with _aligner(rna) as al:
        for n_reads in (8192, 8193):
            batch = E.batch_c(rna, n_reads)
            raw, off, sc = E.pack(batch)
            assert off[-1] < 1_000_000
            tables, routes = al.detect_events_device(raw, off, sc)
            _check_tables(batch, tables, [want[(b[0], len(b[1]))] for b in batch], routes, f"batch (c), {n_reads} reads")
            ten = np.array([b[0].startswith("ordinary_1600") for b in batch])
            assert ten.sum() == 10
            if n_reads == 8192:
                assert not np.any(routes[ten] & 2)
                assert np.all(routes[np.array([len(b[1]) < 1473 for b in batch])] & 2)
            else:
                assert np.all(routes & 2)
            got[n_reads] = tables
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[8192], got[8193]))


@pytest.mark.parametrize("rna", CHEM)
def test_batch_path_agrees_with_the_hook(rna):
    batch = E.batch_a(rna)
    raw, off, sc = E.pack(batch)
    with _aligner(rna) as al:
        tables, routes = al.detect_events_device(raw, off, sc)
        rows, info, qev = al.align_raw(raw, off, sc, 50, 250, return_events=True)
    assert list(info["n_events"]) == [len(t) for t in tables]
    kept = 0
    for i, (name, _, _) in enumerate(batch):
        a, b = int(info["qstart"][i]), int(info["qend"][i])
        if b > a:
            kept += 1
            for f in ("start", "length", "stdv"):
                assert np.array_equal(qev[i][:b - a][f], tables[i][f][a:b]), (i, name, f)
    assert kept > 40


def test_refusals():
    raw = np.zeros(100, np.int16)
    sc = np.array([E.SCALE], np.float64)
    with _aligner(False) as al:
        tables, routes = al.detect_events_device(np.zeros(0, np.int16), np.zeros(1, np.int64), np.zeros((0, 3)))
        assert tables == [] and len(routes) == 0   # n_reads == 0 is fine
        tables, routes = al.detect_events_device(np.zeros(0, np.int16), np.zeros(4, np.int64), np.repeat(sc, 3, axis=0))
        assert [len(t) for t in tables] == [0, 0, 0] and np.all(routes & 2)   # ... and so are reads without samples
        for off in ([1, 100], [0, 60, 50]):
            with pytest.raises(S.SfaError, match="raw_off"):
                al.detect_events_device(raw, np.array(off, np.int64), np.repeat(sc, len(off) - 1, axis=0))
        L, h = al._L, al._h
        ro = np.array([0, 100], np.int64)
        ev = np.zeros(102, S.EVENT_DTYPE)
        nev, rt = np.zeros(1, np.int32), np.zeros(1, np.int32)
        import ctypes as C
        from sigfish_amd import _lib
        good = [raw.ctypes.data_as(C.POINTER(C.c_int16)), ro.ctypes.data_as(_lib.i64p), sc.ctypes.data_as(C.POINTER(C.c_double)), 1,
                ev.ctypes.data_as(C.c_void_p), nev.ctypes.data_as(_lib.i32p), rt.ctypes.data_as(_lib.i32p), None, None]
        assert L.sfa_detect_events_device(h, *good) == 0
        for k in (0, 1, 2, 4, 5, 6):   # a null argument where n_reads > 0
            args = list(good)
            args[k] = None
            assert L.sfa_detect_events_device(h, *args) == -1, k
        args = list(good)
        args[3] = -1
        assert L.sfa_detect_events_device(h, *args) == -1
        assert L.sfa_detect_events_device(None, *good) == -1
    with S.Aligner(_ref(False), 0, devices=[0, 0]) as two:   # a multi-device context
        with pytest.raises(S.SfaError, match="single-device"):
            two.detect_events_device(raw, np.array([0, 100], np.int64), sc)
