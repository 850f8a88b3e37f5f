"""Event maps from the device (sfa_event_maps, sdtw_path.hpp) against the per-row host routine sfa_r2qevent_map, which
tests/test_host_stages.py pins to the reference's path_to_map: every rows-per-lane class and lane width of the band fill,
mixed lengths in one batch, many short contigs, both strands, RNA with and without --invert, --dtw-std; tie-heavy quantised
values and normal ones.  Wherever every query has at most 2048 events and the scratch budget is the default, no row may have
gone to the in-call host routine (maps_on_host == 0): the fallback cannot hide a broken kernel."""
import numpy as np
import pytest

import sigfish_amd as S
from tests.util import device_lists, load_case

pytestmark = pytest.mark.gpu


def _arr(rng, n, quant):
    return (rng.integers(-6, 7, n) / 4).astype(np.float32) if quant else rng.normal(size=n).astype(np.float32)


def _small_ref(rng, lens, rna, quant=True):
    fw = [_arr(rng, n, quant) for n in lens]
    rv = None if rna else [_arr(rng, n, quant) for n in lens]
    return S.RefModel([f"c{i}" for i in range(len(lens))], [n + 5 for n in lens], lens,
                      rng.integers(0, 3, len(lens)) if rna else [0] * len(lens), fw, rv)


def _batch(rng, qlens, quant=True):
    q_off = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int64)
    return _arr(rng, int(q_off[-1]), quant), q_off


def host_map(ref, flag, q, q_off, read, row):
    """sfa_r2qevent_map for one row; None where it declines (unaligned row, no complete map)."""
    if not row["valid"] or row["rid"] < 0:
        return None
    x = q[q_off[read]:q_off[read + 1]]
    ev = np.zeros(len(x), S.EVENT_DTYPE)
    ev["mean"] = x
    j = int(row["rid"])
    y = ref.forward[j] if row["strand"] == ord("+") else ref.reverse[j]
    try:
        return S.r2qevent_map(row, ev, 0, len(x), y, int(ref.st_offset[j]), flag)
    except S.SfaError:
        return None


def assert_maps(got, ref, flag, q, q_off, rows, read_of_row=None):
    assert len(got) == len(rows)
    n_maps = 0
    for k, row in enumerate(rows):
        want = host_map(ref, flag, q, q_off, k if read_of_row is None else int(read_of_row[k]), row)
        if want is None:
            assert len(got[k]) == 0, k
            continue
        n_maps += 1
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want), (k, row, got[k][:6], want[:6])
    return n_maps


CASES = {  # (flag, contig lengths, query lengths): the table of tests/test_secondary_gpu.py
    "dna_r16": (0, [900, 300, 57], [7, 25, 64, 65, 100, 128, 129, 250, 256, 0]),
    "dna_r32": (0, [2600, 700], [257, 300, 512, 513, 1000, 1024, 1025, 2048]),
    "rna": (S.RNA, [1500, 800, 33], [25, 100, 250, 300, 700]),
    "rna_inv": (S.RNA | S.INV, [1200, 400], [64, 250, 600]),
    "rna_std": (S.RNA | S.DTW, [400, 300, 250, 90], [25, 100, 250, 400]),
    "rna_fullref": (S.RNA | S.REF, [2100, 640], [100, 250, 520, 1100]),
    "many_contigs": (0, [160] * 40, [25, 100, 250]),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("quant", [True, False], ids=["quantised", "normal"])
def test_maps_equal_host_routine(case, quant):
    flag, lens, ql = CASES[case]
    rng = np.random.default_rng(1000 * quant + len(case))
    ref = _small_ref(rng, lens, bool(flag & S.RNA), quant)
    qlens = np.array(list(ql) * 3)
    rng.shuffle(qlens)
    q, q_off = _batch(rng, qlens, quant)
    with S.Aligner(ref, flag) as al:
        rows = al.align_db(q, q_off)
        maps = al.event_maps()
        assert al.maps_on_host == 0
        again = al.event_maps(rows)  # the call may be repeated until the next submit
        assert al.maps_on_host == 0
    n = assert_maps(maps, ref, flag, q, q_off, rows)
    assert n >= (len(qlens) - 3) * (0 if flag & S.DTW else 1)
    assert all(np.array_equal(a, b) for a, b in zip(maps, again))


@pytest.mark.parametrize("flag", [0, S.RNA, S.RNA | S.DTW], ids=["dna", "rna", "rna_std"])
def test_maps_of_secondary_rows(flag):
    rng = np.random.default_rng(31 + flag)
    ref = _small_ref(rng, [1300, 500, 260], bool(flag & S.RNA))
    qlens = np.array([25, 64, 100, 250, 300, 600, 1100, 250])
    q, q_off = _batch(rng, qlens)
    with S.Aligner(ref, flag) as al:
        al.set_secondary(4)
        prim = al.align_db(q, q_off)
        sec = al.secondary_rows()
        rows = np.concatenate([prim, sec.reshape(-1)])
        ror = np.concatenate([np.arange(len(prim)), np.repeat(np.arange(len(prim)), 4)]).astype(np.int32)
        maps = al.event_maps(rows, ror)
        assert al.maps_on_host == 0
    assert sec["valid"].sum() > len(prim)
    assert_maps(maps, ref, flag, q, q_off, rows, ror)


def test_entry_points():
    """submit / wait and align_events leave their queries behind like align_db."""
    rng = np.random.default_rng(11)
    ref = _small_ref(rng, [1500, 400], False)
    qlens = np.array([250, 100, 64, 300, 250, 0, 700])
    q, q_off = _batch(rng, qlens)
    with S.Aligner(ref, 0) as al:
        al.submit(q, q_off)
        rows = al.wait()
        assert assert_maps(al.event_maps(), ref, 0, q, q_off, rows) == 6
        assert al.maps_on_host == 0
        tables = []
        for i in range(len(qlens)):
            ev = np.zeros(int(qlens[i]) + 3, S.EVENT_DTYPE)
            ev["mean"][3:] = q[q_off[i]:q_off[i + 1]]
            tables.append(ev if qlens[i] else None)
        rows2 = al.align_events(tables, [3] * len(qlens), [3 + int(x) for x in qlens])
        assert rows2.tobytes() == rows.tobytes()
        assert assert_maps(al.event_maps(), ref, 0, q, q_off, rows2) == 6
        assert al.maps_on_host == 0


def _load_raw(path):
    raws, scal = [], []
    for _, meta, raw in S.Blow5File(path):
        raws.append(raw)
        scal.append([meta["digitisation"], meta["offset"], meta["range"]])
    off = np.concatenate([[0], np.cumsum([len(r) for r in raws])]).astype(np.int64)
    return np.concatenate(raws), off, np.array(scal, np.float64)


def _records(path):
    import struct
    b = open(path, "rb").read()
    (hl,) = struct.unpack_from("<I", b, 64)
    p = 68 + hl
    recs = []
    while b[p:p + 5] != b"5WOLB":
        (sz,) = struct.unpack_from("<Q", b, p)
        recs.append(b[p + 8:p + 8 + sz])
        p += 8 + sz
    return b[9] == 1, b[14] == 1, recs


def _maps_from_query_events(ref, flag, rows, info, qev):
    out = []
    for i, r in enumerate(rows):
        if not r["valid"] or r["rid"] < 0:
            out.append(None)
            continue
        j = int(r["rid"])
        y = ref.forward[j] if r["strand"] == ord("+") else ref.reverse[j]
        ql = int(info["qend"][i] - info["qstart"][i])
        out.append(S.r2qevent_map(r, np.ascontiguousarray(qev[i]), 0, ql, y, int(ref.st_offset[j]), flag))
    return out


@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("name", ["dna_default", "rna_default", "rna_dtw_std", "rna_q1000"])
def test_golden_raw_and_blow5(name, devices):
    """sfa_align_raw and sfa_align_blow5: the queries the device normalised itself serve the maps."""
    c = load_case(name)
    ref = S.RefModel.from_fasta(c["fasta"], c["levels"], c["k"], c["flag"], c["query_size"])
    raw, off, scal = _load_raw(c["blow5"])
    rz, ss, recs = _records(c["blow5"])
    rec_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    kw = {"devices": devices} if devices else {}
    with S.Aligner(ref, c["flag"], **kw) as al:
        rows, info, qev = al.align_raw(raw, off, scal, c["prefix_size"], c["query_size"], return_events=True)
        maps = al.event_maps()
        assert al.maps_on_host == 0
        got = al.align_blow5(b"".join(recs), rec_off, rz, ss, c["prefix_size"], c["query_size"])
        assert got[0].tobytes() == rows.tobytes()
        maps5 = al.event_maps()
        assert al.maps_on_host == 0
    want = _maps_from_query_events(ref, c["flag"], rows, info, qev)
    assert sum(w is not None for w in want) > 0
    for k, w in enumerate(want):
        for m in (maps[k], maps5[k]):
            assert (len(m) == 0) if w is None else np.array_equal(m, w), k


@pytest.mark.parametrize("devs", device_lists())
def test_two_shards(devs):
    rng = np.random.default_rng(13)
    ref = _small_ref(rng, [1200, 300], False)
    qlens = rng.choice([25, 64, 250, 300, 600], size=37)
    q, q_off = _batch(rng, qlens)
    with S.Aligner(ref, 0, devices=devs) as al:
        al.set_secondary(2)
        rows = al.align_db(q, q_off)
        maps = al.event_maps()
        assert al.maps_on_host == 0
        # rows in any order, with their reads named: every shard takes the rows of its own reads
        sec = al.secondary_rows()
        pick = rng.permutation(len(rows))[:20]
        some = np.concatenate([rows[pick], sec[pick, 0]])
        ror = np.concatenate([pick, pick]).astype(np.int32)
        maps2 = al.event_maps(some, ror)
        assert al.maps_on_host == 0
    assert assert_maps(maps, ref, 0, q, q_off, rows) == len(rows)
    assert_maps(maps2, ref, 0, q, q_off, some, ror)


def test_small_budget_slices_and_host_rows():
    """A budget of 64 KiB: the short rows go through in several slices, the rows whose own moves exceed it on the host."""
    rng = np.random.default_rng(17)
    ref = _small_ref(rng, [2500, 800], False)
    qlens = np.array([25, 64, 100, 250, 300, 25, 600, 1100, 64, 2048, 250, 100] * 2)
    q, q_off = _batch(rng, qlens)
    with S.Aligner(ref, 0) as al:
        rows = al.align_db(q, q_off)
        full = al.event_maps()
        assert al.maps_on_host == 0
        al.set_option("map_scratch_bytes", 64 << 10)
        small = al.event_maps()
        on_host = al.maps_on_host
    assert 0 < on_host < len(rows)
    assert assert_maps(small, ref, 0, q, q_off, rows) == len(rows)
    assert all(np.array_equal(a, b) for a, b in zip(full, small))


def test_long_reads_go_to_the_host_routine():
    rng = np.random.default_rng(19)
    ref = _small_ref(rng, [5000, 900], False)
    qlens = [250, 2100, 64, 3000, 700]
    q, q_off = _batch(rng, qlens)
    with S.Aligner(ref, 0) as al:
        rows = al.align_db(q, q_off)
        maps = al.event_maps()
        assert al.maps_on_host == 2
    assert assert_maps(maps, ref, 0, q, q_off, rows) == 5


def test_refusals():
    import torch
    rng = np.random.default_rng(23)
    ref = _small_ref(rng, [700, 300], False)
    q, q_off = _batch(rng, [100, 250, 64])
    with S.Aligner(ref, 0) as al:
        with pytest.raises(S.SfaError, match="no align call"):
            al.event_maps(np.zeros(3, S.RESULT_DTYPE))
        rows = al.align_db(q, q_off)
        with pytest.raises(S.SfaError, match="3 reads"):
            al.event_maps(rows[:2])  # identity numbering needs every read's row
        with pytest.raises(S.SfaError, match="names read"):
            al.event_maps(rows[:2], [0, 3])
        # too small a gap in map_off
        import ctypes as C
        from sigfish_amd import _lib
        off = np.zeros(4, np.int64)
        off[1:] = np.cumsum(rows["pos_end"] - rows["pos_st"] + 1)
        off[3] -= 1
        pairs = np.zeros((int(off[-1]) + 1, 2), np.int32)
        rc = al._L.sfa_event_maps(al._h, rows.ctypes.data_as(C.c_void_p), None, 3, off.ctypes.data_as(_lib.i64p),
                                  pairs.ctypes.data_as(_lib.i32p), None)
        assert rc == -4  # SFA_ERANGE
        # the queries of sfa_align_batch_device are the caller's
        dq = torch.from_numpy(q).cuda()
        dout = torch.zeros(3 * rows.itemsize, dtype=torch.uint8, device="cuda")
        al.align_db_device(dq.data_ptr(), q_off, 3, dout.data_ptr())
        with pytest.raises(S.SfaError, match="sfa_align_batch_device"):
            al.event_maps(rows)
        assert_maps(al.event_maps(al.align_db(q, q_off)), ref, 0, q, q_off, rows)
