"""The two record decompressors of the device with MORE THAN ONE RECORD PER WAVE (blow5_inflate_kernel, blow5_zstd_kernel<kLds>: one
record per lane, `lanes` records per wave, chosen by the host from the batch size -- 1 up to 4 x CUs records, then doubling), on
streams no compressor writes (tests/deflate_craft.py) between ordinary ones, refused records between sound ones, every sound
record in a slot of exactly its size with its neighbour's slot right behind it.  The expected answer of every DEFLATE stream is
zlib's, of every zstd frame the fixture's.  Only streams that the host harnesses run under ASan + UBSan are sent to the device
(tests/test_c_host.py: the crafted table; zlib's own streams: its random campaign; tests/test_zstd_cpu.py: the frames)."""
import math
import zlib

import numpy as np
import pytest
import torch  # (here, not in the fixture: torch finds no GPU once the library has opened the HIP runtime first, so it is loaded first)

import sigfish_amd as S
from tests import deflate_craft as D
from tests.test_deflate_craft_cpu import LANE_MAY_DECLINE
from tests.test_zstd_cpu import frames
from tests.util import load_case

pytestmark = pytest.mark.gpu
REFUSED_SLOT = 64  # a refused record's slot -- or the text its stream holds before the refusal, where that is longer (`room`)


@pytest.fixture(scope="module")
def al():
    c = load_case("dna_default")
    ref = S.RefModel.from_fasta(c["fasta"], c["levels"], c["k"], c["flag"], c["query_size"])
    with S.Aligner(ref, c["flag"], device=0) as a:
        yield a


@pytest.fixture(scope="module")
def cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def batch_size(cu, L):
    """a batch that runs L records per wave (inflate_lanes / zstd_lanes: lanes = L for 4 cu L / 2 < n <= 4 cu L), the smallest one
    plus 37, so that the last wave is partial (38 records over: 2 of 4, 6 of 8, 16 or 32 lanes; with 2 lanes it is full)"""
    n = 4 * cu * (L // 2) + 1 + 37
    assert 4 * cu * (L // 2) < n <= 4 * cu * L and (L == 2 or n % L != 0)
    return n


def entry(name, stream, may_decline=False, room=0):
    """(name, stream, zlib's answer, slot, may be declined): a sound record's slot is exactly its text"""
    want = D.expected(stream)
    return name, stream, want, len(want) if want is not None else max(REFUSED_SLOT, room), may_decline


def crafted_entries():
    """the crafted table as entries: (the ones that rotate through a batch, the ones over 1 KB that appear once)"""
    small, big = [], []
    for name, stream in D.CASES:
        e = entry(name, stream, name in LANE_MAY_DECLINE, D.INFO[name].room)
        (small if e[3] <= 1024 and len(stream) <= 2048 else big).append(e)
    assert len(small) > 600 and 20 < len(big) < 80
    return small, big


@pytest.fixture(scope="module")
def table():
    return crafted_entries()


def zlib_streams():
    """zlib's own streams of 0..600-byte payloads: levels 0, 1 and 9, Z_FIXED, memLevel 1 (many small dynamic blocks)"""
    rng = np.random.default_rng(7)
    out = []
    for k, size in enumerate((0, 1, 2, 3, 9, 31, 64, 100, 129, 200, 257, 258, 259, 300, 333, 400, 471, 512, 555, 600)):
        kind = k % 3
        if kind == 0:
            b = (rng.integers(0, 6, size) * rng.integers(0, 40, size)).astype(np.uint8).tobytes()  # what svb-zd signals look like
        elif kind == 1:
            b = (b"the quick brown fox jumps over the lazy dog " * 14)[:size]
        else:
            b = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        for level in (0, 1, 9):
            out.append(entry(f"zlib_{size}_level_{level}", zlib.compress(b, level)))
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
        out.append(entry(f"zlib_{size}_fixed", co.compress(b) + co.flush()))
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 1, zlib.Z_DEFAULT_STRATEGY)
        out.append(entry(f"zlib_{size}_memlevel_1", co.compress(b) + co.flush()))
    assert all(e[2] is not None for e in out)
    return out


@pytest.fixture(scope="module")
def zlib_entries():
    return zlib_streams()


def rotation(small, extra):
    """refused cases between sound ones, zlib's streams spread through the crafted ones; an odd count, so that record i = case
    i mod K has other neighbours in every wave and sits on another lane every time round"""
    sound = [e for e in small if e[2] is not None] + extra
    refused = [e for e in small if e[2] is None]
    cases = []
    for k in range(max(len(sound), len(refused))):
        cases += sound[k:k + 1] + refused[k:k + 1]
    if math.gcd(len(cases), 32) != 1:
        cases.append(extra[0])
    assert math.gcd(len(cases), 32) == 1
    return cases


def check(got, batch, L):
    """every record's answer against the reference; the first mismatches with their lane"""
    wrong = [(i, i % L, e[0], None if g is None else len(g)) for i, (g, e) in enumerate(zip(got, batch)) if not (g == e[2] or (e[4] and g is None))]
    assert not wrong, (len(wrong), wrong[:12])


@pytest.mark.parametrize("L", [2, 4, 8, 16, 32])
def test_inflate_with_several_records_per_wave(al, cu, table, zlib_entries, L):
    small, big = table
    cases = rotation(small, zlib_entries)
    K = len(cases)
    n = batch_size(cu, L)
    assert n > 4 * cu * (L // 2) and n <= 4 * cu * L  # this batch runs L records per wave
    batch = [cases[i % K] for i in range(n)]
    stride = n // (len(big) + 1)
    for j, e in enumerate(big):  # the texts of 1 .. 64 KB once per batch, each on another lane
        at = 3 + j * stride + j % L
        assert at < n
        batch[at] = e
    assert sum(e[3] for e in batch) < 24 << 20
    # the slots lie back to back: a byte written past one lands in the next record's text and shows there
    got = al.inflate_device([e[1] for e in batch], cap_factor=0, cap_extra=[e[3] for e in batch])
    check(got, batch, L)
    assert sum(g is not None for g in got) > n // 4 and sum(g is None for g in got) > n // 4
    # the records with bytes behind their stream: zlib's bytes or declined is what is asserted; by the decoder's code, declined
    assert all(g is None for g, e in zip(got, batch) if e[4])


def test_crafted_table_with_one_record_per_wave(al, cu, table):
    small, big = table
    cases = small + big
    assert len(cases) == len(D.CASES)
    for a in range(0, len(cases), 4 * cu):  # (at most 4 x CUs records a call: one per wave)
        part = cases[a:a + 4 * cu]
        got = al.inflate_device([e[1] for e in part], cap_factor=0, cap_extra=[e[3] for e in part])
        check(got, part, 1)
        assert all(g is None for g, e in zip(got, part) if e[4])


def test_crafted_headers_as_blow5_records(al, tmp_path):
    """The header cases in front of real record payloads, through the whole record decoder: CINFO 8 (the host reader refuses it, so the
    device must), a spoiled FCHECK -- SFA_BLOW5_INFLATE for them, their neighbours decode; CINFO 0..7, empty stored blocks and a
    fixed block without matches decode like zlib's own stream."""
    from tests.test_blow5_decode_gpu import payload, svb_encode, write_blow5
    rng = np.random.default_rng(11)
    sigs = [np.cumsum(rng.integers(-200, 201, 150 + 37 * k)).astype(np.int16) for k in range(14)]
    pays = [payload(f"read{k}", svb_encode(s), len(svb_encode(s))) for k, s in enumerate(sigs)]
    recs, want_status = [], []
    for k, p in enumerate(pays):
        body = zlib.compress(p, 6)[2:-4]
        if k == 3:
            recs.append(D.wrap(body, p, cinfo=8))
        elif k == 8:
            recs.append(D.wrap(body, p, fcheck_off=1))
        elif k == 10:
            recs.append(D.wrap(D.Deflate().stored(b"").stored(p[:50]).stored(b"").stored(p[50:], 1).done(), p))
        elif k == 12:
            recs.append(D.wrap(D.Deflate().fixed(0).lits(p[:70]).eob().stored(b"").fixed(1).lits(p[70:]).eob().done(), p))
        else:
            recs.append(D.wrap(body, p, cinfo=k % 8, flevel=k % 4))
        want_status.append(S.BLOW5_INFLATE if k in (3, 8) else 0)
        assert (D.expected(recs[-1]) == p) == (want_status[-1] == 0) and (want_status[-1] == 0 or D.expected(recs[-1]) is None)
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    status, heads, raw_off, samples = al.decode_blow5_device(b"".join(recs), off, 1, 1)
    assert list(status) == want_status
    for k, s in enumerate(sigs):
        if want_status[k] == 0:
            assert heads[k]["read_id"] == f"read{k}" and np.array_equal(samples[raw_off[k]:raw_off[k + 1]], s), k
        else:
            assert raw_off[k + 1] == raw_off[k]
    for k in (3, 8):  # the host reader refuses what the device declined
        write_blow5(str(tmp_path / "x.blow5"), recs[k:k + 1], 1, 1)
        with pytest.raises(S.SfaError):
            list(S.Blow5File(str(tmp_path / "x.blow5")))


def test_stale_input_behind_a_batch_is_not_read_as_the_record(al):
    """The device's input buffer keeps what an earlier call left behind the bytes of this one.  A record cut short, with the rest
    of its own stream still lying behind it from the call before, must be refused: the bit reader knows where the record ends."""
    rng = np.random.default_rng(5)
    text = (rng.integers(0, 6, 340) * rng.integers(0, 40, 340)).astype(np.uint8).tobytes()  # what svb-zd signals look like
    z = zlib.compress(text, 9)
    assert 200 < len(z) < 400
    assert al.inflate_device([z], cap_factor=0, cap_extra=len(text)) == [text]
    for m in (8, 23, 64, 65, 100, len(z) // 2, len(z) - 9, len(z) - 5, len(z) - 4, len(z) - 1):
        assert D.expected(z[:m]) is None
        assert al.inflate_device([z[:m]], cap_factor=0, cap_extra=len(text)) == [None], m
    assert al.inflate_device([z], cap_factor=0, cap_extra=len(text)) == [text]


@pytest.mark.parametrize("tables,L", [(1, 2), (1, 4), (0, 2), (0, 8), (0, 32)],
                         ids=["tables_in_lds_2", "tables_in_lds_4", "tables_in_hbm_2", "tables_in_hbm_8", "tables_in_hbm_32"])
def test_zstd_with_several_records_per_wave(al, cu, tables, L):
    fs = frames()
    sound = [(n, f, p, len(p), False) for n, s, p, f in fs if s and len(p) <= 4096]
    bad = [(n, f, None, 4 * len(f) + 20000, False) for n, s, p, f in fs if not s]  # (the slot tests/test_zstd_gpu.py gives them)
    assert len(sound) >= 20 and len(bad) >= 10
    cases = []
    for k in range(max(len(sound), len(bad))):
        cases += sound[k:k + 1] + bad[k:k + 1]
    if math.gcd(len(cases), 32) != 1:
        cases.append(sound[0])
    K = len(cases)
    assert math.gcd(K, 32) == 1
    n = batch_size(cu, L)
    assert n > 4 * cu * (L // 2) and n <= 4 * cu * L  # this batch runs L records per wave (zstd_lanes, up to 4 with the tables in LDS)
    assert L <= (4 if tables else 32)
    batch = [cases[i % K] for i in range(n)]
    al.set_option("zstd_tables", tables)
    try:
        got = al.zstd_device([e[1] for e in batch], cap_factor=0, cap_extra=[e[3] for e in batch])
    finally:
        al.set_option("zstd_tables", 1)  # the default
    check(got, batch, L)
    assert sum(g is not None for g in got) > n // 2
