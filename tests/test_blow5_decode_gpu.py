"""What the device-side BLOW5 reader decodes (blow5_fields_kernel, blow5_svb_kernel through sfa_decode_blow5_device), sample by
sample: records built here, at the sample counts around the svb kernel's 64-key round, in every code layout StreamVByte allows
(over-long ones and 4-byte codes included), in batches around the block's four waves, with and without zlib -- against a plain
numpy decoder written below (int64 running sum, truncated to int16) and against the host reader on the same records in a file.
Declined records get their status and leave their neighbours alone.  Everything is bit-exact."""
import struct
import zlib

import numpy as np
import pytest

import sigfish_amd as S
from tests.util import load_case
from tools.make_blow5 import svb_zd

pytestmark = pytest.mark.gpu

ID_MAX = 136  # kBlow5IdMax: the read id bytes a field row of the device holds (sfa_read_head_t holds 127)
COUNTS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1021, 4099]  # one round of the kernel: 64 keys = 256 samples


@pytest.fixture(scope="module")
def case():
    return load_case("dna_default")


@pytest.fixture(scope="module")
def al(case):
    c = case
    ref = S.RefModel.from_fasta(c["fasta"], c["levels"], c["k"], c["flag"], c["query_size"])
    with S.Aligner(ref, c["flag"], device=0) as a:
        yield a


# ---- the formats, written down from the layout in sigfish_amd/csrc/host/blow5.hpp ----

def svb_encode(x, nb=None):
    """running values x (each and each difference inside int32) -> svb-zd stream; nb: bytes per value (None: the fewest), so
    that a small value can be written over-long"""
    x = np.asarray(x, np.int64)
    d = np.diff(x, prepend=np.int64(0))
    assert np.all(np.abs(x) < 2**31) and np.all(np.abs(d) < 2**31)
    z = np.where(d >= 0, 2 * d, -2 * d - 1)
    least = 1 + (z >= 1 << 8) + (z >= 1 << 16) + (z >= 1 << 24)
    nb = least if nb is None else np.asarray(nb, np.int64)
    assert len(nb) == len(x) and np.all(nb >= least) and np.all(nb <= 4)
    n = len(x)
    codes = np.zeros((n + 3) // 4 * 4, np.uint8)
    codes[:n] = nb - 1
    keys = codes[0::4] | (codes[1::4] << 2) | (codes[2::4] << 4) | (codes[3::4] << 6)
    data = bytearray()
    for v, k in zip(z.tolist(), nb.tolist()):
        data += int(v).to_bytes(4, "little")[:k]
    return struct.pack("<I", n) + keys.astype(np.uint8).tobytes() + bytes(data)


def svb_decode(stream):
    """the reference of this file: svb-zd stream -> int16 samples, None where the data stream is not as long as its keys say"""
    (n,) = struct.unpack_from("<I", stream, 0)
    nk = (n + 3) // 4
    if len(stream) < 4 + nk:
        return None
    keys = np.frombuffer(stream, np.uint8, nk, 4)
    nb = (((keys[:, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)[:n]).astype(np.int64) + 1
    data = np.frombuffer(stream, np.uint8, offset=4 + nk)
    if int(nb.sum()) != len(data):
        return None
    start = np.cumsum(nb) - nb
    z = np.zeros(n, np.int64)
    for t in range(4):
        m = nb > t
        z[m] |= data[start[m] + t].astype(np.int64) << (8 * t)
    d = (z >> 1) ^ -(z & 1)
    return (np.cumsum(d) & 0xffff).astype(np.uint16).view(np.int16)  # int64 running sum, its low 16 bits


def payload(rid, signal, len_field, scaling=(8192.0, -243.0, 1437.976685), aux=b""):
    rid = rid if isinstance(rid, bytes) else rid.encode()
    return struct.pack("<H", len(rid)) + rid + struct.pack("<I4dQ", 0, *scaling, 4000.0, len_field) + signal + aux


def deflate(p):
    """zlib level 6 -- or stored blocks, where that would inflate to more than the slot the device gives a record (4x + 4 KB)"""
    z = zlib.compress(p, 6)
    return z if len(p) <= 4 * len(z) + 4096 else zlib.compress(p, 0)


def batch(payloads, rz):
    recs = [deflate(p) if rz else p for p in payloads]
    return b"".join(recs), np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64), recs


def write_blow5(path, recs, rz, ss):
    text = "@experiment_type\tgenomic_dna\n#char*\tuint32_t\tdouble\tdouble\tdouble\tdouble\tuint64_t\tint16_t*\n"
    text += "#read_id\tread_group\tdigitisation\toffset\trange\tsampling_rate\tlen_raw_signal\traw_signal\n"
    hdr = b"BLOW5\x01" + bytes([0, 2, 0]) + bytes([1 if rz else 0]) + struct.pack("<I", 1) + bytes([1 if ss else 0])
    hdr += b"\0" * (64 - len(hdr)) + struct.pack("<I", len(text)) + text.encode()
    with open(path, "wb") as f:
        f.write(hdr + b"".join(struct.pack("<Q", len(r)) + r for r in recs) + b"5WOLB")


# ---- code layouts: (running values, bytes per value or None) for n samples ----

def lay_one_byte(n, rng):
    return np.cumsum(rng.integers(-128, 128, n)), None


def lay_two_bytes(n, rng):
    return np.cumsum(rng.integers(128, 32768, n) * np.where(np.arange(n) % 2 == 0, 1, -1)), None


def lay_three_bytes(n, rng):  # samples alternating +-32767: differences of 65534 (the first one, 32767, written over-long)
    return np.where(np.arange(n) % 2 == 0, 32767, -32767), np.full(n, 3)


def lay_mixed(n, rng):  # every value 1-4 bytes at random, small values over-long among them; the running value stays inside +-2^30
    nb = rng.integers(1, 5, n)
    x = np.zeros(n, np.int64)
    cur = 0
    for i in range(n):
        top = min(1 << (8 * int(nb[i]) - 1), 1 << 30)
        m = int(rng.integers(0, top)) if rng.integers(0, 3) else int(rng.integers(0, min(top, 100)))
        cur += -m if cur > 0 or (cur == 0 and rng.integers(0, 2)) else m
        x[i] = cur
    return x, nb


def lay_four_bytes(n, rng):  # +-2^24 and +-2^30 in pairs: the running value returns, no decoder needs to wrap
    step = np.array([1 << 24, -(1 << 24), 1 << 30, -(1 << 30), -(1 << 24), 1 << 24, -(1 << 30), 1 << 30], np.int64)
    return np.cumsum(step[np.arange(n) % 8]) + rng.integers(-3, 4, n), None


def lay_int16_excursion(n, rng):  # sums that leave the int16 range both ways and come back: the truncation rule
    ramp = np.array([30000] * 5 + [-30000] * 10 + [30000] * 5, np.int64)
    return np.cumsum(ramp[np.arange(n) % 20]) + rng.integers(-5, 6, n), None


LAYOUTS = [lay_one_byte, lay_two_bytes, lay_three_bytes, lay_mixed, lay_four_bytes, lay_int16_excursion]


def special_layouts(rng):
    out = []
    for at in (255, 256, 257):  # one large difference exactly at / beside the first round's last value, taken back three values on
        d = rng.integers(-100, 101, 600)
        d[at] += 1 << 24
        d[at + 3] -= 1 << 24
        out.append((f"large_at_{at}", np.cumsum(d), None))
    for n in (256, 257, 512, 513):  # a round whose data stream is the full 1 024 bytes, then a round of 1-byte codes
        d = np.concatenate([np.where(np.arange(256) % 2 == 0, 1 << 30, -(1 << 30)), rng.integers(-100, 101, n - 256)])
        out.append((f"full_round_{n}", np.cumsum(d), None))
    d = rng.integers(-100, 101, 512)  # ... and the same 1 024 bytes from small values written over-long
    out.append(("full_round_overlong", np.cumsum(d), np.concatenate([np.full(256, 4), np.full(256, 1)])))
    return out


def svb_cases():
    rng = np.random.default_rng(11)
    cases = [(f"{lay.__name__}_{n}", *lay(n, rng)) for lay in LAYOUTS for n in COUNTS] + special_layouts(rng)
    out = []
    for k, (name, x, nb) in enumerate(cases):
        stream = svb_encode(x, nb)
        want = svb_decode(stream)
        assert want is not None and np.array_equal(want, np.asarray(x, np.int64).astype(np.int16)), name  # (the reference decodes what was meant)
        rid = f"{name}_{'x' * (k % 3)}"  # (ids of different lengths: the signal starts at any alignment)
        out.append((name, rid, payload(rid, stream, len(stream), aux=bytes(k % 5)), want))
    # canonical encodings by the tool that writes the benchmark files
    for n in (5, 257, 1021):
        raw = rng.integers(-32768, 32768, n).astype(np.int16)
        stream = svb_zd(raw)
        assert np.array_equal(svb_decode(stream), raw)
        out.append((f"make_blow5_{n}", f"tool_{n}", payload(f"tool_{n}", stream, len(stream)), raw))
    return out


SVB_CASES = svb_cases()  # built once, shared, never changed


def check_decoded(got, cases, recs):
    """cases: (name, read id, payload, samples) -- every record decoded, with its head and its samples"""
    status, heads, raw_off, samples = got
    assert list(status) == [0] * len(cases)
    assert [h["read_id"] for h in heads] == [c[1] for c in cases]
    assert [h["n_samples"] for h in heads] == [len(c[3]) for c in cases] and list(np.diff(raw_off)) == [len(c[3]) for c in cases]
    assert [(h["digitisation"], h["offset"], h["range"]) for h in heads] == [(8192.0, -243.0, 1437.976685)] * len(cases)
    assert [h["record_bytes"] for h in heads] == [len(r) for r in recs]
    for i, c in enumerate(cases):
        g = samples[raw_off[i]:raw_off[i + 1]]
        assert np.array_equal(g, c[3]), (c[0], np.flatnonzero(g != c[3])[:8])


def check_host_reader(path, cases):
    reads = list(S.Blow5File(path))
    assert [r[0] for r in reads] == [c[1] for c in cases]
    for (rid, meta, sig), c in zip(reads, cases):
        assert np.array_equal(sig, c[3]), c[0]


@pytest.mark.parametrize("rz", [0, 1])
def test_svb_every_count_and_code_layout(al, rz, tmp_path):
    blob, off, recs = batch([c[2] for c in SVB_CASES], rz)
    check_decoded(al.decode_blow5_device(blob, off, rz, 1), SVB_CASES, recs)
    write_blow5(str(tmp_path / "x.blow5"), recs, rz, 1)
    check_host_reader(str(tmp_path / "x.blow5"), SVB_CASES)


@pytest.mark.parametrize("rz", [0, 1])
@pytest.mark.parametrize("n_records", [1, 3, 4, 5, 9])
def test_svb_batch_shapes(al, rz, n_records):
    """records of different lengths in one call, around the four waves of a block"""
    pick = [SVB_CASES[(7 * i + 3 * n_records) % len(SVB_CASES)] for i in range(n_records)]
    blob, off, recs = batch([c[2] for c in pick], rz)
    check_decoded(al.decode_blow5_device(blob, off, rz, 1), pick, recs)


PLAIN_CASES = []
for _n in (0, 1, 63, 64, 65, 1000):
    for _id in ("even", "odd"):  # 4 and 3 id bytes: the samples start at an even and at an odd offset of the payload
        _raw = np.random.default_rng(_n).integers(-32768, 32768, _n).astype(np.int16)
        PLAIN_CASES.append((f"plain_{_n}_{_id}", f"{_id}", payload(_id, _raw.tobytes(), _n, aux=b"\x07" * (_n % 3)), _raw))


@pytest.mark.parametrize("rz", [0, 1])
def test_plain_int16_counts_and_alignments(al, rz, tmp_path):
    assert {(2 + len(c[1]) + 44) % 2 for c in PLAIN_CASES} == {0, 1}  # both alignments of the first sample
    blob, off, recs = batch([c[2] for c in PLAIN_CASES], rz)
    check_decoded(al.decode_blow5_device(blob, off, rz, 0), PLAIN_CASES, recs)
    write_blow5(str(tmp_path / "x.blow5"), recs, rz, 0)
    check_host_reader(str(tmp_path / "x.blow5"), PLAIN_CASES)


def _good(k):
    return SVB_CASES[(11 * k + 40) % len(SVB_CASES)]


def check_mixed(got, entries, recs):
    """entries: (case, expected status); a decoded record has its samples whatever its neighbours are, a record the fields
    declined counts none"""
    status, heads, raw_off, samples = got
    assert list(status) == [e[1] for e in entries]
    for i, (c, st) in enumerate(entries):
        assert heads[i]["record_bytes"] == len(recs[i])
        if st == 0:
            assert heads[i]["read_id"] == c[1] and heads[i]["n_samples"] == len(c[3])
            assert np.array_equal(samples[raw_off[i]:raw_off[i + 1]], c[3]), c[0]
        elif st != S.BLOW5_STREAM:
            assert raw_off[i + 1] == raw_off[i] and heads[i]["n_samples"] == 0 and heads[i]["read_id"] == ""


@pytest.mark.parametrize("rz", [0, 1])
def test_stream_one_byte_short_and_one_byte_long(al, rz, tmp_path):
    """the data stream must be exactly as long as the keys say, as the host reader demands (decode_svb_zd: data == end)"""
    x = np.cumsum(np.random.default_rng(5).integers(-300, 301, 300))
    stream = svb_encode(x)
    short = ("short", "short", payload("short", stream[:-1], len(stream) - 1, aux=b"\1\2\3"), None)
    long_ = ("long", "long", payload("long", stream + b"\0", len(stream) + 1), None)
    empty_long = ("empty_long", "empty_long", payload("empty_long", svb_encode([]) + b"\0", 5), None)
    assert svb_decode(stream[:-1]) is None and svb_decode(stream + b"\0") is None and svb_decode(svb_encode([]) + b"\0") is None
    entries = [(_good(0), 0), (short, S.BLOW5_STREAM), (_good(1), 0), (long_, S.BLOW5_STREAM), (empty_long, S.BLOW5_STREAM), (_good(2), 0), (_good(3), 0)]
    blob, off, recs = batch([e[0][2] for e in entries], rz)
    check_mixed(al.decode_blow5_device(blob, off, rz, 1), entries, recs)
    for bad in (1, 3, 4):  # the host reader refuses each of them
        write_blow5(str(tmp_path / "x.blow5"), recs[bad:bad + 1], rz, 1)
        with pytest.raises(S.SfaError):
            list(S.Blow5File(str(tmp_path / "x.blow5")))


@pytest.mark.parametrize("rz", [0, 1])
def test_declined_fields_leave_the_neighbours_alone(al, rz):
    """Records that end in the field parser with status -1 (tests/c/blow5_fields_host.cpp shows that they do, on the host under
    sanitizers): the svb kernel returns at once for them.  An empty signal and a declined record in the middle of a batch."""
    stream = svb_encode(np.arange(40))
    empty = ("empty", "empty", payload("empty", svb_encode([]), 4), np.zeros(0, np.int16))
    beyond = ("l_beyond", "l_beyond", payload("l_beyond", stream, len(stream) + 1), None)
    long_id = ("long_id", "i" * (ID_MAX + 1), payload("i" * (ID_MAX + 1), stream, len(stream)), None)
    entries = [(_good(4), 0), (empty, 0), (beyond, S.BLOW5_FIELDS), (_good(5), 0), (long_id, S.BLOW5_FIELDS), (_good(6), 0)]
    blob, off, recs = batch([e[0][2] for e in entries], rz)
    check_mixed(al.decode_blow5_device(blob, off, rz, 1), entries, recs)
    # plain int16: length fields whose doubling wraps
    sig = np.arange(10, dtype=np.int16)
    entries = [(PLAIN_CASES[10], 0), (("2^62", "a", payload("a", sig.tobytes(), 1 << 62), None), S.BLOW5_FIELDS), (PLAIN_CASES[7], 0),
               (("2^63-1", "b", payload("b", sig.tobytes(), (1 << 63) - 1), None), S.BLOW5_FIELDS), (PLAIN_CASES[11], 0),
               (("one_more", "c", payload("c", sig.tobytes(), 11), None), S.BLOW5_FIELDS)]
    blob, off, recs = batch([e[0][2] for e in entries], rz)
    check_mixed(al.decode_blow5_device(blob, off, rz, 0), entries, recs)


def test_record_that_does_not_inflate_and_small_capacity(al):
    cases = [_good(7), _good(8), _good(9)]
    blob, off, recs = batch([c[2] for c in cases], 1)
    recs[1] = recs[1][:-5]  # truncated zlib stream
    recs.append(zlib.compress(cases[0][2] + bytes(40000), 6))  # sound, but inflating beyond its slot of 4x + 4 KB
    blob, off = b"".join(recs), np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    check_mixed(al.decode_blow5_device(blob, off, 1, 1), [(cases[0], 0), (cases[1], S.BLOW5_INFLATE), (cases[2], 0), (cases[0], S.BLOW5_INFLATE)], recs)
    total = len(cases[0][3]) + len(cases[2][3])
    status, heads, raw_off, samples = al.decode_blow5_device(blob, off, 1, 1, capacity=total)
    assert raw_off[-1] == total and np.array_equal(samples[raw_off[2]:], cases[2][3])
    with pytest.raises(S.SfaError, match="room for"):
        al.decode_blow5_device(blob, off, 1, 1, capacity=total - 1)


def test_align_blow5_hands_hostile_records_to_the_host_reader(al, case):
    """sfa_align_blow5 itself: a length field of 2^62 or a surplus byte in the data stream sends the batch to the host reader
    (counted), whose answer is the call's: an error naming the record."""
    reads = list(S.Blow5File(case["blow5"]))[:6]
    scal = [(m["digitisation"], m["offset"], m["range"]) for _, m, _ in reads]
    for ss in (0, 1):
        sigs = [svb_zd(raw) if ss else raw.tobytes() for _, _, raw in reads]
        fields = [len(s) if ss else len(raw) for s, (_, _, raw) in zip(sigs, reads)]
        pls = [payload(rid, s, f, sc) for (rid, _, _), s, f, sc in zip(reads, sigs, fields, scal)]
        blob, off, _ = batch(pls, 0)
        before = al.profile()["blow5_fallbacks"]
        rows, info, heads = al.align_blow5(blob, off, 0, ss)
        assert al.profile()["blow5_fallbacks"] == before and [h["read_id"] for h in heads] == [r[0] for r in reads]
        bad = list(pls)
        bad[4] = payload(reads[4][0], sigs[4] + b"\0", fields[4] + 1, scal[4]) if ss else payload(reads[4][0], sigs[4], 1 << 62, scal[4])
        blob, off, _ = batch(bad, 0)
        with pytest.raises(S.SfaError, match="record 4"):
            al.align_blow5(blob, off, 0, ss)
        assert al.profile()["blow5_fallbacks"] == before + 1
        # ... and the context goes on: the sound batch again, same rows
        again = al.align_blow5(*batch(pls, 0)[:2], 0, ss)
        assert again[0].tobytes() == rows.tobytes() and al.profile()["blow5_fallbacks"] == before + 1
