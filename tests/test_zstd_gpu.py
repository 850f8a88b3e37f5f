"""zstd-compressed BLOW5 records on the device (blow5_zstd_kernel, zstd_kernels.hpp): the decompressor alone on the frames of
tests/golden/zstd/frames.npz, the record decoder on the zstd fixture files against their zlib twins and the host reader, malformed
frames between sound records (declined, the host reader takes the batch), and the command line on the zstd files.  Only frames the
host harness (tests/test_zstd_cpu.py, the same decoder text under ASan) runs are sent to the device; nothing random."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import sigfish_amd as S
from tests.test_zstd_cpu import ZSTD, frames, zstd_files
from tests.util import GOLD, ROOT, load_case

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "sigfish_amd", "bin", "sigfish-amd")


def records(path):
    """(record_press, signal_svb, [record bytes]) of a BLOW5 file, framing only"""
    b = open(path, "rb").read()
    (hl,) = struct.unpack_from("<I", b, 64)
    p = 68 + hl
    recs = []
    while b[p:p + 5] != b"5WOLB":
        (sz,) = struct.unpack_from("<Q", b, p)
        recs.append(b[p + 8:p + 8 + sz])
        p += 8 + sz
    return b[9], b[14] == 1, recs


def offsets(recs):
    return np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)


@pytest.fixture(scope="module")
def al():
    c = load_case("dna_default")
    ref = S.RefModel.from_fasta(c["fasta"], c["levels"], c["k"], c["flag"], c["query_size"])
    with S.Aligner(ref, c["flag"], device=0) as a:
        yield a


@pytest.mark.parametrize("tables", [0, 1], ids=["tables_in_hbm", "tables_in_lds"])
def test_device_zstd_on_the_fixture_frames(al, tables):
    al.set_option("zstd_tables", tables)
    try:
        fs = frames()
        sound = [(n, p, f) for n, s, p, f in fs if s]
        # every slot as large as the largest content (factor 0, the largest as extra)
        got = al.zstd_device([f for _, _, f in sound], cap_factor=0, cap_extra=max(len(p) for _, p, _ in sound))
        for (name, plain, _), g in zip(sound, got):
            assert g == plain, name
        # malformed frames between sound records: declined, the neighbours decode
        bad = [(n, f) for n, s, _, f in fs if not s]
        mixed, want = [], []
        for k, (name, frame) in enumerate(bad):
            n, plain, f = sound[k % len(sound)]
            if len(plain) > 20000:
                n, plain, f = sound[0]
            mixed += [f, frame]
            want += [plain, None]
        mixed.append(sound[1][2])
        want.append(sound[1][1])
        got = al.zstd_device(mixed, cap_factor=4, cap_extra=20000)
        assert got == want, [k for k, (g, w) in enumerate(zip(got, want)) if g != w]
        # a sound frame larger than its slot is declined, not an overrun
        big = next(f for n, p, f in sound if n.startswith("zeros_200000"))
        assert al.zstd_device([big], cap_factor=4, cap_extra=4096) == [None]
    finally:
        al.set_option("zstd_tables", 1)  # the default


@pytest.mark.parametrize("path", [p for p in zstd_files() if "sp1_dna" in p or "zstd3_svb.blow5" in p], ids=os.path.basename)
def test_decode_blow5_device_equals_the_zlib_twin_and_the_host_reader(al, path):
    press, svb, recs = records(path)
    assert press == 2
    reads = list(S.Blow5File(path))
    zrecs = [zlib.compress(S.zstd_decompress(r), 6) for r in recs]  # the zlib twin: the same payloads, deflated
    reps = (70 + len(recs) - 1) // len(recs)
    for n in (1, 63, 64, 65, len(recs)):  # wave and block edges of one lane per record
        rs, zs, want = (recs * reps)[:n], (zrecs * reps)[:n], (reads * reps)[:n]
        status, heads, raw_off, samples = al.decode_blow5_device(b"".join(rs), offsets(rs), S.PRESS_ZSTD, svb)
        zstatus, zheads, zraw_off, zsamples = al.decode_blow5_device(b"".join(zs), offsets(zs), S.PRESS_ZLIB, svb)
        assert not status.any() and not zstatus.any()
        assert np.array_equal(raw_off, zraw_off) and np.array_equal(samples, zsamples)
        for h, zh, (rid, meta, sig), r in zip(heads, zheads, want, rs):
            assert {k: v for k, v in h.items() if k != "record_bytes"} == {k: v for k, v in zh.items() if k != "record_bytes"}
            assert h["read_id"] == rid and h["n_samples"] == len(sig) and h["record_bytes"] == len(r)
            assert (h["digitisation"], h["offset"], h["range"]) == (meta["digitisation"], meta["offset"], meta["range"])
        assert np.array_equal(samples, np.concatenate([sig for _, _, sig in want]))


def test_malformed_record_is_declined_and_the_host_reader_takes_the_batch(al):
    """A malformed frame between sound records: SFA_BLOW5_INFLATE for it, its neighbours decode, align_blow5 hands the batch to the
    host reader (blow5_fallbacks + 1).  The host reader runs the same decoder, so what the device declines for being malformed
    the host refuses by name: the call ends with an error for that record.  (A zstd record that only the DEVICE declines does
    not exist -- one decoder text, one slot rule on both sides -- so there are no host rows to compare on such a batch.)"""
    path = os.path.join(ZSTD, "sp1_dna_zstd3_svb.blow5")
    press, svb, recs = records(path)
    recs = recs * 2
    want = al.align_blow5(b"".join(recs), offsets(recs), S.PRESS_ZSTD, svb)
    bad = [f for n, s, _, f in frames() if not s and n in ("wrong_checksum", "truncated_in_sequences", "offset_before_start_of_output")]
    assert len(bad) == 3
    for frame in bad:
        rs = list(recs)
        rs[3] = frame
        status, heads, raw_off, samples = al.decode_blow5_device(b"".join(rs), offsets(rs), S.PRESS_ZSTD, svb)
        assert status[3] == S.BLOW5_INFLATE and not np.delete(status, 3).any()
        assert heads[2]["read_id"] == want[2][2]["read_id"] and heads[4]["read_id"] == want[2][4]["read_id"]
        before = al.profile()["blow5_fallbacks"]
        with pytest.raises(S.SfaError, match="record 3"):  # nobody can read it: the host reader names it
            al.align_blow5(b"".join(rs), offsets(rs), S.PRESS_ZSTD, svb)
        assert al.profile()["blow5_fallbacks"] == before + 1


@pytest.mark.parametrize("path", [os.path.join(ZSTD, n) for n in ("sp1_dna_zstd1.blow5", "sp1_dna_zstd19_svb.blow5", "sp1_dna_zstd3_svb_xxh.blow5", "sequin_rna_zstd3_svb.blow5")],
                         ids=os.path.basename)
def test_align_blow5_on_zstd_files_equals_align_raw(path):
    c = load_case("rna_default" if "sequin" in path else "dna_default")
    press, svb, recs = records(path)
    reads = list(S.Blow5File(path))
    raw = np.concatenate([sig for _, _, sig in reads])
    raw_off = np.concatenate([[0], np.cumsum([len(sig) for _, _, sig in reads])]).astype(np.int64)
    meta = np.array([(m["digitisation"], m["offset"], m["range"]) for _, m, _ in reads])
    ref = S.RefModel.from_fasta(c["fasta"], c["levels"], c["k"], c["flag"], c["query_size"])
    with S.Aligner(ref, c["flag"], device=0) as a:
        want_rows, want_info, want_ev = a.align_raw(raw, raw_off, meta, c["prefix_size"], c["query_size"], return_events=True)
        rows, info, heads, ev = a.align_blow5(b"".join(recs), offsets(recs), press, svb, c["prefix_size"], c["query_size"], return_events=True)
        assert rows.tobytes() == want_rows.tobytes() and info.tobytes() == want_info.tobytes() and ev.tobytes() == want_ev.tobytes()
        assert [h["read_id"] for h in heads] == [rid for rid, _, _ in reads]
        assert [h["record_bytes"] for h in heads] == [len(r) for r in recs]
        p = a.profile()
        assert p["blow5_fallbacks"] == 0 and p["decode_ms"] > 0, a._L.sfa_last_error()


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    import itertools
    d = tmp_path_factory.mktemp("models")
    out = {}
    for k in (5, 6):
        lv = np.fromfile(os.path.join(GOLD, "models", f"syn{k}.f32"), np.float32)
        p = d / f"syn{k}.model"
        with open(p, "w") as f:
            f.write(f"#k\t{k}\nkmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\n")
            for kmer, v in zip(itertools.product("ACGT", repeat=k), lv):
                f.write("%s\t%.4f\t1.5000\t1.0\t1.0\n" % ("".join(kmer), v))
        out[k] = str(p)
    return out


@pytest.mark.parametrize("parse", ["--gpu-parse", "--host-parse", None])
@pytest.mark.parametrize("name,file", [("dna_default", "sp1_dna_zstd3_svb.blow5"), ("rna_default", "sequin_rna_zstd3_svb.blow5")])
def test_cli_dtw_on_zstd_files_prints_the_golden_output(name, file, parse, models):
    c = load_case(name)
    cmd = [BIN, "dtw", "--kmer-model", models[c["k"]], "--verbose", "0", *[str(a) for a in c["args"]], *([parse] if parse else []), c["fasta"], os.path.join(ZSTD, file)]
    out = subprocess.run(cmd, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert out.stdout.decode() == c["out_text"]


def test_cli_realtime_on_a_zstd_file_prints_what_it_prints_for_the_zlib_file(models, tmp_path):
    import sys
    c = load_case("dna_default")
    zl = str(tmp_path / "zlib.blow5")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_blow5.py"), c["blow5"], zl, "--copies", "1", "--keep-ids", "--compress"], check=True, capture_output=True)
    outs = []
    for path in (zl, os.path.join(ZSTD, "sp1_dna_zstd3_svb.blow5")):
        r = subprocess.run([BIN, "realtime", "--kmer-model", models[c["k"]], "--verbose", "0", c["fasta"], path], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1] and outs[0]
