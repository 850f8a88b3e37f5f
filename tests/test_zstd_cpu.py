"""zstd-compressed BLOW5 files on the host: the decoder of sigfish_amd/csrc/zstd_lane.hpp as a stand-alone program under
ASan + UBSan (tests/c/zstd_lane_host.cpp), through the C-ABI (sfa_zstd_decompress / zstd_decompress) on every frame of
tests/golden/zstd/frames.npz, and behind the reader (Blow5File, shards, record ranges) on the zstd twins of the reference's
fixture files (tools/make_zstd_fixtures.py wrote both)."""
import glob
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib
from tests.util import GOLD, ROOT

ZSTD = os.path.join(GOLD, "zstd")
BIN = os.path.join(ROOT, "sigfish_amd", "bin", "sigfish-amd")


def frames():
    """[(name, sound, plain bytes, frame bytes)] of frames.npz"""
    z = np.load(os.path.join(ZSTD, "frames.npz"))
    return [(str(n), bool(z["sound"][k]), z[f"plain_{int(z['plain_of'][k])}"].tobytes(), z[f"frame_{k}"].tobytes()) for k, n in enumerate(z["names"])]


def zstd_files():
    return sorted(glob.glob(os.path.join(ZSTD, "*.blow5")))


def twin(path):
    """the reference's fixture file a zstd file was written from, and how many of its reads it holds"""
    name = os.path.basename(path)
    src = os.path.join(GOLD, "data", ("sp1_dna" if name.startswith("sp1_dna") else "sequin_rna") + ".blow5")
    return src


def test_fixture_folder_is_what_the_generator_writes():
    names = [os.path.basename(p) for p in zstd_files()]
    for base in ("sp1_dna", "sequin_rna"):
        for level in (1, 3, 19):
            assert f"{base}_zstd{level}.blow5" in names and f"{base}_zstd{level}_svb.blow5" in names
        assert f"{base}_zstd3_svb_xxh.blow5" in names
    fs = frames()
    assert sum(s for _, s, _, _ in fs) >= 40 and sum(not s for _, s, _, _ in fs) >= 10
    for p in zstd_files() + [os.path.join(ZSTD, "frames.npz")]:
        assert os.path.getsize(p) < (1 << 20)


def test_zstd_lane_decoder_on_the_host_with_sanitizers(tmp_path):
    """The decoder text the device compiles, as a stand-alone host program under ASan + UBSan: every fixture frame (sound ones
    byte-exact into a slot of exactly their size, malformed ones declined or within the slot), then -- where libzstd.so.1
    opens -- 2 000 random streams against libzstd, each also truncated and with flipped bytes.  Exit status = mismatches."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "zstd_lane_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "c", "zstd_lane_host.cpp"), "-ldl"], capture_output=True, timeout=600)
    if build.returncode != 0 and b"sanitize" in build.stderr:
        pytest.skip("toolchain without sanitizer runtimes")
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    flat = str(tmp_path / "frames.bin")
    fs = frames()
    with open(flat, "wb") as f:
        f.write(struct.pack("<I", len(fs)))
        for _, sound, plain, frame in fs:
            f.write(struct.pack("<III", 1 if sound else 0, len(plain), len(frame)) + plain + frame)
    run = subprocess.run([exe, flat, "2000", "3"], capture_output=True, timeout=900)
    text = (run.stdout + run.stderr).decode()
    assert run.returncode == 0, text[-3000:]
    n_sound, n_bad = sum(s for _, s, _, _ in fs), sum(not s for _, s, _, _ in fs)
    assert f"fixtures: {n_sound} sound, {n_bad} malformed, 0 failures" in text, text[-3000:]
    assert "2000 iterations, 0 failures" in text or "random campaign skipped" in text, text[-3000:]
    assert "ERROR: AddressSanitizer" not in text and "runtime error" not in text, text[-3000:]


def test_zstd_decompress_on_every_fixture_frame():
    L = _lib.load()
    for name, sound, plain, frame in frames():
        got = S.zstd_decompress(frame, cap=len(plain) if sound else None)
        if sound:
            assert got == plain, name
            if plain:  # a byte short: declined
                assert S.zstd_decompress(frame, cap=len(plain) - 1) is None, name
        else:
            assert got is None, name
        out = np.zeros(max(len(plain), 1) + 4 * len(frame) + 4096, np.uint8)
        rc = L.sfa_zstd_decompress(frame, len(frame), out.ctypes.data, out.size)
        assert rc == (len(plain) if sound else -1), name


def test_new_abi_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "sigfish_amd.h")).read()
    L = _lib.load()
    for sym in ("sfa_zstd_decompress", "sfa_zstd_device"):
        assert sym in _lib.SYMBOLS and sym + "(" in header and getattr(L, sym)
    for k, v in (("SFA_PRESS_NONE", 0), ("SFA_PRESS_ZLIB", 1), ("SFA_PRESS_ZSTD", 2)):
        assert f"#define {k} {v}" in header
    assert (S.PRESS_NONE, S.PRESS_ZLIB, S.PRESS_ZSTD) == (0, 1, 2)


@pytest.fixture(scope="module")
def twins():
    return {p: list(S.Blow5File(p)) for p in glob.glob(os.path.join(GOLD, "data", "*.blow5"))}


def same_reads(got, want):
    assert len(got) == len(want)
    for (rid, meta, sig), (wrid, wmeta, wsig) in zip(got, want):
        assert rid == wrid and meta == wmeta and sig.dtype == wsig.dtype and np.array_equal(sig, wsig), rid


@pytest.mark.parametrize("path", zstd_files(), ids=os.path.basename)
def test_blow5file_reads_zstd_files_like_their_twins(path, twins):
    """(fails on a reader that refuses record compression method 2: it cannot open the file)"""
    assert open(path, "rb").read(10)[9] == 2
    want = twins[twin(path)]
    got = list(S.Blow5File(path))
    assert 2 <= len(got) <= len(want)
    want = want[:len(got)]  # (the larger RNA variants hold the first reads)
    same_reads(got, want)
    for G in (2, 3, 7):  # the union of the shards is the whole file, in order
        parts = [list(S.Blow5File(path).select_shard(r, G)) for r in range(G)]
        same_reads([x for part in parts for x in part], want)
    same_reads(list(S.Blow5File(path).select_records(1, 1)), want[1:2])
    same_reads(list(S.Blow5File(path).select_records(1)), want[1:])
    same_reads(list(S.Blow5File(path).select_records(len(want))), [])


def test_cli_help_is_unchanged_and_ex_zd_signals_are_still_refused(tmp_path):
    helptext = subprocess.run([BIN, "dtw", "--help"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert helptext.stdout.decode() == open(os.path.join(ZSTD, "dtw_help.txt")).read()  # (as printed before zstd files were read)
    b = bytearray(open(os.path.join(ZSTD, "sp1_dna_zstd3_svb.blow5"), "rb").read())
    b[14] = 2  # signal_press ex-zd
    path = str(tmp_path / "exzd.blow5")
    open(path, "wb").write(bytes(b))
    with pytest.raises(S.SfaError, match=r"signal compression method 2 is not supported \(svb-zd or none only\)"):
        S.Blow5File(path)
    b[14], b[9] = 1, 3  # a record method nobody knows
    open(path, "wb").write(bytes(b))
    with pytest.raises(S.SfaError, match="record compression method 3 is not supported"):
        S.Blow5File(path)
