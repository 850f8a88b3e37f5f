#!/usr/bin/env python3
"""make_zstd_fixtures.py -- writes tests/golden/zstd/: the reference's fixture files re-compressed record by record with zstd,
and frames.npz, (plain, frame) pairs and a short list of malformed frames for the decoder of sigfish_amd/csrc/zstd_lane.hpp.
Run once, on a machine with libzstd.so.1 (through ctypes, tools/make_blow5.py); the output is committed as data.

    python tools/make_zstd_fixtures.py

Every sound frame is checked against libzstd here (it decompresses to its plain bytes), every malformed frame is checked to be
refused by libzstd, and every sound record of the files fits 4x its size + 4 KB, the limit of the readers' route.
frames.npz: names[k], sound[k] (1: frame k decodes to its plain bytes; 0: malformed), frame_k, plain_of[k] = j, plain_j (uint8)."""
import os
import struct
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_blow5 import Zstd  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "zstd")
DATA = os.path.join(ROOT, "tests", "golden", "data")
MAGIC = struct.pack("<I", 0xFD2FB528)


def records(path):
    b = open(path, "rb").read()
    (hl,) = struct.unpack_from("<I", b, 64)
    p = 68 + hl
    recs = []
    while b[p:p + 5] != b"5WOLB":
        (sz,) = struct.unpack_from("<Q", b, p)
        recs.append(b[p + 8:p + 8 + sz])
        p += 8 + sz
    return b[9], b[14], recs


def block(kind, body, last=True, size=None):
    """a block header + body; kind 0 raw, 1 RLE, 2 compressed, 3 reserved"""
    n = len(body) if size is None else size
    return struct.pack("<I", (n << 3) | (kind << 1) | (1 if last else 0))[:3] + body


def lit_header(kind, n, fmt):
    """raw (0) / RLE (1) literals header in size format 0 (5 bits), 1 (12 bits), 3 (20 bits)"""
    if fmt == 0:
        return bytes([kind | (n << 3)])
    if fmt == 1:
        return struct.pack("<H", kind | (1 << 2) | (n << 4))
    return struct.pack("<I", kind | (3 << 2) | (n << 4))[:3]


def handmade():
    """frames libzstd does not write on demand: every size format of raw and RLE literals, headers, block types"""
    out = []
    for fmt, n in ((0, 31), (1, 1000), (3, 5000)):
        lit = bytes((7 * i + 3) & 255 for i in range(n))
        body = lit_header(0, n, fmt) + lit + b"\0"  # no sequences
        out.append((f"hand_raw_literals_fmt{fmt}", lit, MAGIC + bytes([0x00, 0x38]) + block(2, body)))  # window descriptor (128 KB), no content size
        body = lit_header(1, n, fmt) + b"Q" + b"\0"
        out.append((f"hand_rle_literals_fmt{fmt}", b"Q" * n, MAGIC + bytes([0x00, 0x38]) + block(2, body)))
    # content size of 4 and of 8 bytes, a dictionary id field that says 0, raw and RLE blocks
    p = bytes(range(200))
    out.append(("hand_fcs4_raw_block", p, MAGIC + bytes([0x20 | 0x80]) + struct.pack("<I", 200) + block(0, p)))
    out.append(("hand_fcs8_rle_block", b"z" * 300, MAGIC + bytes([0x20 | 0xC0]) + struct.pack("<Q", 300) + block(1, b"z", size=300)))
    out.append(("hand_dict_id_zero_two_blocks", p + p, MAGIC + bytes([0x20 | 0x80 | 1, 0]) + struct.pack("<I", 400) + block(0, p, last=False) + block(0, p)))
    out.append(("hand_window_descriptor_three_blocks", p + b"k" * 50 + p, MAGIC + bytes([0x00, 0x08]) + block(0, p, False) + block(1, b"k", False, 50) + block(0, p)))
    bad = [("bad_dictionary_id", MAGIC + bytes([0x20 | 1, 200, 5]) + block(0, p)),
           ("bad_reserved_block_type", MAGIC + bytes([0x20, 200]) + block(3, p)),
           ("bad_block_beyond_block_maximum", MAGIC + bytes([0x00, 0x00]) + block(0, bytes(1500))),  # 1 KB window, 1500-byte block
           ("bad_reserved_header_bit", MAGIC + bytes([0x20 | 8, 200]) + block(0, p)),
           ("bad_treeless_without_tree", MAGIC + bytes([0x20, 10]) + block(2, struct.pack("<I", 3 | (10 << 4) | (2 << 14))[:3] + b"\x01\x01" + b"\0"))]
    return out, bad


def first_block_sections(frame):
    """offsets of the first block of a one-frame input: (block start, literals section end = sequences section start, block end)"""
    fhd = frame[4]
    fcs = (1 if fhd & 0x20 else 0) if fhd >> 6 == 0 else (2, 4, 8)[(fhd >> 6) - 1]
    at = 5 + (0 if fhd & 0x20 else 1) + (fhd & 3 if fhd & 3 < 3 else 4) + fcs
    bh = frame[at] | (frame[at + 1] << 8) | (frame[at + 2] << 16)
    assert (bh >> 1) & 3 == 2, "first block is not compressed"
    b0 = at + 3
    t, sf = frame[b0] & 3, (frame[b0] >> 2) & 3
    if t < 2:
        hb = (1, 2, 1, 3)[sf]
        v = int.from_bytes(frame[b0:b0 + hb], "little")
        n = v >> 3 if hb == 1 else v >> 4
        lit_end = b0 + hb + (n if t == 0 else 1)
    else:
        hb, sb = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
        v = int.from_bytes(frame[b0:b0 + hb], "little")
        lit_end = b0 + hb + ((v >> (4 + sb)) & ((1 << sb) - 1))
    return b0, lit_end, b0 + (bh >> 3)


def main():
    z = Zstd()
    rng = np.random.default_rng(20240)
    os.makedirs(OUT, exist_ok=True)
    # ---- the fixture files ----
    total = 0
    for name in ("sp1_dna", "sequin_rna"):
        src = os.path.join(DATA, name + ".blow5")
        for svb in (False, True):
            for level, checksum in ((1, False), (3, False), (19, False), (3, True)):
                if checksum and not svb:
                    continue  # one of each file with the checksum flag
                dst = os.path.join(OUT, f"{name}_zstd{level}{'_svb' if svb else ''}{'_xxh' if checksum else ''}.blow5")
                # (the RNA file is 300 KB and more in every variant: one variant keeps all eight reads, the others the first two)
                first = [] if name == "sp1_dna" or (level == 3 and svb and not checksum) else ["--first", "2"]
                subprocess.run([sys.executable, os.path.join(HERE, "make_blow5.py"), src, dst, "--copies", "1", "--keep-ids", *first, "--record-press", "zstd", "--zstd-level", str(level),
                                "--signal-press", "svb-zd" if svb else "none", *(["--zstd-checksum"] if checksum else [])], check=True, capture_output=True)
                rp, sp, recs = records(dst)
                assert rp == 2 and sp == (1 if svb else 0)
                for r in recs:
                    plain = z.decompress(r, 4 * len(r) + 4096)
                    assert plain is not None, "a record does not fit 4x its size + 4 KB"
                assert os.path.getsize(dst) < (1 << 20)
                total += os.path.getsize(dst)
                print(f"{os.path.basename(dst)}: {len(recs)} records, {os.path.getsize(dst)} bytes")
    # ---- frames ----
    sound, bad = [], []

    def add(name, plain, frame):
        plain, frame = bytes(plain), bytes(frame)
        assert z.decompress(frame, len(plain) + 64) == plain, name
        sound.append((name, plain, frame))

    def add_bad(name, frame):
        if z.decompress(bytes(frame), 1 << 20) is not None:  # (what the format forbids and this libzstd lets pass is named here)
            assert name in ("bad_block_beyond_block_maximum", "bad_reserved_header_bit"), name
            print(f"{name}: libzstd {z.version()} takes it")
        bad.append((name, b"", bytes(frame)))

    deltas = lambda n: (rng.integers(0, 6, n) * rng.integers(0, 40, n)).astype(np.uint8).tobytes()  # noqa: E731
    for n in (0, 1, 2, 1023, 1024, 1025, 16383, 16384):
        d = deltas(n)
        add(f"deltas_{n}_l3", d, z.compress(d, 3))
        add(f"random_{n}_l1", r := rng.integers(0, 256, n, dtype=np.uint8).tobytes(), z.compress(r, 1))
    add("zeros_5000", bytes(5000), z.compress(bytes(5000), 3))
    add("zeros_200000", bytes(200000), z.compress(bytes(200000), 3))
    add("six_symbols_3000", r := rng.integers(0, 6, 3000, dtype=np.uint8).tobytes(), z.compress(r, 19))
    add("six_symbols_60", r := rng.integers(0, 6, 60, dtype=np.uint8).tobytes() * 2, z.compress(r, 19))
    add("two_hundred_symbols_6000", r := rng.integers(0, 200, 6000, dtype=np.uint8).tobytes(), z.compress(r, 3))
    add("skewed_255_symbols_20000", r := np.minimum(rng.geometric(0.03, 20000), 255).astype(np.uint8).tobytes(), z.compress(r, 3))
    phrase = (b"the quick brown fox " * 400)[:7777]
    for level in (1, 3, 19):
        add(f"phrase_l{level}", phrase, z.compress(phrase, level))
    add("phrase_aaaa", b"abcd" + b"a" * 3000 + b"abcdabcdabcdabcd" * 30, z.compress(b"abcd" + b"a" * 3000 + b"abcdabcdabcdabcd" * 30, 3))
    # several blocks of low-entropy bytes: treeless literals, repeat modes, repeat offsets across blocks
    words = [deltas(int(rng.integers(3, 40))) for _ in range(300)]
    low = b"".join(words[int(k)] for k in rng.integers(0, 300, 20000))[:150000]
    assert 140000 <= len(low) <= 300000
    for level in (1, 3, 19):
        add(f"low_entropy_{len(low)}_l{level}", low, z.compress(low, level))
    # a match further back than 2^17: offset codes with more than 16 extra bits
    a = rng.integers(0, 4, 135000, dtype=np.uint8).tobytes()
    far = a + deltas(500) + a[:3000]
    add("far_match_l19", far, z.compress(far, 19))
    add("streamed_no_content_size", low, z.compress_stream(low, 3))
    add("streamed_small_no_content_size", phrase[:300], z.compress_stream(phrase[:300], 3))
    add("checksum", phrase, z.compress(phrase, 3, checksum=True))
    add("checksum_multi_block", low, z.compress(low, 3, checksum=True))
    add("checksum_empty", b"", z.compress(b"", 3, checksum=True))
    add("two_frames", phrase + deltas(1000)[:0] + bytes(100), z.compress(phrase, 3) + z.compress(bytes(100), 1))
    skip = struct.pack("<II", 0x184D2A53, 11) + b"hello world"
    add("skippable_in_front", phrase, skip + z.compress(phrase, 3))
    add("skippable_between_and_behind", phrase + phrase, z.compress(phrase, 3) + skip + z.compress(phrase, 19, checksum=True) + skip)
    hand, hand_bad = handmade()
    for name, plain, frame in hand:
        add(name, plain, frame)
    # ---- malformed ----
    f = z.compress(np.minimum(rng.geometric(0.03, 20000), 255).astype(np.uint8).tobytes(), 3)  # Huffman literals in four streams
    g = z.compress(phrase + deltas(4000), 19)
    add_bad("truncated_in_header", g[:5])
    b0, lit_end, end = first_block_sections(g)
    add_bad("truncated_in_literals", g[:b0 + (lit_end - b0) // 2])
    add_bad("truncated_in_sequences", g[:lit_end + (end - lit_end) // 2])
    add_bad("truncated_last_byte", g[:-1])
    b0f, lit_end_f, _ = first_block_sections(f)
    add_bad("truncated_in_huffman_streams", f[:lit_end_f - 100])
    # a flipped bit in an FSE table description: the first compressed table of the sequences section of a frame that has one
    h = None
    for cand in (z.compress(low[:60000], 19), z.compress(low[:60000], 3), g):
        _, le, _ = first_block_sections(cand)
        nb = 1 if cand[le] < 128 else (2 if cand[le] < 255 else 3)
        modes = cand[le + nb]
        if (modes >> 6) == 2:  # literal lengths FSE-compressed: its description follows the modes byte
            h = bytearray(cand)
            h[le + nb + 1] ^= 0x08  # accuracy log + 8: beyond the limit of 9
            break
    assert h is not None, "no frame with an FSE-compressed literal-length table"
    add_bad("flipped_bit_in_fse_table", h)
    # a match that reaches in front of the frame's output: the frame was compressed against a prefix the decoder does not have
    z._params(3, False)
    z.L.ZSTD_CCtx_refPrefix.restype = z.C.c_size_t
    z.L.ZSTD_CCtx_refPrefix.argtypes = [z.C.c_void_p, z.C.c_char_p, z.C.c_size_t]
    prefix = deltas(3000)
    assert not z.L.ZSTD_isError(z.L.ZSTD_CCtx_refPrefix(z.cctx, prefix, len(prefix)))
    body = prefix[500:2500] + deltas(200)
    cap = z.L.ZSTD_compressBound(len(body))
    dst = z.C.create_string_buffer(cap)
    n = z.L.ZSTD_compress2(z.cctx, dst, cap, body, len(body))
    assert not z.L.ZSTD_isError(n)
    add_bad("offset_before_start_of_output", dst.raw[:n])
    c = bytearray(z.compress(phrase, 3, checksum=True))
    c[-1] ^= 0x40
    add_bad("wrong_checksum", c)
    small = z.compress(deltas(100), 3)
    assert small[4] == 0x20 and small[5] == 100  # single segment, one byte of content size
    add_bad("content_size_too_small", small[:5] + bytes([99]) + small[6:])
    add_bad("content_size_too_large", small[:5] + bytes([101]) + small[6:])
    for name, frame in hand_bad:
        add_bad(name, frame)
    allf = sound + bad
    plains = sorted({plain for _, plain, _ in allf}, key=lambda b: (len(b), b))  # (several frames of one input share it)
    arrays = {"names": np.array([n for n, _, _ in allf]), "sound": np.array([1] * len(sound) + [0] * len(bad), np.uint8),
              "plain_of": np.array([plains.index(plain) for _, plain, _ in allf], np.int32)}
    for j, plain in enumerate(plains):
        arrays[f"plain_{j}"] = np.frombuffer(plain, np.uint8)
    for k, (_, _, frame) in enumerate(allf):
        arrays[f"frame_{k}"] = np.frombuffer(frame, np.uint8)
    path = os.path.join(OUT, "frames.npz")
    np.savez_compressed(path, **arrays)
    total += os.path.getsize(path)
    print(f"frames.npz: {len(sound)} sound, {len(bad)} malformed, {os.path.getsize(path)} bytes; folder {total} bytes (libzstd {z.version()})")


if __name__ == "__main__":
    main()
