#!/usr/bin/env python3
"""Device-side decoding of zstd records next to zlib records (tools/blow5_decode_bench.py measures the zlib route alone):
decode_ms of sfa_align_blow5 for one batch of K records -- the same reads as zlib level 6 + svb-zd, as zstd level 3 + svb-zd
with the decoder's tables in HBM scratch (option zstd_tables 0) and in LDS (1) -- interleaved, `reps` rounds, medians and
spread.  Run on the GPU box:  python tools/zstd_decode_bench.py [K] [reps]"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sigfish_amd as S  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def records(path, k):
    b = open(path, "rb").read()
    (hl,) = struct.unpack_from("<I", b, 64)
    p = 68 + hl
    recs = []
    while b[p:p + 5] != b"5WOLB" and len(recs) < k:
        (sz,) = struct.unpack_from("<Q", b, p)
        recs.append(b[p + 8:p + 8 + sz])
        p += 8 + sz
    return b"".join(recs), np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)


def main():
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    d = tempfile.mkdtemp()
    files = {}
    for name, press in (("zlib", ["--record-press", "zlib"]), ("zstd", ["--record-press", "zstd", "--zstd-level", "3"])):
        files[name] = os.path.join(d, name + ".blow5")
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_blow5.py"), os.path.join(GOLD, "data", "sp1_dna.blow5"), files[name],
                        "--copies", str(k // 5 + 1), *press, "--signal-press", "svb-zd", "--jobs", "8"], check=True, capture_output=True)
    zl, zs = records(files["zlib"], k), records(files["zstd"], k)
    lv = np.fromfile(os.path.join(GOLD, "models", "syn6.f32"), np.float32)
    ref = S.RefModel.from_fasta(os.path.join(GOLD, "data", "nCoV-2019.reference.fasta"), lv, 6, 0, 250)
    sides = [("zlib level 6", zl, S.PRESS_ZLIB, 0), ("zstd level 3, tables in HBM", zs, S.PRESS_ZSTD, 0), ("zstd level 3, tables in LDS", zs, S.PRESS_ZSTD, 1)]
    ms = {name: [] for name, *_ in sides}
    with S.Aligner(ref, 0, device=0) as al:
        for name, (blob, off), press, tables in sides:  # warm-up: buffers grow, code objects load
            al.set_option("zstd_tables", tables)
            al.align_blow5(blob, off, press, True)
        for r in range(reps):
            for name, (blob, off), press, tables in sides:
                al.set_option("zstd_tables", tables)
                al.align_blow5(blob, off, press, True)
                pr = al.profile()
                assert pr["blow5_fallbacks"] == 0
                ms[name].append(pr["decode_ms"])
                print(f"round {r}: {name}: decode {pr['decode_ms']:.3f} ms ({len(blob) / 1e6:.1f} MB of records)", flush=True)
    for name, v in ms.items():
        print(f"K {k}: {name}: median {np.median(v):.3f} ms, min {min(v):.3f}, max {max(v):.3f} over {reps} rounds")


if __name__ == "__main__":
    main()
