"""A plain C99 program (tests/c/abi_host.c, gcc -std=c99 -pedantic) drives the C-ABI exactly as the reference's
align_db hook would; its rows must equal the oracle's.  Proves the header is C (not C++) and the boundary works
without Python in the loop."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.util import ROOT


def _build(tmp_path):
    exe = str(tmp_path / "abi_host")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "abi_host.c"), "-L", os.path.join(ROOT, "sigfish_amd", "lib"),
                           "-lsigfish_amd", "-Wl,-rpath," + os.path.join(ROOT, "sigfish_amd", "lib"), "-o", exe])
    return exe


def test_header_is_strict_c99(tmp_path):
    _build(tmp_path)  # -Werror -pedantic


@pytest.mark.gpu
@pytest.mark.parametrize("rna", [False, True])
def test_c_host_matches_oracle(tmp_path, oracle, rna):
    import sigfish_amd as S
    exe = _build(tmp_path)
    rng = np.random.default_rng(4 + rna)
    lens = [333, 57, 1200]
    fw = [rng.normal(size=n).astype(np.float32) for n in lens]
    rv = None if rna else [rng.normal(size=n).astype(np.float32) for n in lens]
    offs = [0, 2, 5] if rna else [0, 0, 0]
    flag = S.RNA if rna else 0
    reads = []
    for i in range(13):
        ne = int(rng.integers(0, 420)) if i != 5 else 0
        a = min(50, ne)
        b = min(a + 250, ne)
        reads.append((ne, a, b, rng.normal(size=ne).astype(np.float32)))
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", flag, len(lens), len(reads)))
        for i, n in enumerate(lens):
            f.write(struct.pack("<2i", n, offs[i]))
            f.write(fw[i].tobytes())
            if not rna:
                f.write(rv[i].tobytes())
        for ne, a, b, m in reads:
            f.write(struct.pack("<3q", ne, a, b))
            f.write(m.tobytes())
    subprocess.check_call([exe, fin, fout])
    got = np.fromfile(fout, S.RESULT_DTYPE)
    oref = oracle.RefSynth([f"c{i}" for i in range(3)], [n + 5 for n in lens], lens, offs, fw, rv)
    q = np.concatenate([m[a:b] for ne, a, b, m in reads])
    q_off = np.concatenate([[0], np.cumsum([b - a for ne, a, b, m in reads])]).astype(np.int64)
    want = oracle.align_batch(q, q_off, oref, flag, threads=4)
    assert np.array_equal(got["valid"], want["valid"])
    v = want["valid"] == 1
    assert got[v].tobytes() == want[v].tobytes()


def test_host_units_under_sanitizers(tmp_path):
    """ASan + UBSan over the host-side C++ (reader, inflate, StreamVByte, events, query selection, planner): CPU build
    only -- the GPU pool runs no sanitizers."""
    import shutil
    if not shutil.which("g++"):
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "sigfish_amd", "csrc")
    exe = str(tmp_path / "host_asan")
    units = [os.path.join(csrc, u) for u in ("sfa_host.cpp", "host/blow5.cpp", "host/inflate.cpp", "host/events.cpp", "host/refio.cpp", "host/sam.cpp")]
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
                            "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "host_asan.cpp"), *units, "-lz", "-lpthread"],
                           capture_output=True, timeout=600)
    if build.returncode != 0 and b"sanitize" in build.stderr:
        pytest.skip("toolchain without sanitizer runtimes")
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    data = os.path.join(ROOT, "tests", "golden")
    run = subprocess.run([exe, str(tmp_path), os.path.join(data, "data", "sp1_dna.blow5"), os.path.join(data, "data", "sequin_rna.blow5"),
                          os.path.join(data, "random", "rnd_dna.blow5")], capture_output=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr).decode()[-3000:]
    assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]


def test_buffer_type_under_sanitizers(tmp_path):
    """sfa::Buf (sfa_buf.hpp), the context's one buffer type, on a counting malloc / free policy under ASan + UBSan
    (tests/c/buf_host.cpp): no allocation below the capacity, growth by bytes + bytes / 8 + 256 with the old block freed once,
    a failing allocator leaves an empty buffer and SFA_ENOMEM with the message, moves transfer ownership, a scope of buffers
    ends with nothing live."""
    import shutil
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "buf_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I",
                            os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "c", "buf_host.cpp")],
                           capture_output=True, timeout=600)
    if build.returncode != 0 and b"sanitize" in build.stderr:
        pytest.skip("toolchain without sanitizer runtimes")
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    run = subprocess.run([exe], capture_output=True, timeout=120)
    assert run.returncode == 0 and b"0 live, 0 failures" in run.stdout, (run.stdout + run.stderr).decode()[-3000:]
    assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]
    assert b"LeakSanitizer" not in run.stderr, run.stderr.decode()[-3000:]


def test_device_inflate_lane_decoder_on_the_host_with_sanitizers(tmp_path):
    """The per-lane DEFLATE decoder of the device-side BLOW5 reader (blow5_kernels.hpp: the body of blow5_inflate_kernel),
    compiled for the host: against zlib on 4 000 random streams (every block type, encoder setting and window size,
    arbitrary bytes behind the stream), too-small output slots, corrupted streams -- under ASan + UBSan, which the GPU pool
    cannot run.  In front of them the crafted streams of tests/deflate_craft.py (answers from zlib): every sound one decodes into
    a heap block of exactly its size and is refused in one a byte smaller, every refused one is refused; the only sound streams
    declined are the ones with bytes behind them (the lane decoder takes the Adler-32 from the end of the record)."""
    import shutil
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "device_inflate_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(ROOT, "tests", "c", "device_inflate_host.cpp"), "-lz"], capture_output=True, timeout=600)
    if build.returncode != 0 and b"sanitize" in build.stderr:
        pytest.skip("toolchain without sanitizer runtimes")
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    from tests import deflate_craft as D
    from tests.test_deflate_craft_cpu import LANE_MAY_DECLINE
    flat = str(tmp_path / "cases.bin")
    D.flat_file(flat)
    run = subprocess.run([exe, "4000", "3", flat], capture_output=True, timeout=900)
    assert run.returncode == 0 and b"4000 iterations, 0 failures" in run.stdout, (run.stdout + run.stderr).decode()[-3000:]
    text = (run.stdout + run.stderr).decode()
    n_sound = sum(1 for _, s in D.CASES if D.expected(s) is not None)
    assert n_sound > 200 and len(D.CASES) - n_sound > 400
    assert f"crafted: {n_sound} sound, {len(D.CASES) - n_sound} refused, 0 failures" in text, text[-3000:]
    assert f"crafted: {len(LANE_MAY_DECLINE)} of the sound ones declined by design" in text, text[-3000:]
    assert "ERROR: AddressSanitizer" not in text and "runtime error" not in text, text[-3000:]


@pytest.mark.parametrize("sanitizers", [False, True])
def test_device_field_parser_on_the_host_beside_the_host_reader(tmp_path, sanitizers):
    """The field parser of the device-side BLOW5 reader (blow5_kernels.hpp: blow5_parse_fields, the body of blow5_fields_kernel),
    compiled for the host beside the host reader (tests/c/blow5_fields_host.cpp): payload lengths around the fixed fields, id
    lengths around the row, length fields up to 2^64-1 for both signal methods, 4 000 seeded mutations -- every payload in a
    heap block of exactly its length.  An accepted record has its signal inside the payload and the host reader's fields; a
    rejected one the host reader rejects as well.  Plain, and under ASan + UBSan, which the GPU pool cannot run."""
    import shutil
    if not shutil.which("g++"):
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "sigfish_amd", "csrc")
    exe = str(tmp_path / "blow5_fields_host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitizers else []
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", *flags, "-o", exe, os.path.join(ROOT, "tests", "c", "blow5_fields_host.cpp"),
                            os.path.join(csrc, "host", "blow5.cpp"), os.path.join(csrc, "host", "inflate.cpp"), "-lz", "-lpthread"],
                           capture_output=True, timeout=600)
    if sanitizers and build.returncode != 0 and b"sanitize" in build.stderr:
        pytest.skip("toolchain without sanitizer runtimes")
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    run = subprocess.run([exe, "4000", "1"], capture_output=True, timeout=600)
    assert run.returncode == 0 and b"4148 cases, 0 failures" in run.stdout, (run.stdout + run.stderr).decode()[-3000:]
    assert b"ERROR: AddressSanitizer" not in run.stderr and b"runtime error" not in run.stderr, run.stderr.decode()[-3000:]


def test_strip_heights_cover_every_query_length(tmp_path):
    """sfa::strip_rows_per_lane (sdtw_strips.hpp), compiled for the host with hipcc: for every query length from 2049 to 400 000
    events the strips cover the query, the last one holds at least one row, the height is an instantiated one -- a violation
    would index rows outside the query on the device."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "strip_rows")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "sigfish_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "c", "strip_rows_host.hip")], capture_output=True, timeout=600)
    assert build.returncode == 0, build.stderr.decode()[-2000:]
    run = subprocess.run([exe], capture_output=True, timeout=300)
    assert run.returncode == 0 and run.stdout.startswith(b"0 violations"), (run.stdout + run.stderr).decode()
    assert b"0.800" in run.stdout  # at least 80 % of the rows of any query's strips are query rows
