#!/usr/bin/env python3
"""Secondary-mapping fixtures (tests/golden/secondary/<case>.npz) from the reference's OWN code: for every golden case with
q <= 2048, the five aln_t entries update_aln() leaves per read (src/sigfish.c:507-626, driven in dtw_single's order, :828-960),
with subsequence() / std_dtw() and update_aln()'s traceback all taken from oracle/_ref/libsigfish_ref.so (make -C oracle ref).

    python tools/make_secondary_golden.py [--check]      (--check: rebuild in memory and compare with the committed files)
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from tests.util import GOLD, case_names, load_case  # noqa: E402

OUT = os.path.join(GOLD, "secondary")
CAP = 5  # SECONDARY_CAP, src/sigfish.h:41
MAX_Q = 2048


class AlnT(C.Structure):  # aln_t, src/sigfish.h:146-158
    _fields_ = [("rid", C.c_int32), ("pos_st", C.c_int32), ("pos_end", C.c_int32), ("score", C.c_float), ("score2", C.c_float),
                ("d", C.c_char), ("mapq", C.c_uint8), ("r2qevent_map", C.c_void_p), ("r2qevent_size", C.c_int32)]


assert C.sizeof(AlnT) == 40, C.sizeof(AlnT)


def _lib():
    L = O.reference_lib()
    if L is None:
        return None
    L.init_aln.restype = C.POINTER(AlnT)
    L.init_aln.argtypes = []
    L.update_aln.restype = None
    L.update_aln.argtypes = [C.POINTER(AlnT), C.c_float, C.c_int32, C.c_int32, C.c_char, C.POINTER(C.c_float), C.c_int32, C.c_int32]
    L.free_aln.restype = None
    L.free_aln.argtypes = [C.POINTER(AlnT)]
    return L


def _sha(arrs):
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a, "<f4").tobytes())
    return h.hexdigest()


def case_list():
    return [n for n in case_names() if load_case(n)["query_size"] <= MAX_Q]


def build_case(L, name):
    c = load_case(name)
    flag = c["flag"]
    rna = bool(flag & O.RNA)
    ref = O.gen_ref(O.read_fasta(c["fasta"]), c["levels"], c["k"], flag, c["query_size"])
    assert _sha(ref.forward) == str(c["fwd_sha256"]), name
    if ref.reverse is not None:
        assert _sha(ref.reverse) == str(c["rev_sha256"]), name
    q_off = c["q_off"]
    n = len(q_off) - 1
    f = {k: np.zeros((n, CAP), t) for k, t in (("rid", np.int32), ("pos_st", np.int32), ("pos_end", np.int32), ("score", np.float32),
                                               ("strand", np.uint8), ("flip_pos_st", np.int32), ("flip_pos_end", np.int32))}
    fp = C.POINTER(C.c_float)
    for i in range(n):
        ev = np.asarray(c["queries"][q_off[i]:q_off[i + 1]], np.float32)
        qlen = len(ev)
        query = ev[::-1].copy() if (rna and not (flag & O.INV)) else ev  # src/sigfish.c:860-866
        aln = L.init_aln()
        for j in range(ref.num_ref):
            strands = [(b"+", ref.forward[j], bool(flag & O.DTW))] + ([] if rna else [(b"-", ref.reverse[j], False)])
            for d, y, std in strands:
                rlen = len(y)
                cost = O.ref_std_dtw(query, y) if std else O.ref_subsequence(query, y)
                cp = np.ascontiguousarray(cost, np.float32)
                ptr = cp.ctypes.data_as(fp)
                if std:  # src/sigfish.c:914-917
                    L.update_aln(aln, float(cp[-1, -1]), j, rlen - 1, d, ptr, qlen, rlen)
                    continue
                last = cp[-1]
                for k in range(0, rlen, qlen):  # src/sigfish.c:891-901: first strict minimum of every window of qlen columns
                    w = last[k:k + qlen]
                    m = int(np.argmin(w))
                    assert np.isfinite(w[m]), (name, i, j)
                    L.update_aln(aln, float(w[m]), j, k + m, d, ptr, qlen, rlen)
        for l in range(CAP):
            a = aln[l]
            f["rid"][i, l], f["pos_st"][i, l], f["pos_end"][i, l] = a.rid, a.pos_st, a.pos_end
            f["score"][i, l] = a.score
            f["strand"][i, l] = a.d[0] if a.d else 0
            if a.rid >= 0:  # src/sigfish.c:969-975
                rl, off = int(ref.ref_lengths[a.rid]), int(ref.st_offset[a.rid])
                plus = a.d == b"+"
                f["flip_pos_st"][i, l] = (a.pos_st if plus else rl - a.pos_end) + off
                f["flip_pos_end"][i, l] = (a.pos_end if plus else rl - a.pos_st) + off
            else:
                f["flip_pos_st"][i, l] = f["flip_pos_end"][i, l] = -1
        L.free_aln(aln)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    L = _lib()
    if L is None:
        sys.exit("oracle/_ref/libsigfish_ref.so missing: make -C oracle ref")
    os.makedirs(OUT, exist_ok=True)
    bad = 0
    for name in case_list():
        f = build_case(L, name)
        path = os.path.join(OUT, name + ".npz")
        if args.check:
            z = np.load(path)
            same = all(np.array_equal(z[k], v) for k, v in f.items())
            bad += not same
            print(name, "ok" if same else "DIFFERS")
        else:
            np.savez_compressed(path, **f)
            print(name, os.path.getsize(path), "bytes")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
