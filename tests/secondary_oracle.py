"""The reference's sorted top-5 candidate list per read (init_aln / update_aln / dtw_single, src/sigfish.c:507-626, 828-983),
restated on the oracle's cost matrices: what `--secondary yes` prints behind each primary."""
import numpy as np

from sigfish_amd.api import RESULT_DTYPE, RNA, DTW, INV

CAP = 5  # SECONDARY_CAP, src/sigfish.h:41


def _update_aln(aln, score, rid, pos, d, pos_st):
    l = 0
    while l < CAP and not (score > aln[l][0]):
        l += 1
    if l == 0:
        return
    for m in range(l - 1):
        aln[m] = aln[m + 1]
    aln[l - 1] = (np.float32(score), rid, pos_st, pos, d)


def top5(O, events, ref, flag):
    """aln[0] (worst) .. aln[4] (best) of one read as (score, rid, pos_st, pos_end, strand), columns of the strand's own array."""
    ev = np.asarray(events, np.float32)
    qlen = len(ev)
    rna = bool(flag & RNA)
    query = ev[::-1].copy() if (rna and not (flag & INV)) else ev
    aln = [(np.float32(np.inf), -1, -1, -1, 0)] * CAP
    if qlen == 0:
        return aln
    for j in range(len(ref.forward)):
        strands = [("+", ref.forward[j], bool(flag & DTW))]
        if not rna:
            strands.append(("-", ref.reverse[j], False))
        for d, y, std in strands:
            rlen = len(y)
            if std:
                cost = O.std_dtw(query, y)
                pos = rlen - 1
                _update_aln(aln, cost[-1, pos], j, pos, d, O.path_start(cost, pos))
                continue
            cost = O.subsequence(query, y)
            last = cost[-1]
            for k in range(0, rlen, qlen):  # windows of qlen columns, first strict minimum (src/sigfish.c:891-901)
                w = last[k:k + qlen]
                pos = k + int(np.argmin(w))
                _update_aln(aln, w.min(), j, pos, d, O.path_start(cost, pos))
    return aln


def secondary_rows(O, events, q_off, ref, flag, n_sec=4):
    """Expected sfa_secondary_rows(): [n_reads, 4] of RESULT_DTYPE, best secondary first."""
    n = len(q_off) - 1
    out = np.zeros((n, 4), RESULT_DTYPE)
    out["rid"] = -1
    out["pos_st"] = -1
    out["pos_end"] = -1
    out["score"] = np.inf
    out["score2"] = np.inf
    for i in range(n):
        aln = top5(O, events[q_off[i]:q_off[i + 1]], ref, flag)
        for k in range(n_sec):
            sc, rid, st, en, d = aln[3 - k]
            if rid < 0 or not np.isfinite(sc):
                continue
            rl, off = int(ref.ref_lengths[rid]), int(ref.st_offset[rid])
            r = out[i, k]
            r["valid"] = 1
            r["rid"] = rid
            r["strand"] = ord(d)
            r["pos_st"] = (st if d == "+" else rl - en) + off  # src/sigfish.c:971-975
            r["pos_end"] = (en if d == "+" else rl - st) + off
            r["score"] = sc
            r["score2"] = aln[2 - k][0] if k < 3 else np.float32(np.inf)
            r["mapq"] = 0
    return out


def load_fixture(name):
    """tests/golden/secondary/<name>.npz (tools/make_secondary_golden.py): aln[0..4] per read from the reference's update_aln."""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "secondary", name + ".npz"))
    return {k: z[k] for k in z.files}


def rows_from_fixture(f, n_sec=4):
    """The rows sfa_secondary_rows() must return for a fixture: [n_reads, 4], best secondary (aln[3]) first."""
    n = f["rid"].shape[0]
    out = np.zeros((n, 4), RESULT_DTYPE)
    out["rid"] = -1
    out["pos_st"] = -1
    out["pos_end"] = -1
    out["score"] = np.inf
    out["score2"] = np.inf
    for k in range(n_sec):
        l = 3 - k
        ok = (f["rid"][:, l] >= 0) & np.isfinite(f["score"][:, l])
        r = out[:, k]
        r["valid"] = ok
        r["rid"] = np.where(ok, f["rid"][:, l], -1)
        r["strand"] = np.where(ok, f["strand"][:, l], 0)
        r["pos_st"] = np.where(ok, f["flip_pos_st"][:, l], -1)
        r["pos_end"] = np.where(ok, f["flip_pos_end"][:, l], -1)
        r["score"] = np.where(ok, f["score"][:, l], np.inf)
        r["score2"] = np.where(ok, f["score"][:, l - 1] if l > 0 else np.inf, np.inf)
        out[:, k] = r
    return out
