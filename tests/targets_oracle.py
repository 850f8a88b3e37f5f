"""Python restatement of the target-class rules (sigfish_amd/csrc/target_rules.hpp) for the tests: the column mask of a list of
targets, and the classes of a slot from its carried rows.  test_session_targets_cpu.py compares the mask with the C++ header's;
test_session_targets_gpu.py compares Session.classes with classes_of_rows over Session.row."""
import numpy as np


def jobs_of(ref_lengths, strands):
    """[(contig, strand char, length, first column)] in the order of a slot's row: contig-major, '+' before '-'"""
    out, at = [], 0
    for r, n in enumerate(ref_lengths):
        for s in range(strands):
            out.append((r, "+-"[s], int(n), at))
            at += int(n)
    return out


def coordinate(strand, col, ref_length, offset):
    """what a row reports for an alignment that ends in column `col`: pos_end on '+', pos_st on '-'"""
    return (col if strand == "+" else ref_length - col) + offset


def mask_of(targets, ref_lengths, offsets, strands):
    """bool [total columns]: every column against every interval"""
    jobs = jobs_of(ref_lengths, strands)
    mask = np.zeros(sum(j[2] for j in jobs), bool)
    for r, strand, n, at in jobs:
        x = np.array([coordinate(strand, c, n, int(offsets[r])) for c in range(n)])
        for contig, begin, end in targets:
            if contig == r:
                mask[at:at + n] |= (begin <= x) & (x < end)
    return mask


def mask_of_wide(targets, ref_lengths, offsets, strands):
    """mask_of for rows of 10^5 columns: a job's coordinates as one array (test_class_shapes_cpu.py compares the two)"""
    jobs = jobs_of(ref_lengths, strands)
    mask = np.zeros(sum(j[2] for j in jobs), bool)
    for r, strand, n, at in jobs:
        x = coordinate(strand, np.arange(n, dtype=np.int64), n, int(offsets[r]))
        for contig, begin, end in targets:
            if contig == r:
                mask[at:at + n] |= (begin <= x) & (x < end)
    return mask


def words_of(mask):
    bits = np.zeros((len(mask) + 31) // 32 * 32, np.uint8)
    bits[:len(mask)] = mask
    return [int(w) for w in np.packbits(bits.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").reshape(-1)]


def classes_of_rows(row, mask, ref_lengths, offsets, strands):
    """row: float32 [total columns], the slot's jobs back to back -> dict of the sfa_class_t fields but n_events / valid"""
    jobs = jobs_of(ref_lengths, strands)
    out = {}
    for name, sel in (("on", mask), ("off", ~mask)):
        cols = np.flatnonzero(sel)
        if len(cols) == 0:
            out.update({f"{name}_score": np.float32(np.inf), f"{name}_rid": -1, f"{name}_pos_end": -1, f"{name}_strand": 0, f"{name}_col": -1})
            continue
        g = int(cols[np.argmin(row[cols])])  # (argmin: the first of equal minima, and cols rise)
        r, strand, n, at = [j for j in jobs if j[3] <= g < j[3] + j[2]][0]
        out.update({f"{name}_score": row[g], f"{name}_rid": r, f"{name}_pos_end": coordinate(strand, g - at, n, int(offsets[r])), f"{name}_strand": ord(strand),
                    f"{name}_col": g})
    return out
