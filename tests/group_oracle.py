"""Python restatement of the target-group rules (sigfish_amd/csrc/group_rules.hpp) for the tests: the label of every column under
a list of group targets, the best column of every entry of a slot from its carried row (lexicographic minimum of (cost, column)),
the head and the decision.  test_session_groups_cpu.py compares the labels with the C++ header's and the decision with the
library's; test_session_groups_gpu.py compares Session.group_bests with entries_of_row over Session.row."""
import numpy as np

from tests import targets_oracle as T


def labels_of(targets, n_groups, ref_lengths, offsets, strands):
    """int [total columns]: every column against every interval (contig, begin, end, group); the lowest group that covers it, or
    n_groups"""
    jobs = T.jobs_of(ref_lengths, strands)
    label = np.full(sum(j[2] for j in jobs), n_groups, np.int64)
    for r, strand, n, at in jobs:
        x = T.coordinate(strand, np.arange(n, dtype=np.int64), n, int(offsets[r]))
        for contig, begin, end, group in targets:
            if contig == r:
                hit = (begin <= x) & (x < end)
                label[at:at + n][hit] = np.minimum(label[at:at + n][hit], group)
    return label


def place(col, ref_lengths, offsets, strands):
    """(rid, pos_end, strand code) of column `col` of a slot's row"""
    r, strand, n, at = [j for j in T.jobs_of(ref_lengths, strands) if j[3] <= col < j[3] + j[2]][0]
    return r, T.coordinate(strand, col - at, n, int(offsets[r])), ord(strand)


def entries_of_row(row, label, n_groups, ref_lengths, offsets, strands):
    """row: float32 [total columns] -> ([n_groups + 1] of (score, rid, pos_end, strand, column), head dict).  An entry without
    columns: (+inf, -1, -1, 0, -1).  The minimum is lexicographic in (cost, column): np.argmin's first minimum over rising columns."""
    assert not np.isnan(row).any() and not (np.signbit(row)).any()
    out = []
    for g in range(n_groups + 1):
        cols = np.flatnonzero(label == g)
        if len(cols) == 0:
            out.append((np.float32(np.inf), -1, -1, 0, -1))
            continue
        c = int(cols[np.argmin(row[cols])])
        out.append((row[c], *place(c, ref_lengths, offsets, strands), c))
    # the order of entries: (cost, column), entries without columns last and never named
    have = sorted((float(e[0]), e[4], g) for g, e in enumerate(out) if e[4] >= 0)
    head = dict(best=have[0][2] if have else -1, second=have[1][2] if len(have) > 1 else -1,
                best_score=out[have[0][2]][0] if have else np.float32(np.inf), second_score=out[have[1][2]][0] if len(have) > 1 else np.float32(np.inf))
    return out, head


def decide(head, min_events, margin):
    """group_decide: the best entry's index or None"""
    if not head["valid"] or head["best"] < 0 or head["n_events"] < min_events or not (margin >= 0) or not np.isfinite(margin):
        return None
    second = np.float32(np.inf) if head["second"] < 0 else np.float32(head["second_score"])
    with np.errstate(all="ignore"):
        ok = np.float32(second - np.float32(head["best_score"])) >= np.float32(np.float32(margin) * np.float32(head["n_events"]))
    return int(head["best"]) if ok else None
