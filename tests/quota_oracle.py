"""Python restatement of the rules of open and closed groups (sigfish_amd/csrc/quota_rules.hpp) for the tests: row, labels and
bitmap in, record out.  The labels and the placing of a column are tests/group_oracle.py's.  test_session_quota_cpu.py compares
record_of_row with the C++ header's through tests/c/quota_rules.cpp; test_session_quota_gpu.py compares Session.open_classes
with it over Session.row."""
import numpy as np

from tests import group_oracle as G


def open_words(n_groups):
    return (n_groups + 31) // 32


def bitmap(n_groups, open_groups):
    """uint32[open_words]: the bits of `open_groups` set"""
    w = np.zeros(open_words(n_groups), np.uint32)
    for g in open_groups:
        assert 0 <= g < n_groups
        w[g // 32] |= np.uint32(1 << (g % 32))
    return w


def is_on(label, n_groups, open_bits):
    """bool per column: the label is a group (not n_groups) and its bit is set; None: every group is open"""
    label = np.asarray(label, np.int64)
    group = label < n_groups
    if open_bits is None:
        return group
    bits = np.asarray(open_bits, np.uint32)
    assert len(bits) == open_words(n_groups)
    safe = np.where(group, label, 0)
    return group & (((bits[safe // 32] >> (safe % 32).astype(np.uint32)) & 1) == 1)


def record_of_row(row, label, n_groups, open_bits, ref_lengths, offsets, strands):
    """row: float32 [total columns] -> dict of the sfa_open_class_t fields but n_events / valid.  A class's best column is the
    lexicographic minimum of (cost, column): np.argmin's first minimum over rising columns (a class of +inf columns: its first)."""
    assert not np.isnan(row).any() and not np.signbit(row).any()
    on = is_on(label, n_groups, open_bits)
    out = {}
    for side, cols in (("on", np.flatnonzero(on)), ("off", np.flatnonzero(~on))):
        if len(cols) == 0:
            out.update({f"{side}_score": np.float32(np.inf), f"{side}_rid": -1, f"{side}_pos_end": -1, f"{side}_strand": 0, f"{side}_group": -1, f"{side}_col": -1})
            continue
        c = int(cols[np.argmin(row[cols])])
        rid, pos, strand = G.place(c, ref_lengths, offsets, strands)
        out.update({f"{side}_score": row[c], f"{side}_rid": rid, f"{side}_pos_end": pos, f"{side}_strand": strand, f"{side}_group": int(label[c]), f"{side}_col": c})
    return out


class QuotaBook:
    """the quota book restated: note_accept -> the bitmap changed"""

    def __init__(self, n_groups, quota):
        self.n_groups, self.quota, self.count = n_groups, [quota] * n_groups, [0] * n_groups
        self.open = bitmap(n_groups, range(n_groups))

    def is_open(self, g):
        return 0 <= g < self.n_groups and bool((int(self.open[g // 32]) >> (g % 32)) & 1)

    def note_accept(self, g):
        if not 0 <= g < self.n_groups:
            return False
        self.count[g] += 1
        if self.quota[g] <= 0 or self.count[g] < self.quota[g] or not self.is_open(g):
            return False
        self.open[g // 32] &= np.uint32(~(1 << (g % 32)) & 0xffffffff)
        return True
