"""An independent numpy model of a session's reach targets (sigfish_amd/csrc/reach_rules.hpp), for the tests: which columns a
list of stranded targets with a lead-in admits, the anchor of every column, and the live mask under a depth cap, which reads the
depth of the ANCHOR.  Nothing here is taken from the header: place_col is restated from its definition (`j + off` on '+',
`rl - j + off` on '-'), the rule from the issue's two inequalities, column by column over every target, in Python integers (no
overflow to think about).  test_reach_model_cpu.py compares the header with the model; test_session_reach_gpu.py the device.

A target is (contig, begin, end, lead, strand) with strand '+', '-' or None (both)."""
import numpy as np

NONE, BELOW_TRACK = -1, -2  # entries: off target; an anchor below the contig's offset, which has no depth


def place_col(strand, j, rl, off):
    """the coordinate a row reports for an alignment that ends in column j of a strand's array"""
    return j + off if strand == "+" else rl - j + off


class Reach:
    """ref_lengths / offsets per contig, strands 1 (RNA: '+' only) or 2 (DNA: '+' then '-' of every contig)"""

    def __init__(self, ref_lengths, offsets, strands):
        self.rl, self.off, self.strands = [int(x) for x in ref_lengths], [int(x) for x in offsets], int(strands)
        self.depth = [np.zeros(n + 1, np.int64) for n in self.rl]  # entry x - off stands for coordinate x; both strands share it
        self.jobs, at = [], 0  # (contig, strand, first column)
        for c, n in enumerate(self.rl):
            for s in "+-"[:self.strands]:
                self.jobs.append((c, s, at))
                at += n
        self.total = at

    def columns(self):
        """(global column, contig, strand, coordinate) of every column of a slot's row"""
        for c, s, at in self.jobs:
            for j in range(self.rl[c]):
                yield at + j, c, s, place_col(s, j, self.rl[c], self.off[c])

    @staticmethod
    def admitting(targets, c, s, x):
        """the targets that admit coordinate x of a (contig c, strand s) job"""
        out = []
        for t in targets:
            tc, b, e, lead, ts = t
            if tc != c or (ts is not None and ts != s):
                continue
            if (s == "+" and b - lead <= x < e) or (s == "-" and b <= x < e + lead):
                out.append(t)
        return out

    def tables(self, targets):
        """(bool [total]: on target, int64 [total]: the anchor's COORDINATE or -1, bool [total]: admitted through a lead only)"""
        mask, anchor, lead_only = np.zeros(self.total, bool), np.full(self.total, -1, np.int64), np.zeros(self.total, bool)
        for g, c, s, x in self.columns():
            adm = self.admitting(targets, c, s, x)
            if not adm:
                continue
            mask[g] = True
            anchor[g] = min(max(x, t[1]) for t in adm) if s == "+" else max(min(x, t[2] - 1) for t in adm)
            lead_only[g] = not any(t[1] <= x < t[2] for t in adm)
        return mask, anchor, lead_only

    def entries(self, targets):
        """(mask, int64 [total]): the anchor as an index into its contig's depth track, NONE, or BELOW_TRACK"""
        mask, anchor, _ = self.tables(targets)
        entry = np.full(self.total, NONE, np.int64)
        for g, c, s, x in self.columns():
            if mask[g]:
                entry[g] = anchor[g] - self.off[c] if anchor[g] >= self.off[c] else BELOW_TRACK
        return mask, entry

    def add(self, intervals):
        """depth += 1 over every [begin, end) of coordinates; what lies outside the contig's coordinates counts nowhere"""
        for c, b, e in intervals:
            lo, hi = max(int(b) - self.off[c], 0), min(int(e) - self.off[c], self.rl[c] + 1)
            if lo < hi:
                self.depth[c][lo:hi] += 1

    def live_mask(self, targets, cap):
        """bool [total]: on target, and the depth of the anchor below the cap (an anchor below the track has depth 0)"""
        mask, entry = self.entries(targets)
        live = np.zeros(self.total, bool)
        for g, c, s, x in self.columns():
            if mask[g]:
                live[g] = True if entry[g] == BELOW_TRACK else self.depth[c][entry[g]] < cap
        return live


def words_of(mask):
    """the mask as 32-bit words, bit j % 32 of word j // 32"""
    bits = np.zeros((len(mask) + 31) // 32 * 32, np.uint64)
    bits[:len(mask)] = mask
    return [int((bits[w * 32:w * 32 + 32] << np.arange(32, dtype=np.uint64)).sum()) for w in range(len(bits) // 32)]
