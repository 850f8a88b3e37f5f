"""An independent numpy model of a session's coverage cap (sigfish_amd/csrc/coverage_rules.hpp), for the tests: the depth tracks,
the live mask per column and its count, and the live columns turned back into coordinate intervals.  Nothing here is taken from
the header or from tests/targets_oracle.py: place_col is restated from its definition (`j + off` on '+', `rl - j + off` on '-').
test_session_coverage_cpu.py compares the model with the header's coverage_live_mask; test_session_coverage_gpu.py compares the
device with the model."""
import numpy as np


def place_col(strand, j, rl, off):
    """the coordinate a row reports for an alignment that ends in column j of a strand's array"""
    return j + off if strand == "+" else rl - j + off


class Coverage:
    """ref_lengths / offsets per contig, strands 1 (RNA: '+' only) or 2 (DNA: '+' then '-' of every contig)"""

    def __init__(self, ref_lengths, offsets, strands, cap):
        self.rl, self.off, self.strands, self.cap = [int(x) for x in ref_lengths], [int(x) for x in offsets], int(strands), int(cap)
        self.depth = [np.zeros(n + 1, np.int64) for n in self.rl]  # entry x - off stands for coordinate x; both strands share it
        self.jobs, at = [], 0  # (contig, strand, first column)
        for c, n in enumerate(self.rl):
            for s in "+-"[:self.strands]:
                self.jobs.append((c, s, at))
                at += n
        self.total = at

    def add(self, intervals):
        """depth += 1 over every [begin, end) of coordinates; what lies outside the contig's coordinates counts nowhere"""
        for c, b, e in intervals:
            lo, hi = max(int(b) - self.off[c], 0), min(int(e) - self.off[c], self.rl[c] + 1)
            if lo < hi:
                self.depth[c][lo:hi] += 1

    def base_mask(self, targets):
        """bool [total columns]: the column's coordinate lies in a target of its contig"""
        m = np.zeros(self.total, bool)
        for c, s, at in self.jobs:
            for j in range(self.rl[c]):
                x = place_col(s, j, self.rl[c], self.off[c])
                m[at + j] = any(t[0] == c and t[1] <= x < t[2] for t in targets)
        return m

    def live_mask(self, targets):
        """bool [total columns]: on target and depth below the cap"""
        m = self.base_mask(targets)
        for c, s, at in self.jobs:
            for j in range(self.rl[c]):
                m[at + j] = m[at + j] and self.depth[c][place_col(s, j, self.rl[c], self.off[c]) - self.off[c]] < self.cap
        return m

    def open_columns(self, targets):
        return int(self.live_mask(targets).sum())

    def open_pieces(self, targets):
        """{strand class: [(contig, begin, end)]}: the live columns of the '+' jobs and of the '-' jobs as maximal runs of
        coordinates.  The rule closes a coordinate on both strands at once, so wherever both strands have a column for a coordinate
        the two lists agree; a coordinate only one strand reports (off on '-' has no column, off + rl on '+' has none) appears in
        that strand's list alone."""
        live = self.live_mask(targets)
        out = {}
        for c, s, at in self.jobs:
            xs = sorted(place_col(s, j, self.rl[c], self.off[c]) for j in range(self.rl[c]) if live[at + j])
            runs = out.setdefault(s, [])
            for x in xs:
                if runs and runs[-1][0] == c and runs[-1][2] == x:
                    runs[-1][2] = x + 1
                else:
                    runs.append([c, x, x + 1])
        return {s: [tuple(r) for r in runs] for s, runs in out.items()}

    def open_list(self, targets):
        """one target list for Session.set_targets that gives the live mask: the union of the strand classes' pieces"""
        pieces = self.open_pieces(targets)
        return sorted(set(p for runs in pieces.values() for p in runs))


def words_of(mask):
    """the mask as 32-bit words, bit j % 32 of word j // 32"""
    bits = np.zeros((len(mask) + 31) // 32 * 32, np.uint64)
    bits[:len(mask)] = mask
    return [int((bits[w * 32:w * 32 + 32] << np.arange(32, dtype=np.uint64)).sum()) for w in range(len(bits) // 32)]
