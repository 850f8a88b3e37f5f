"""An independent numpy model of a session's group cap (sigfish_amd/csrc/group_cover_rules.hpp), for the tests: the depth tracks,
the base label of every column (the lowest group id whose interval holds the column's coordinate, else the background n_groups),
the live label (the base label while the coordinate's depth lies below the cap, else the background), the lowest column of every
live label, the depth record of every entry over the forward-strand columns, and the live columns turned back into group targets.
Nothing here is taken from the headers or from tests/coverage_model.py: the column-to-coordinate mapping is restated from its
definition (`j + off` on '+', `rl - j + off` on '-').  test_session_group_cover_cpu.py compares the model with the header's host
functions; test_session_group_cover_gpu.py compares the device with the model."""
import numpy as np

NO_COLUMN = 2 ** 31 - 1
COVER_DTYPE = np.dtype([("columns", "<i8"), ("capped", "<i8"), ("depth_sum", "<u8"), ("depth_min", "<u4"), ("depth_max", "<u4")])


def coordinate(strand, j, rl, off):
    """the coordinate a row reports for an alignment that ends in column j of a strand's array"""
    return j + off if strand == "+" else rl - j + off


class GroupCover:
    """ref_lengths / offsets per contig, strands 1 (RNA: '+' only) or 2 (DNA: '+' then '-' of every contig); targets are
    (contig, begin, end, group) with 0 <= group < n_groups"""

    def __init__(self, ref_lengths, offsets, strands, n_groups, targets, cap):
        self.rl, self.off, self.strands = [int(x) for x in ref_lengths], [int(x) for x in offsets], int(strands)
        self.n_groups, self.cap = int(n_groups), int(cap)
        self.depth = [np.zeros(n + 1, np.int64) for n in self.rl]  # entry x - off stands for coordinate x; both strands share it
        self.jobs, at = [], 0  # (contig, strand, first column)
        for c, n in enumerate(self.rl):
            for s in "+-"[:self.strands]:
                self.jobs.append((c, s, at))
                at += n
        self.total = at
        self.set_targets(targets)

    def set_targets(self, targets):
        """the label of every COORDINATE entry of every contig, then of every column"""
        by_coord = [np.full(n + 1, self.n_groups, np.int64) for n in self.rl]
        for c, b, e, g in targets:
            lo, hi = max(int(b) - self.off[c], 0), min(int(e) - self.off[c], self.rl[c] + 1)
            if lo < hi:
                by_coord[c][lo:hi] = np.minimum(by_coord[c][lo:hi], int(g))
        self.by_coord = by_coord

    def entries(self, c, s):
        """the track entry of every column of job (c, s)"""
        j = np.arange(self.rl[c])
        return (j if s == "+" else self.rl[c] - j)  # coordinate(s, j, rl, off) - off

    def add(self, intervals):
        for c, b, e in intervals:
            lo, hi = max(int(b) - self.off[c], 0), min(int(e) - self.off[c], self.rl[c] + 1)
            if lo < hi:
                self.depth[c][lo:hi] += 1

    def base_labels(self):
        out = np.empty(self.total, np.int64)
        for c, s, at in self.jobs:
            out[at:at + self.rl[c]] = self.by_coord[c][self.entries(c, s)]
        return out

    def live_labels(self, cap=None):
        cap = self.cap if cap is None else cap
        out = np.empty(self.total, np.int64)
        for c, s, at in self.jobs:
            e = self.entries(c, s)
            out[at:at + self.rl[c]] = np.where(self.depth[c][e] < cap, self.by_coord[c][e], self.n_groups)
        return out

    def firsts(self):
        """the lowest column of every live label, NO_COLUMN for none"""
        live = self.live_labels()
        out = np.full(self.n_groups + 1, NO_COLUMN, np.int64)
        cols = np.arange(self.total)
        np.minimum.at(out, live, cols)
        return out

    def records(self):
        """per entry 0 .. n_groups over the columns of the '+' jobs whose BASE label is the entry"""
        rec = np.zeros(self.n_groups + 1, COVER_DTYPE)
        rec["depth_min"] = 2 ** 32 - 1
        for c, s, at in self.jobs:
            if s != "+":
                continue
            e = self.entries(c, s)
            lab, d = self.by_coord[c][e], self.depth[c][e]
            for g in np.unique(lab):
                dg = d[lab == g]
                r = rec[g]
                r["columns"] += len(dg)
                r["capped"] += int((dg >= self.cap).sum())
                r["depth_sum"] += int(dg.sum())
                r["depth_min"] = min(int(r["depth_min"]), int(dg.min()))
                r["depth_max"] = max(int(r["depth_max"]), int(dg.max()))
        return rec

    def open_pieces(self):
        """(contig, begin, end, group) runs of coordinates whose live label is `group`: given to a fresh session as group targets
        they make its BASE table this model's LIVE table -- the live label is a function of the coordinate, on both strands.  Only
        coordinates some column reports are listed (entry 0 has no '-' column and entry rl no '+' column; with one strand entry rl
        has none at all)."""
        out = []
        for c in range(len(self.rl)):
            hi = self.rl[c] + (1 if self.strands == 2 else 0)
            live = np.where(self.depth[c] < self.cap, self.by_coord[c], self.n_groups)[:hi]
            if hi == 0:
                continue
            starts = np.concatenate([[0], np.flatnonzero(live[1:] != live[:-1]) + 1])  # where a run of equal labels begins
            ends = np.concatenate([starts[1:], [hi]])
            for a, b in zip(starts.tolist(), ends.tolist()):
                if live[a] != self.n_groups:
                    out.append((c, a + self.off[c], b + self.off[c], int(live[a])))
        return out
