"""An independent numpy model of a session's reach groups (sigfish_amd/csrc/reach_group_rules.hpp), for the tests.  Nothing here is
taken from the header: place_col is restated from its definition (`j + off` on '+', `rl - j + off` on '-'), admission from the two
inequalities, column by column over every target, in Python integers.  test_reach_group_rules_cpu.py checks it on hand-made
columns; test_session_group_reach_gpu.py and test_realtime_group_reach_gpu.py compare the device with it.

A target is (contig, begin, end, lead, group, strand) with strand '+', '-' or None / 0 / '.' (both), or a record of
REACH_GROUP_TARGET_DTYPE."""
import numpy as np

NONE, BELOW_TRACK = -1, -2


def _norm(t):
    c, b, e, lead, g, s = (t[f] for f in ("contig", "begin", "end", "lead", "group", "strand")) if isinstance(t, np.void) else t
    s = None if s in (None, 0, ".", "") else (chr(int(s)) if not isinstance(s, str) else s)
    return int(c), int(b), int(e), int(lead), int(g), s


def columns(lens, offs, strands):
    """(global column, contig, strand, coordinate) of every column of a slot's row"""
    at = 0
    for c, n in enumerate(lens):
        for s in "+-"[:strands]:
            for j in range(n):
                yield at + j, c, s, (j + offs[c] if s == "+" else n - j + offs[c])
            at += n


def label_of(targets, n_groups, c, s, x):
    """(label, anchor coordinate or None) of coordinate x of a (contig c, strand s) job"""
    own = []  # (the target's own anchor, its group) of every admitting target
    for tc, b, e, lead, g, ts in targets:
        if tc != c or (ts is not None and ts != s):
            continue
        if s == "+" and b - lead <= x < e:
            own.append((max(x, b), g))
        if s == "-" and b <= x < e + lead:
            own.append((min(x, e - 1), g))
    if not own:
        return n_groups, None
    anchor = min(a for a, _ in own) if s == "+" else max(a for a, _ in own)
    return min(g for a, g in own if a == anchor), anchor


def tables(targets, n_groups, lens, offs, strands):
    """(uint16 [total]: the label, int32 [total]: the anchor as an index into its contig's depth track, NONE, BELOW_TRACK)"""
    targets = [_norm(t) for t in targets]
    total = strands * int(sum(lens))
    label, entry = np.full(total, n_groups, np.uint16), np.full(total, NONE, np.int32)
    by_contig = {}
    for t in targets:
        by_contig.setdefault(t[0], []).append(t)
    for g, c, s, x in columns(lens, offs, strands):
        if c not in by_contig:
            continue
        l, a = label_of(by_contig[c], n_groups, c, s, x)
        if a is not None:
            label[g], entry[g] = l, (a - offs[c] if a >= offs[c] else BELOW_TRACK)
    return label, entry


def live_labels(label, entry, depth, cap, n_groups, lens, strands):
    """the live table: the base label while the depth of the ANCHOR's entry lies below the cap (BELOW_TRACK: depth 0).  depth: one
    array of ref_length + 1 entries per contig"""
    live = label.copy()
    at = 0
    for c, n in enumerate(lens):
        for _ in range(strands):
            for j in range(at, at + n):
                if label[j] != n_groups and entry[j] >= 0 and depth[c][entry[j]] >= cap:
                    live[j] = n_groups
            at += n
    return live


def records(label, entry, depth, cap, n_groups, lens, offs, strands):
    """(columns, capped, depth_sum, depth_min, depth_max) per entry 0 .. n_groups over the BODY columns of the '+' jobs: those
    whose anchor entry is their own track entry"""
    rec = [[0, 0, 0, 0xffffffff, 0] for _ in range(n_groups + 1)]
    for g, c, s, x in columns(lens, offs, strands):
        if s != "+" or entry[g] != x - offs[c]:
            continue
        d, r = int(depth[c][entry[g]]), rec[int(label[g])]
        r[0] += 1
        r[1] += d >= cap
        r[2] += d
        r[3], r[4] = min(r[3], d), max(r[4], d)
    return [tuple(r) for r in rec]


def firsts(label, n_groups):
    """the lowest column of every label, -1: none"""
    out = np.full(n_groups + 1, -1, np.int64)
    for l in range(n_groups + 1):
        at = np.flatnonzero(label == l)
        if len(at):
            out[l] = at[0]
    return out
