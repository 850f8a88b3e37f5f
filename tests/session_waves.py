"""Which waves a session call runs (helpers of test_session_waves_cpu.py / test_session_waves_gpu.py; no test, no fixture).

plan_call() restates the grouping rule of the session sweep in Python -- class_for (sfa_plan.hpp), the launch split at 2048
events (plan_session_call) and the sort key and wave filling of plan_launch (both in sigfish_amd/csrc/session_plan.hpp, the pure
header sfa_session.hip plans with; test_session_plan_cpu.py compares that C++ with plan_call) -- so that a test can say which
(class shape, first chunk or carried row, occupancy, g0) combinations a schedule reaches, and what the planner's task and
launch counts must be.  build_matrix() is a schedule of ONE call that reaches all of them; test_session_waves_cpu.py asserts
that it does, and that the hand-written SCHED of test_session_gpu.py does not.

How build_matrix reads its specification where the grouping rule leaves no choice: pieces of one kind, class and residue
(length modulo R) are sorted by length and cut into waves, so two waves of one residue cannot be chosen independently.  The
two-slot wave "longest with the shortest of the same residue" is 128 & 72, 256 & 144, 512 & 288, 1024 & 544 (residue 0) as
listed; for those shapes the full wave therefore starts one residue lower, at hi - 1 (hi - 1, hi - 1 - R, ...: g0 = 0 .. 64 /
lanes - 1 as intended, rq = R - 2).  For (4, 16) the pair is 61 & 1 (residue 1) and the full wave is 64, 60, 56, 52.  The
class's shortest length lo + 1 has residue 1 in every class: alone in its wave for the other shapes (so the three-slot wave
takes residue 3), the short end of the pair for (4, 16).
"""
from collections import namedtuple

import numpy as np

SHAPES = [(32, 64), (32, 32), (32, 16), (16, 16), (8, 16), (4, 16)]  # kClassShapes: (R, lanes), long first
MAX_PIECE = 2048  # kMaxQuery: events of one slot inside one launch


def class_for(n):
    """Index into SHAPES for a piece of n events (1 .. MAX_PIECE)."""
    assert 1 <= n <= MAX_PIECE
    c = 0
    while c + 1 < 6 and n <= SHAPES[c + 1][0] * SHAPES[c + 1][1]:
        c += 1
    return c


def class_bounds(ci):
    """(lo, hi): the class holds pieces of lo < n <= hi events."""
    hi = SHAPES[ci][0] * SHAPES[ci][1]
    lo = SHAPES[ci + 1][0] * SHAPES[ci + 1][1] if ci + 1 < 6 else 0
    return lo, hi


Piece = namedtuple("Piece", "call slot len total first")


class Group:
    """One wave's worth of pieces: what a (group, job) task of the sweep works on."""

    def __init__(self, ci, first, pieces):
        self.R, self.lanes = SHAPES[ci]
        self.first, self.pieces = first, pieces
        self.qlen = pieces[0].len  # (descending inside the run: the first is the longest)
        self.lq, self.rq = (self.qlen - 1) // self.R, (self.qlen - 1) % self.R
        self.g0 = [(self.qlen - p.len) // self.R for p in pieces]
        self.occupancy, self.capacity = len(pieces), 64 // self.lanes

    @property
    def shape(self):
        return (self.R, self.lanes)

    def describe(self, slot):
        i = [p.slot for p in self.pieces].index(slot)
        return (f"shape {self.shape}, {'first' if self.first else 'carried'}, wave of {self.occupancy}/{self.capacity} "
                f"(lengths {[p.len for p in self.pieces]}), g0 {self.g0[i]}, lq {self.lq}, rq {self.rq}")


def plan_launch(pieces):
    """-> [Group] in task order (plan_launch of session_plan.hpp)."""
    def key(p):
        ci = class_for(p.len)
        return (-p.first, ci, p.len % SHAPES[ci][0], -p.len, p.call)
    ps = sorted(pieces, key=key)
    groups, i = [], 0
    while i < len(ps):
        p = ps[i]
        ci = class_for(p.len)
        R, lanes = SHAPES[ci]
        g = []
        while len(g) < 64 // lanes and i < len(ps) and ps[i].first == p.first and class_for(ps[i].len) == ci and ps[i].len % R == p.len % R:
            g.append(ps[i])
            i += 1
        groups.append(Group(ci, p.first, g))
    return groups


def plan_call(chunks, held):
    """chunks: [(slot, events)] of one extend call, held: {slot: events the slot holds before it}.  -> [[Group]]: one list per
    launch; launch p holds events [p * 2048, (p + 1) * 2048) of every chunk that is that long."""
    launches, p = [], 0
    while True:
        pieces = []
        for i, (slot, n) in enumerate(chunks):
            done = p * MAX_PIECE
            if n <= done:
                continue
            k = min(MAX_PIECE, n - done)
            have = held.get(slot, 0) + done
            pieces.append(Piece(i, slot, k, have + k, 1 if have == 0 else 0))
        if not pieces:
            return launches
        launches.append(plan_launch(pieces))
        p += 1


def counts(launches, n_jobs):
    """(n_tasks, fill_launches) the planner must report for the call."""
    return sum(len(gs) for gs in launches) * n_jobs, len(launches)


def classes_per_launch(launches):
    return [len({(g.shape, g.first) for g in gs}) for gs in launches]


def coverage(launches):
    """{(shape, first): {"groups", "full", "partial", "max_g0_full", "g0_eq_lq", "max_occupancy"}} over all launches."""
    cov = {}
    for gs in launches:
        for g in gs:
            c = cov.setdefault((g.shape, g.first), dict(groups=0, full=0, partial=0, max_g0_full=-1, g0_eq_lq=0, max_occupancy=0))
            c["groups"] += 1
            c["max_occupancy"] = max(c["max_occupancy"], g.occupancy)
            if g.occupancy == g.capacity:
                c["full"] += 1
                c["max_g0_full"] = max(c["max_g0_full"], max(g.g0))
            else:
                c["partial"] += 1
            if g.lq > 0 and max(g.g0) == g.lq:  # the shortest chunk starts in the owner's lane
                c["g0_eq_lq"] += 1
    return cov


def shortfalls(cov, kinds=(1, 0)):
    """The conditions of the coverage table that `cov` does not reach, as [(shape, first, what)]."""
    miss = []
    for first in kinds:
        for shape in SHAPES:
            c = cov.get((shape, first))
            cap = 64 // shape[1]
            if c is None:
                miss.append((shape, first, "never run"))
                continue
            if c["groups"] < 2:
                miss.append((shape, first, "fewer than 2 groups"))
            if cap > 1:
                if c["full"] == 0:
                    miss.append((shape, first, "no full wave"))
                elif c["max_g0_full"] < cap - 1:
                    miss.append((shape, first, "no full wave with g0 >= 64 / lanes - 1"))
                if c["partial"] == 0:
                    miss.append((shape, first, "no partly filled wave"))
        if not any(c["g0_eq_lq"] for (sh, f), c in cov.items() if f == first):
            miss.append((None, first, "no wave with g0 == lq"))
    return miss


# ---- the matrix ----
PAIRS = {(4, 16): (61, 1), (8, 16): (128, 72), (16, 16): (256, 144), (32, 16): (512, 288), (32, 32): (1024, 544)}
N_SLOTS = 128
ZERO_SLOT, UNNAMED_SLOT = 101, 7  # hold a row before the matrix call; named with a zero-length chunk / not named in it
IDLE_EVENTS = {ZERO_SLOT: 50, UNNAMED_SLOT: 90}


def matrix_lengths():
    """[[lengths of one intended wave]] of the matrix call, longest class first."""
    waves = [[2048], [1025], [2047]]  # (32, 64): one slot per wave
    for ci in range(1, 6):
        R, lanes = SHAPES[ci]
        ns = 64 // lanes
        lo, hi = class_bounds(ci)
        pair = PAIRS[(R, lanes)]
        top = hi - 1 if pair[0] % R == hi % R else hi  # (the pair's residue is taken: see the module docstring)
        waves.append([top - k * R for k in range(ns)])                            # a full wave, g0 = 0 .. ns - 1
        waves.append(list(pair))                                                  # longest & shortest of a residue
        res3 = [n for n in range(hi, lo, -1) if n % R == 3]
        waves.append([res3[0], res3[len(res3) // 2], res3[-1]][:max(ns - 1, 1)])  # partly filled, another residue
        if lo + 1 not in pair:
            waves.append([lo + 1])                                                # the class's shortest length, alone
    waves.append([2])  # one more group: n_tasks of the 18-job DNA reference is then no multiple of 4 (a block's last waves idle)
    return waves


def _prefix(i):
    return [3, 40, 77, 130][i] if i < 4 else 130 + 21 * (i - 3)


Matrix = namedtuple("Matrix", "slots lens prefix")  # per matrix slot, in matrix order: slot id, chunk length, earlier events


def build_matrix(kind):
    """The schedule of ONE call: Matrix(slots, lens, prefix).  kind "first": the slots are empty before it (prefix 0); "carried":
    slot i has had an earlier call with prefix[i] events, all different."""
    assert kind in ("first", "carried")
    lens = [n for w in matrix_lengths() for n in w]
    ids = [int(s) for s in np.random.default_rng(2024).permutation(N_SLOTS) if s not in (ZERO_SLOT, UNNAMED_SLOT)][:len(lens)]
    # prefixes by rank of the chunk length, the four shortest in order (totals from 4 events on), the others scattered
    rank = {i: r for r, i in enumerate(sorted(range(len(lens)), key=lambda i: (lens[i], i)))}
    scatter = [rank[i] if rank[i] < 4 else 4 + ((rank[i] - 4) * 19) % (len(lens) - 4) for i in range(len(lens))]
    prefix = [_prefix(scatter[i]) if kind == "carried" else 0 for i in range(len(lens))]
    return Matrix(ids, lens, prefix)


SPLIT = [(41, 2049), (3, 4097), (90, 64), (17, 300)]  # (slot, events) of one call: pieces that span two and three launches

# continuation: one more chunk per slot, of another class than the slot's matrix chunk (the first entry from position i on,
# cyclically, whose class differs)
CONT_LENS = [200, 5, 70, 600, 33, 1100, 129, 300, 64, 520, 17, 90, 257, 1, 1030, 128]


def continuation_lengths(m):
    out = []
    for i, n in enumerate(m.lens):
        k = i
        while class_for(CONT_LENS[k % len(CONT_LENS)]) == class_for(n):
            k += 1
        out.append(CONT_LENS[k % len(CONT_LENS)])
    return out
