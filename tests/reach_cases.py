"""The reference and the target lists the reach tests share (test_reach_model_cpu.py holds the header against the numpy model on
them, test_session_reach_gpu.py the device), chosen for the build kernel's edges: contigs of 31, 33, 95, 257 and 300 k-mers with
non-zero offsets, so that jobs start and end inside a mask word, inside a wave (64 columns) and inside a block (256 columns), and
the first block holds several jobs.  DNA: 1432 columns in 10 jobs, 6 blocks; RNA: 716 columns in 5 jobs, 3 blocks.

LEAD_ONLY[name] = (dna, rna): columns admitted through a lead-in alone (inside no admitting target's body), worked out by hand
from the rule -- a '+' job of contig c reports off .. off + rl - 1, a '-' job off + 1 .. off + rl -- so that the model itself is
held against something.  None: not worked out (the random list)."""
import functools

import numpy as np

from tests import reach_model as M

LENS = [31, 33, 95, 257, 300]
OFFS = [5, 12, 100, 7, 1000]


def _thousand():
    rng = np.random.default_rng(1000)
    out = []
    for _ in range(1000):
        c = int(rng.integers(0, 5))
        limit = OFFS[c] + LENS[c] + 1
        b = int(rng.integers(0, limit))
        e = min(limit, b + 1 + int(rng.integers(0, 4)))
        out.append((c, b, e, int(rng.choice([0, 0, 1, 2, 5, 9])), [None, "+", "-"][int(rng.integers(0, 3))]))
    return out


CASES = {
    # a contig's first and last coordinate (end = off + rl + 1), on contigs of 300 and of 31 columns
    "first and last coordinate": [(4, 1000, 1001, 10, None), (4, 1300, 1301, 10, None), (0, 5, 6, 3, "+"), (0, 36, 37, 3, "-")],
    "a lead longer than the contig": [(3, 100, 110, 5000, None)],
    "a lead that reaches below the offset": [(2, 110, 120, 50, "+"), (4, 1005, 1010, 2000, "+")],
    "plus only": [(3, 50, 80, 30, "+"), (4, 1100, 1150, 64, "+")],
    "minus only": [(3, 50, 80, 30, "-"), (4, 1100, 1150, 64, "-")],  # (on RNA: an empty result)
    "both strands": [(3, 50, 80, 30, None), (4, 1100, 1150, 64, None)],
    "overlapping lead-ins": [(4, 1100, 1110, 80, None), (4, 1130, 1140, 90, None)],  # the anchor takes the nearer body
    "a lead-in over another target's body": [(3, 100, 150, 0, None), (3, 160, 170, 40, "+"), (3, 80, 90, 40, "-")],
    "touching": [(2, 120, 130, 6, None), (2, 130, 140, 6, None), (2, 140, 141, 0, None)],
    "bodies below the offset": [(2, 0, 50, 120, None), (2, 90, 100, 30, "-")],  # '-' anchors no row reports: entry -2
    "one": [(1, 20, 25, 4, None)],
    "a thousand": _thousand(),
}
LEAD_ONLY = {
    "first and last coordinate": (20, 10), "a lead longer than the contig": (248, 93), "a lead that reaches below the offset": (15, 15), "plus only": (94, 94),
    "minus only": (94, 0), "both strands": (188, 94), "overlapping lead-ins": (210, 100), "a lead-in over another target's body": (20, 10), "touching": (11, 6),
    "bodies below the offset": (69, 0), "one": (8, 4), "a thousand": None,
}


@functools.lru_cache(maxsize=None)
def model_tables(name, strands):
    """(mask, anchor coordinates, lead-only, entries) of a case under the numpy model; computed once, never written to"""
    md = M.Reach(LENS, OFFS, strands)
    mask, anchor, lead_only = md.tables(CASES[name])
    mask2, entry = md.entries(CASES[name])
    assert np.array_equal(mask, mask2)
    for a in (mask, anchor, lead_only, entry):
        a.setflags(write=False)
    return mask, anchor, lead_only, entry
