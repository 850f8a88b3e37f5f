"""What the three query calls of a session refuse, and what a refused call leaves (sfa_session_classes, sfa_session_group_bests
with and without `bests`, sfa_session_open_classes: one prologue, query_run of sfa_session_targets.hip).  Every refusal -- a slot
out of range, a slot named twice, the feature not configured, for open_classes a bitmap of the wrong size -- returns SFA_EINVAL
with its message and comes before the first write to the caller's records: the output arrays are filled with a byte pattern in
front of the call and compared byte for byte behind it.  Then one good call over a poisoned, an extended and an empty slot, in
that order: "none" records for the first and the last, a finite record for the one in the middle, and a profile that is the
call's device time and nothing else.  Reference: two contigs of 40 and 70 k-mers, DNA; a 4-slot session; the calls go through
ctypes, since the Python wrappers allocate the records themselves."""
import ctypes as C

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib
from sigfish_amd.api import CLASS_DTYPE, GROUP_BEST_DTYPE, GROUP_HEAD_DTYPE, OPEN_CLASS_DTYPE
from tests.test_session_gpu import _events, _small_ref

pytestmark = pytest.mark.gpu

LENS = [40, 70]
N_SLOTS, N_GROUPS = 4, 2
EXTENDED, EMPTY, POISONED = 0, 1, 2
PATTERN = 0xA5
EINVAL = -1


class Call:
    """one of the calls: its output arrays for n entries, pre-filled with the pattern, and the call itself"""

    def __init__(self, kind, se, n, n_words=None):
        self.kind, self.se, self.n = kind, se, n
        self.n_words = n_words
        shapes = {"classes": [(n, CLASS_DTYPE)], "group_bests": [((n, N_GROUPS + 1), GROUP_BEST_DTYPE), (n, GROUP_HEAD_DTYPE)],
                  "group_bests_heads_only": [(n, GROUP_HEAD_DTYPE)], "open_classes": [(n, OPEN_CLASS_DTYPE)]}[kind]
        self.out = [np.frombuffer(bytearray([PATTERN]) * (int(np.prod(shape)) * dt.itemsize), dt).reshape(shape) for shape, dt in shapes]
        self.before = [o.tobytes() for o in self.out]

    def run(self, slots):
        L, h = self.se._L, self.se._h
        sl = np.ascontiguousarray(slots, np.int32)
        ptr = [o.ctypes.data_as(C.c_void_p) for o in self.out]
        if self.kind == "classes":
            return L.sfa_session_classes(h, sl.ctypes.data_as(_lib.i32p), len(sl), ptr[0])
        if self.kind == "group_bests":
            return L.sfa_session_group_bests(h, sl.ctypes.data_as(_lib.i32p), len(sl), ptr[0], ptr[1])
        if self.kind == "group_bests_heads_only":
            return L.sfa_session_group_bests(h, sl.ctypes.data_as(_lib.i32p), len(sl), None, ptr[0])
        bits = None if self.n_words is None else np.full(self.n_words, 0xFFFFFFFF, np.uint32)
        return L.sfa_session_open_classes(h, sl.ctypes.data_as(_lib.i32p), len(sl), None if bits is None else bits.ctypes.data_as(C.POINTER(C.c_uint32)),
                                          0 if bits is None else len(bits), ptr[0])

    def untouched(self):
        return [o.tobytes() for o in self.out] == self.before


def refused(kind, se, slots, text, n_words=None):
    call = Call(kind, se, len(slots), n_words)
    rc = call.run(slots)
    msg = se._L.sfa_last_error().decode()
    assert rc == EINVAL and msg == text, (kind, slots, rc, msg)
    assert call.untouched(), (kind, slots, "a refused call wrote to the caller's records")


@pytest.mark.parametrize("kind", ["classes", "group_bests", "group_bests_heads_only", "open_classes"])
def test_refusals_leave_the_records_and_a_good_call_fills_them(kind):
    rng = np.random.default_rng(11)
    ref = _small_ref(rng, LENS, False)
    off = [int(x) for x in ref.st_offset]
    who = "sfa_session_group_bests" if kind.startswith("group_bests") else "sfa_session_" + kind
    grouped = kind != "classes"
    feature = "the session has no groups (sfa_session_target_groups)" if grouped else "the session has no targets (sfa_session_targets)"
    with S.Aligner(ref, 0) as al, al.session(N_SLOTS) as se:
        refused(kind, se, [EXTENDED], f"{who}: {feature}")  # the feature is not configured
        if grouped:
            se.set_target_groups([(0, off[0] + 3, off[0] + 20, 0), (1, off[1] + 10, off[1] + 60, 1)], N_GROUPS)
        else:
            se.set_targets([(1, off[1] + 10, off[1] + 60)])
        se.extend([EXTENDED], _events(rng, 30, True), [0, 30])
        se.extend([POISONED], np.array([0.25, np.nan, 0.5], np.float32), [0, 3])
        assert list(se.lengths([EXTENDED, EMPTY, POISONED, 3])) == [30, 0, 3, 0]
        refused(kind, se, [EXTENDED, N_SLOTS], f"{who}: slot {N_SLOTS} out of range (the session has {N_SLOTS})")
        refused(kind, se, [-1], f"{who}: slot -1 out of range (the session has {N_SLOTS})")
        refused(kind, se, [EXTENDED, EMPTY, EXTENDED], f"{who}: slot {EXTENDED} is named twice in one call")
        refused(kind, se, [POISONED, EXTENDED, POISONED], f"{who}: slot {POISONED} is named twice in one call")
        if kind == "open_classes":
            refused(kind, se, [EXTENDED], f"{who}: the bitmap of {N_GROUPS} groups has 1 words, not 2", n_words=2)
            # (this refusal stands in front of the slots': a bad slot beside a bad bitmap is the bitmap's message)
            refused(kind, se, [N_SLOTS], f"{who}: the bitmap of {N_GROUPS} groups has 1 words, not 2", n_words=2)

        call = Call(kind, se, 3, n_words=1 if kind == "open_classes" else None)
        assert call.run([POISONED, EXTENDED, EMPTY]) == 0, se._L.sfa_last_error().decode()
        assert not call.untouched()
        prof = al.profile()
        assert prof["class_ms"] == prof["total_ms"] > 0, prof
        if kind == "classes" or kind == "open_classes":
            rec = call.out[0] if kind == "classes" else call.out[0]["cls"]
            for i in (0, 2):  # the "none" record
                assert rec["valid"][i] == 0 and np.isposinf(rec["on_score"][i]) and np.isposinf(rec["off_score"][i]), (kind, i, rec[i])
                assert rec["on_rid"][i] == rec["off_rid"][i] == rec["on_pos_end"][i] == rec["off_pos_end"][i] == -1, (kind, i, rec[i])
            assert rec["valid"][1] == 1 and rec["n_events"][1] == 30, (kind, rec[1])
            assert np.isfinite(rec["on_score"][1]) and np.isfinite(rec["off_score"][1]) and rec["on_rid"][1] >= 0 and rec["off_rid"][1] >= 0, (kind, rec[1])
            if kind == "open_classes":
                on_g, off_g = call.out[0]["on_group"], call.out[0]["off_group"]
                assert on_g[0] == off_g[0] == on_g[2] == off_g[2] == -1 and on_g[1] in (0, 1) and off_g[1] == N_GROUPS, (on_g, off_g)  # (off: the background)
        else:
            heads = call.out[-1]
            for i in (0, 2):
                assert heads["valid"][i] == 0 and heads["best"][i] == -1 and heads["second"][i] == -1 and np.isposinf(heads["best_score"][i]), (kind, i, heads[i])
            assert heads["valid"][1] == 1 and heads["n_events"][1] == 30 and heads["best"][1] in (0, 1, 2) and np.isfinite(heads["best_score"][1]), (kind, heads[1])
            if kind == "group_bests":
                bests = call.out[0]
                for i in (0, 2):
                    assert np.isposinf(bests["score"][i]).all() and (bests["rid"][i] == -1).all() and (bests["pos_end"][i] == -1).all(), (kind, i, bests[i])
                assert np.isfinite(bests["score"][1]).all() and (bests["rid"][1] >= 0).all(), (kind, bests[1])  # both groups and the background have columns
                assert bests["score"][1].min() == heads["best_score"][1]
