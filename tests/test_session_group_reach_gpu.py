"""Reach groups of a session on the device (sfa_session_target_groups_reach / sfa_session_group_reach_tables:
reach_group_rules.hpp, sdtw_session_reachgroup.hpp) against the numpy model of tests/reach_group_model.py, bit for bit.  The shapes:
rows of 0, 1, 2 and 3 columns mod 4; jobs that begin inside a lane's quad of four columns; runs that begin at each of a quad's four
positions (asserted on the model's tables); a row of 1024 + 5 columns -- two blocks, the last quad reaching beyond the row -- and one
of 3 columns; a label that first appears in the second block; the named cases of tests/c/reach_group_rules.cpp.  The label table
and the anchors are read back; group_bests and open_classes against numpy over Session.row in event and raw mode, with and without
start columns; the live table under a group cap, which reads the depth of the anchor; the depth records over the body columns;
a plain table in place of a reach table and back; a spread session on a row of odd width; the refusals.  The lowest column of
every label, which both kernels reduce on the device, is observed where it reaches an answer: classes whose every column costs +inf."""
import ctypes as C

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib
from tests import group_oracle as G
from tests import quota_oracle as Q
from tests import reach_group_model as M
from tests.test_session_raw_gpu import SCALING, synth_signal

pytestmark = pytest.mark.gpu

# name -> (ref lengths, offsets, rna).  total columns: 1432 = 0 (mod 4) with jobs that begin at columns 31, 62, 95 ... inside quads;
# 1029 = 1 (mod 4), two blocks and a last quad of one column; 66 = 2; 3 = 3, a row shorter than a quad
SHAPES = {"dna five contigs": ([31, 33, 95, 257, 300], [7, 0, 100, 3, 1000], False), "rna 1029": ([1029], [5], True), "rna 31 + 35": ([31, 35], [2, 9], True),
          "rna 3": ([3], [4], True)}


def make_ref(rng, shape):
    lens, offs, rna = SHAPES[shape]
    arr = lambda n: (rng.integers(-6, 7, n) / 4).astype(np.float32)
    fw = [arr(n) for n in lens]
    return S.RefModel([f"c{i}" for i in range(len(lens))], [n + 5 for n in lens], lens, offs, fw, None if rna else [arr(n) for n in lens])


def flag_of(shape):
    return (S.RNA | S.INV) if SHAPES[shape][2] else 0


def strands_of(shape):
    return 1 if SHAPES[shape][2] else 2


def offsets(chunks):
    return np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)


def feed(sessions, rng, slots, n):
    chunks = [(rng.integers(-6, 7, n) / 4).astype(np.float32) for _ in slots]
    for se in sessions:
        se.extend(slots, np.concatenate(chunks), offsets(chunks))


def lists_of(shape):
    """name -> (targets, n_groups) for a shape: (contig, begin, end, lead, group, strand)"""
    lens, offs, _ = SHAPES[shape]
    if shape == "rna 3":
        return {"one column": ([(0, 5, 6, 1, 0, None)], 1), "all three": ([(0, 6, 7, 9, 1, "+"), (0, 4, 5, 0, 0, None)], 2), "minus only": ([(0, 4, 7, 2, 0, "-")], 3)}
    if shape == "rna 31 + 35":
        return {"two contigs": ([(0, 10, 14, 3, 1, None), (1, 20, 30, 40, 0, "+"), (1, 40, 44, 2, 2, "+")], 3), "1023 groups": ([(1, 12, 13, 5, 1022, None), (0, 30, 33, 1, 0, None)], 1023)}
    if shape == "rna 1029":
        # runs that begin at columns 20, 25, 30, 35 (0, 1, 2, 3 mod 4: the lead-ins) and 24, 29, 34, 39 (the bodies); group 6 first appears in
        # the second block (column 1024 on: coordinates 1029 ..), group 5 in the row's last quad
        return {"quads": ([(0, 5 + 24 + 5 * q, 5 + 26 + 5 * q, 4, q, None) for q in range(4)] + [(0, 1031, 1032, 1, 6, "+"), (0, 1033, 1034, 0, 5, None)], 7),
                "clipped at the first column": ([(0, 9, 12, 400, 4, "+"), (0, 1000, 1034, 2000, 1, None)], 5),
                "equal begins": ([(0, 40, 50, 10, 5, "+"), (0, 40, 45, 10, 2, "+"), (0, 600, 700, 0, 3, None), (0, 650, 660, 30, 0, None)], 8)}
    o = offs
    return {
        # two targets with equal begin and different groups; a body inside another group's lead-in; a lead clipped at the contig's first
        # column; '-' targets ending at and below ref_st_offset; both strands
        "named cases": ([(3, o[3] + 40, o[3] + 50, 10, 5, "+"), (3, o[3] + 40, o[3] + 45, 10, 2, "+"), (3, o[3] + 100, o[3] + 120, 60, 0, None), (3, o[3] + 70, o[3] + 75, 0, 1, None),
                         (0, o[0] + 4, o[0] + 8, 400, 4, "+"), (2, 0, 100, 20, 6, "-"), (2, 0, 101, 3, 3, "-"), (4, o[4] + 10, o[4] + 250, 25, 7, "-"), (4, o[4] + 200, o[4] + 301, 25, 6, "+"),
                         (1, 0, 34, 0, 2, None)], 8),
        "one group": ([(2, 120, 130, 11, 0, None), (4, 1100, 1150, 64, 0, "-"), (0, 7, 39, 0, 0, None)], 1),
        "1023 groups": ([(4, 1100, 1150, 64, 1022, None), (4, 1140, 1160, 64, 511, "+"), (3, 3, 4, 1 << 30, 0, None), (3, 259, 261, 1 << 30, 1, "-")], 1023),
        "empty contigs": ([(1, 10, 20, 5, 1, "-")], 2),
    }


def rnd_list(rng, shape, n, n_groups):
    lens, offs, _ = SHAPES[shape]
    out = []
    for _ in range(n):
        c = int(rng.integers(len(lens)))
        limit = offs[c] + lens[c] + 1
        b = int(rng.integers(limit))
        e = b + 1 + int(rng.integers(min(limit - b, 40)))
        out.append((c, b, e, int(rng.choice([0, 1, 7, 33, 400])), int(rng.integers(n_groups)), [None, "+", "-"][int(rng.integers(3))]))
    return out


def check_tables(se, targets, n_groups, shape, what):
    lens, offs, _ = SHAPES[shape]
    label, entry = M.tables(targets, n_groups, lens, offs, strands_of(shape))
    got_label, got_anchor = se.group_reach_tables()
    assert got_label.dtype == np.uint16 and got_anchor.dtype == np.int32 and len(got_label) == len(got_anchor) == len(label)
    assert np.array_equal(got_label, label), (what, np.flatnonzero(got_label != label)[:8])
    assert np.array_equal(got_anchor, entry), (what, np.flatnonzero(got_anchor != entry)[:8])
    assert se.group_count() == n_groups
    return label, entry


def rows_of(se, slots, shape):
    lens = SHAPES[shape][0]
    live = se.lengths(slots)
    return {sl: np.concatenate([se.row(sl, r, s)[0] for r in range(len(lens)) for s in "+-"[:strands_of(shape)]]) for sl, n in zip(slots, live) if n > 0}


def check_rows(se, slots, label, n_groups, shape, what, rows=None):
    """group_bests and open_classes (every group open; some closed) against numpy over the carried rows under `label`"""
    lens, offs, _ = SHAPES[shape]
    strands = strands_of(shape)
    rows = rows_of(se, slots, shape) if rows is None else rows
    bests, heads = se.group_bests(slots)
    opens = [None, Q.bitmap(n_groups, [g for g in range(n_groups) if g % 3 != 1] if n_groups > 1 else [])]
    got_open = [se.open_classes(slots, b) for b in opens]
    for i, sl in enumerate(slots):
        if sl not in rows:
            assert heads[i]["valid"] == 0 and heads[i]["best"] == -1 and all(g[i]["cls"]["valid"] == 0 and g[i]["on_group"] == -1 for g in got_open), (what, sl)
            continue
        want, head = G.entries_of_row(rows[sl], label, n_groups, lens, offs, strands)
        w = np.array([(s, r, p, st, (0, 0, 0)) for s, r, p, st, _ in want], S.GROUP_BEST_DTYPE)
        bad = np.flatnonzero((bests[i]["score"].view(np.uint32) != w["score"].view(np.uint32)) | (bests[i]["rid"] != w["rid"]) | (bests[i]["pos_end"] != w["pos_end"])
                             | (bests[i]["strand"] != w["strand"]))
        assert len(bad) == 0, (what, sl, bad[:5], bests[i][bad[:5]], w[bad[:5]])
        h = heads[i]
        assert h["valid"] == 1 and h["best"] == head["best"] and h["second"] == head["second"], (what, sl, h, head)
        assert np.float32(h["best_score"]).view(np.uint32) == np.float32(head["best_score"]).view(np.uint32), (what, sl, h, head)
        for bits, got in zip(opens, got_open):
            rec = Q.record_of_row(rows[sl], label, n_groups, bits, lens, offs, strands)
            c = got[i]["cls"]
            for side in ("on", "off"):
                assert np.float32(c[f"{side}_score"]).view(np.uint32) == np.float32(rec[f"{side}_score"]).view(np.uint32), (what, sl, side, got[i], rec)
                for f in ("rid", "pos_end", "strand"):
                    assert c[f"{side}_{f}"] == rec[f"{side}_{f}"], (what, sl, side, f, got[i], rec)
                assert got[i][f"{side}_group"] == rec[f"{side}_group"], (what, sl, side, got[i], rec)
            assert c["valid"] == 1


@pytest.mark.parametrize("shape", list(SHAPES))
def test_tables_are_the_models_and_the_rows_read_them(shape):
    rng = np.random.default_rng(sum(SHAPES[shape][0]))
    ref = make_ref(rng, shape)
    slots = [0, 1, 2]
    starts = set()
    with S.Aligner(ref, flag_of(shape)) as al, al.session(3) as se:
        with pytest.raises(S.SfaError, match="no reach groups"):
            se.group_reach_tables()
        feed((se,), rng, slots[1:], 30)  # (slot 0 stays empty)
        rows = rows_of(se, slots, shape)
        lists = dict(lists_of(shape))
        for k in range(3):
            ng = [3, 64, 1023][k]
            lists[f"random {k}"] = (rnd_list(rng, shape, 2 + 6 * k, ng), ng)
        for name, (targets, ng) in lists.items():  # one list replaces the other
            se.set_reach_target_groups(targets, ng)
            label, entry = check_tables(se, targets, ng, shape, name)
            check_rows(se, slots, label, ng, shape, name, rows)
            starts.update(int(c) % 4 for c in np.flatnonzero(np.diff(label.astype(np.int64)) != 0) + 1)
            if name == "quads":  # group 6 has no column in the first block, group 5 lives in the row's last quad alone
                assert M.firsts(label, ng)[6] == 1026 - 1 and M.firsts(label, ng)[5] == 1028 and len(label) == 1029
        if sum(SHAPES[shape][0]) > 8:
            assert starts == {0, 1, 2, 3}  # a run began at each of a quad's four positions
        se.set_reach_target_groups([], 1)  # off: as set_target_groups([], ..)
        assert se.group_count() == 0
        with pytest.raises(S.SfaError, match="no reach groups"):
            se.group_reach_tables()
        with pytest.raises(S.SfaError, match="no groups"):
            se.group_bests([1])


@pytest.mark.parametrize("mode", ["dna_no_start", "dna_raw", "dna_raw_no_start", "rna_no_start"])
def test_rows_in_every_mode(mode):
    rna, raw, starts = mode.startswith("rna"), "raw" in mode, "no_start" not in mode
    shape = "rna 1029" if rna else "dna five contigs"
    rng = np.random.default_rng(70 + len(mode))
    ref = make_ref(rng, shape)
    slots = [0, 1, 2]
    with S.Aligner(ref, flag_of(shape)) as al, al.session(3, starts=starts) as se:
        if raw:
            sig = [synth_signal(rng, 2000) for _ in slots[1:]]
            se.configure_raw(3, 25, 70)
            se.extend_raw(slots[1:], np.concatenate(sig), offsets(sig), [SCALING] * len(sig))
        else:
            feed((se,), rng, slots[1:], 35)
        rows = rows_of(se, slots, shape)
        for name, (targets, ng) in list(lists_of(shape).items())[:2]:
            se.set_reach_target_groups(targets, ng)
            label, _ = check_tables(se, targets, ng, shape, (mode, name))
            check_rows(se, slots, label, ng, shape, (mode, name), rows)


@pytest.mark.parametrize("shape", ["dna five contigs", "rna 1029"])
def test_lead_0_strand_0_is_set_target_groups(shape):
    rng = np.random.default_rng(83)
    ref = make_ref(rng, shape)
    lens, offs, _ = SHAPES[shape]
    ng = 5
    plain = [(c, b, e, g) for c, b, e, _, g, _ in rnd_list(rng, shape, 14, ng)]
    slots = [0, 1, 2]
    with S.Aligner(ref, flag_of(shape)) as al, al.session(3) as se, al.session(3) as twin:
        feed((se, twin), rng, slots[1:], 40)
        se.set_reach_target_groups([(c, b, e, 0, g, None) for c, b, e, g in plain], ng)
        twin.set_target_groups(plain, ng)
        label, anchor = se.group_reach_tables()
        assert np.array_equal(label.astype(np.int64), G.labels_of(plain, ng, lens, offs, strands_of(shape)))
        own = np.array([x - offs[c] for g, c, s, x in M.columns(lens, offs, strands_of(shape))])
        assert np.array_equal(anchor[label != ng], own[label != ng]) and (anchor[label == ng] == S.REACH_NONE).all()
        for a, b in zip(se.group_bests(slots), twin.group_bests(slots)):
            assert a.tobytes() == b.tobytes()
        bits = Q.bitmap(ng, [0, 2, 3])
        assert se.open_classes(slots, bits).tobytes() == twin.open_classes(slots, bits).tobytes()


# ---- classes whose every column costs +inf: the only place where the lowest column of every label, which the build kernel and the
# live kernel reduce on the device, reaches an answer (sfa_session_open_classes places such a class at its lowest column) ----
def test_classes_of_inf_columns_are_placed_by_the_kernels_firsts():
    """A row of 1026 + 43 columns (two blocks, 1 mod 4).  Contig 1 lies in the second block and its levels are 3e38, so its columns
    cost +inf; contig 0 is finite and one group covers all of it.  Every label but that group has its lowest column in the second
    block, at positions 1, 2 and 2 of a quad; under the cap the lowest LIVE column of group 0 moves from 1033 to 1037."""
    lens, offs = [1026, 43], [5, 9]
    rng = np.random.default_rng(107)
    arr = lambda n: (rng.integers(-6, 7, n) / 4).astype(np.float32)
    ref = S.RefModel(["c0", "c1"], [n + 5 for n in lens], lens, offs, [arr(lens[0]), np.full(lens[1], 3e38, np.float32)], None)
    at = lens[0]  # contig 1's first column; column at + j reports coordinate 9 + j
    # group 0: body j 10 .. 14 with a lead-in j 7 .. 9; group 1: j 32 .. 34; group 2: all of contig 0; group 3: no column
    targets, ng = [(1, 19, 24, 3, 0, "+"), (1, 41, 44, 0, 1, None), (0, 5, 5 + lens[0], 0, 2, None)], 4
    slots = [2, 0, 1]
    with S.Aligner(ref, S.RNA | S.INV) as al, al.session(3) as se:
        chunks = [arr(9) for _ in slots]
        se.extend(slots, np.concatenate(chunks), offsets(chunks))
        rows = {sl: np.concatenate([se.row(sl, r, "+")[0] for r in range(2)]) for sl in slots}
        for sl in slots:
            assert np.isposinf(rows[sl][at:]).all() and np.isfinite(rows[sl][:at]).all()
        se.set_reach_target_groups(targets, ng)
        label, entry = M.tables(targets, ng, lens, offs, 1)
        got_label, got_anchor = se.group_reach_tables()
        assert np.array_equal(got_label, label) and np.array_equal(got_anchor, entry)
        assert list(M.firsts(label, ng)) == [at + 7, at + 32, 0, -1, at] and at + 7 == 1033 and at > 1024

        def check(lab, what):
            out = {}
            for name, open_groups in (("g0", [0]), ("g0 g1", [0, 1]), ("g1", [1]), ("g2", [2]), ("g0 g2", [0, 2]), ("g3", [3]), ("all", None)):
                bits = None if open_groups is None else Q.bitmap(ng, open_groups)
                got = se.open_classes(slots, bits)
                for i, sl in enumerate(slots):
                    rec = Q.record_of_row(rows[sl], lab, ng, bits, lens, offs, 1)
                    c = got[i]["cls"]
                    for side in ("on", "off"):
                        assert np.float32(c[f"{side}_score"]).view(np.uint32) == np.float32(rec[f"{side}_score"]).view(np.uint32), (what, name, sl, side, got[i], rec)
                        for f in ("rid", "pos_end", "strand"):
                            assert c[f"{side}_{f}"] == rec[f"{side}_{f}"], (what, name, sl, side, f, got[i], rec)
                        assert got[i][f"{side}_group"] == rec[f"{side}_group"], (what, name, sl, side, got[i], rec)
                out[name] = got
            return out

        # ---- without a cap: the build kernel's firsts ----
        got = check(label, "base")
        for name, col, group in (("g0", at + 7, 0), ("g0 g1", at + 7, 0), ("g1", at + 32, 1)):  # ON is +inf at the open labels' lowest column
            assert np.isposinf(got[name]["cls"]["on_score"]).all() and (got[name]["cls"]["on_rid"] == 1).all() and (got[name]["cls"]["on_pos_end"] == offs[1] + col - at).all(), name
            assert (got[name]["on_group"] == group).all() and np.isfinite(got[name]["cls"]["off_score"]).all()
        for name in ("g2", "g0 g2"):  # everything finite is ON: OFF is +inf at contig 1's first column, the background's lowest
            assert np.isposinf(got[name]["cls"]["off_score"]).all() and (got[name]["cls"]["off_rid"] == 1).all() and (got[name]["cls"]["off_pos_end"] == offs[1]).all(), name
            assert (got[name]["off_group"] == ng).all() and np.isfinite(got[name]["cls"]["on_score"]).all()
        assert (got["g3"]["cls"]["on_rid"] == -1).all() and (got["g3"]["on_group"] == -1).all()
        # ---- under a group cap, after an add over group 0's first base: the live kernel's firsts ----
        se.configure_group_coverage(1)
        check(label, "cap, depth 0")
        se.add_coverage([(1, 19, 20)])
        live = M.live_labels(label, entry, [se.coverage(c) for c in range(2)], 1, ng, lens, 1)
        assert list(M.firsts(live, ng)) == [at + 11, at + 32, 0, -1, at] and (live[at + 7:at + 11] == ng).all()  # the lead-in and the first base closed
        got = check(live, "cap, after the add")
        assert (got["g0"]["cls"]["on_pos_end"] == offs[1] + 11).all() and (got["g0"]["on_group"] == 0).all() and np.isposinf(got["g0"]["cls"]["on_score"]).all()
        se.add_coverage([(1, 9, 10)])  # the background's own depth closes nothing: its lowest column stays
        got = check(live, "cap, the background covered")
        assert (got["g2"]["cls"]["off_pos_end"] == offs[1]).all() and (got["g2"]["off_group"] == ng).all()
        se.add_coverage([(1, 20, 24)])  # the rest of group 0: no live column is left, ON under [0] is empty
        live = M.live_labels(label, entry, [se.coverage(c) for c in range(2)], 1, ng, lens, 1)
        assert M.firsts(live, ng)[0] == -1
        got = check(live, "cap, group 0 full")
        assert (got["g0"]["cls"]["on_rid"] == -1).all() and (got["g0"]["on_group"] == -1).all()


def depth_of(se, shape):
    return [se.coverage(c) for c in range(len(SHAPES[shape][0]))]


def check_capped(se, slots, targets, ng, cap, shape, what, rows):
    """under a group cap: the rows read the model's live table, the records are the model's over the body columns"""
    lens, offs, _ = SHAPES[shape]
    label, entry = M.tables(targets, ng, lens, offs, strands_of(shape))
    depth = depth_of(se, shape)
    live = M.live_labels(label, entry, depth, cap, ng, lens, strands_of(shape))
    check_rows(se, slots, live, ng, shape, what, rows)
    want = np.array(M.records(label, entry, depth, cap, ng, lens, offs, strands_of(shape)), S.GROUP_COVER_DTYPE)
    got = se.group_coverage()
    assert got.tobytes() == want.tobytes(), (what, got, want)
    assert np.array_equal(se.group_reach_tables()[0], label)  # (the base table is kept beside the live one)
    return label, live


@pytest.mark.parametrize("shape", ["dna five contigs", "rna 1029"])
def test_the_group_cap_reads_the_depth_of_the_anchor(shape):
    rng = np.random.default_rng(89)
    ref = make_ref(rng, shape)
    lens, offs, rna = SHAPES[shape]
    c = 0 if rna else 3
    o = offs[c]
    # group 0: a '+' body at o + 40 .. o + 50 with a lead-in of 10; group 1 overlaps its tail with a lead of its own; group 2 on '-' only
    targets = [(c, o + 40, o + 50, 10, 0, "+"), (c, o + 48, o + 60, 4, 1, None), (c, o + 20, o + 25, 6, 2, "-")] + ([] if rna else [(4, 1100, 1150, 64, 1, None), (2, 0, 100, 20, 2, "-")])
    ng, cap, slots = 3, 2, [0, 1, 2]
    with S.Aligner(ref, flag_of(shape)) as al, al.session(3) as se:
        feed((se,), rng, slots[1:], 40)
        rows = rows_of(se, slots, shape)
        se.set_reach_target_groups(targets, ng)
        se.configure_group_coverage(cap)
        label, live = check_capped(se, slots, targets, ng, cap, shape, "depth 0", rows)
        assert np.array_equal(live, label)
        at = 0 if rna else 2 * sum(lens[:c])  # the '+' job's first column
        col = lambda x: at + x - o
        steps = [([(c, o + 40, o + 41)], "the first base once: cap - 1"), ([(c, o + 40, o + 41)], "the first base at the cap"), ([(c, o + 30, o + 40)] * 3, "the lead-in, not the body"),
                 ([(c, o + 20, o + 25)] * 2 + ([] if rna else [(4, 1100, 1101)] * 2), "the '-' group's last base but one; a body's first base")]
        for k, (iv, what) in enumerate(steps):
            se.add_coverage(iv)
            label, live = check_capped(se, slots, targets, ng, cap, shape, what, rows)
            if k == 0:
                assert np.array_equal(live, label)
            if k >= 1:  # the lead-in o + 30 .. o + 39 and the first base are closed, the rest of the body stays
                assert (live[col(o + 30):col(o + 41)] == ng).all() and (live[col(o + 41):col(o + 48)] == 0).all() and (label[col(o + 30):col(o + 48)] == 0).all()
            if k == 2:  # covering the lead-in closed nothing more
                assert int((live != ng).sum()) == before
            before = int((live != ng).sum())
        rec = se.group_coverage()
        assert rec["columns"][0] == 10 and rec["columns"][2] == 0 and rec["depth_min"][2] == 0xffffffff and rec["columns"][ng] == 0  # body columns of '+' jobs; a '-' group is empty
        # ---- reach -> plain -> reach: the depth is kept, the live table is derived again each time ----
        depth = [d.copy() for d in depth_of(se, shape)]
        plain = [(c, o + 30, o + 60, 1), (c, o + 10, o + 12, 0)]
        se.set_target_groups(plain, 2)
        with pytest.raises(S.SfaError, match="no reach groups"):
            se.group_reach_tables()
        assert all(np.array_equal(a, b) for a, b in zip(depth, depth_of(se, shape)))
        pl = G.labels_of(plain, 2, lens, offs, strands_of(shape))
        own = np.array([depth[cc][x - offs[cc]] >= cap for g, cc, s, x in M.columns(lens, offs, strands_of(shape))])
        check_rows(se, slots, np.where(own, 2, pl), 2, shape, "a plain table reads the column's own depth", rows)
        se.set_reach_target_groups(targets, ng)
        check_capped(se, slots, targets, ng, cap, shape, "reach again", rows)
        se.configure_group_coverage(0)
        check_rows(se, slots, label, ng, shape, "cap off", rows)
        se.configure_group_coverage(cap)
        se.set_reach_target_groups([], ng)
        with pytest.raises(S.SfaError, match="no group cap"):
            se.group_coverage()


def test_spread_session_on_a_row_of_odd_width():
    shape = "rna 1029"
    rng = np.random.default_rng(97)
    ref = make_ref(rng, shape)
    order = [4, 0, 3, 1]
    targets, ng = lists_of(shape)["quads"]
    with S.Aligner(ref, flag_of(shape)) as one, S.Aligner(ref, flag_of(shape), devices=[0, 0]) as many:
        with one.session(5) as plain, many.session(5, spread=True) as spread:
            feed((plain, spread), rng, [1, 2, 3, 4], 45)
            for se in (plain, spread):
                se.set_reach_target_groups(targets, ng)
            label, _ = check_tables(spread, targets, ng, shape, "spread")
            assert spread.group_count() == ng
            for a, b in zip(spread.group_bests(order), plain.group_bests(order)):
                assert a.tobytes() == b.tobytes()
            assert spread.open_classes(order, Q.bitmap(ng, [0, 5, 6])).tobytes() == plain.open_classes(order, Q.bitmap(ng, [0, 5, 6])).tobytes()
            for se in (plain, spread):
                se.configure_group_coverage(1)
                se.add_coverage([(0, 5 + 24, 5 + 25), (0, 1031, 1032)])
            assert spread.group_coverage().tobytes() == plain.group_coverage().tobytes()
            for a, b in zip(spread.group_bests(order), plain.group_bests(order)):
                assert a.tobytes() == b.tobytes()
            with pytest.raises(S.SfaError, match="group 7 out of range"):
                spread.set_reach_target_groups([(0, 40, 50, 3, 7, None)], ng)
            check_tables(spread, targets, ng, shape, "a refusal on every shard leaves every shard as it was")
            spread.set_target_groups([(0, 40, 50, 0)], 1)
            with pytest.raises(S.SfaError, match="no reach groups"):
                spread.group_reach_tables()


def test_refusals_leave_the_session_as_it_was():
    shape = "dna five contigs"
    rng = np.random.default_rng(101)
    ref = make_ref(rng, shape)
    lib = _lib.load()
    targets, ng = lists_of(shape)["named cases"]
    with S.Aligner(ref, 0) as al, al.session(3) as se:
        feed((se,), rng, [0, 1, 2], 30)
        se.set_reach_target_groups(targets, ng)
        se.configure_group_coverage(3)
        se.add_coverage([(4, 1100, 1120)])
        depth = se.coverage(4)
        before = [x.tobytes() for x in se.group_bests([0, 1, 2])]
        good = (4, 1000, 1301, 1 << 30, 1, "-")
        bad = [((-1, 0, 1, 0, 0, None), "contig -1 out of range"), ((5, 0, 1, 0, 0, None), "contig 5 out of range"), ((2, -1, 4, 0, 0, None), "is negative"), ((2, 4, 4, 0, 0, None), "is empty"),
               ((2, 100, 197, 0, 0, None), "lies beyond contig 2"), ((2, 100, 110, -1, 0, None), "lead -1 outside"), ((2, 100, 110, (1 << 30) + 1, 0, None), "outside 0 .. 1073741824"),
               ((2, 100, 110, 3, 0, "x"), "strand 120"), ((2, 100, 110, 3, 0, 1), "strand 1 is none"), ((2, 100, 110, 3, -1, None), "group -1 out of range"),
               ((2, 100, 110, 3, ng, None), f"group {ng} out of range")]
        for t, word in bad:
            with pytest.raises(S.SfaError, match=word) as err:
                se.set_reach_target_groups([good, t], ng)
            assert "sfa_session_target_groups_reach: target 1:" in str(err.value)
        for n_groups in (0, -1, 1024):
            with pytest.raises(S.SfaError, match="n_groups .* is not in 1 .. 1023"):
                se.set_reach_target_groups([good], n_groups)
        padded = np.zeros(2, S.REACH_GROUP_TARGET_DTYPE)
        padded[0] = padded[1] = (4, 1100, 1150, 5, 0, 0, (0, 0, 0))
        padded["pad"][1][2] = 1
        with pytest.raises(S.SfaError, match="target 1: the padding is not zero"):
            se.set_reach_target_groups(padded, ng)
        with pytest.raises(S.SfaError, match="at most 1048576"):
            se.set_reach_target_groups(np.zeros((1 << 20) + 1, S.REACH_GROUP_TARGET_DTYPE), ng)
        assert lib.sfa_session_target_groups_reach(None, None, 0, 1) != 0 and lib.sfa_session_target_groups_reach(se._h, None, 2, 1) != 0 and b"bad argument" in lib.sfa_last_error()
        # the tables, the answers and the depth are what they were
        label, entry = check_tables(se, targets, ng, shape, "after the refusals")
        assert [x.tobytes() for x in se.group_bests([0, 1, 2])] == before and np.array_equal(se.coverage(4), depth)
        # sfa_session_group_reach_tables: the size, and either pointer may be NULL
        cols = len(label)
        l, a = np.full(cols + 1, 9, np.uint16), np.full(cols + 1, 7, np.int32)
        lp, ap = l.ctypes.data_as(C.POINTER(C.c_uint16)), a.ctypes.data_as(_lib.i32p)
        for nc in (cols - 1, cols + 1, 0):
            assert lib.sfa_session_group_reach_tables(se._h, lp, ap, nc) != 0
        assert (l == 9).all() and (a == 7).all()  # nothing was written by a refused call
        assert lib.sfa_session_group_reach_tables(se._h, lp, None, cols) == 0 and lib.sfa_session_group_reach_tables(se._h, None, ap, cols) == 0
        assert lib.sfa_session_group_reach_tables(se._h, None, None, 0) == 0 and lib.sfa_session_group_reach_tables(None, lp, ap, cols) != 0
        assert l[cols] == 9 and a[cols] == 7 and np.array_equal(l[:cols], label) and np.array_equal(a[:cols], entry)  # nothing behind the tables was touched
        se.set_reach_target_groups([good], ng)  # the longest lead and a '-' target over a whole contig pass
        assert int((se.group_reach_tables()[0] != ng).sum()) == SHAPES[shape][0][4]
        with al.session(2, resweep=True) as rs:
            with pytest.raises(S.SfaError, match="RESWEEP"):
                rs.set_reach_target_groups([good], ng)
            with pytest.raises(S.SfaError, match="no reach groups"):
                rs.group_reach_tables()
