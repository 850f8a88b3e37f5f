"""Target classes of a session on the GPU (sfa_session_targets / sfa_session_classes: target_rules.hpp, sdtw_session_class.hpp).
The yardstick is numpy over the carried rows Session.row() reads back, under the Python restatement of the mask
(tests/targets_oracle.py): scores bit for bit, contig, coordinate and strand equal, after EVERY extend call.  Reference: contigs
of 37, 64, 65 and 300 k-mers, 9 slots.  Jobs begin inside mask words and inside 16-byte quads, but of the kernel's paths these
shapes reach few (tests/test_class_shapes_cpu.py::test_what_the_existing_shapes_reach): a DNA row has 932 columns, a multiple of 4,
so every slot begins on a 16-byte boundary and has neither head nor tail; an RNA row has 466, so slots begin 0 or 2 words behind a
boundary, with a head of 0 or 2 columns and a tail of 2 or 0, and a quad's mask bits straddle two words at shift 30 only.  A row is
one part, and only the first of a lane's eight quads (u == 0) has a column.  Every other alignment, heads and tails of 1 and 3
columns, shifts 29 and 31, u >= 1, several parts, ties across lanes, waves and parts, and the classes whose every column costs +inf
are tests/test_session_class_edges_gpu.py's.
A twin session without targets takes the same calls: its rows must be the same bytes.
The class coordinate is tied to what a finalized row reports (pos_end on '+', pos_st on '-'), and one replay(targets=...) run of 12
synthetic reads on 4 channels, with enrich and with deplete, is compared with `sigfish-amd realtime --targets`: stdout, trace and
summary line, every line's tc / ac / tm recomputed from the class record."""
import numpy as np
import pytest

import sigfish_amd as S
from tests import targets_oracle as T
from tests.test_session_gpu import _events, _small_ref
from tests.test_session_raw_gpu import SCALING, synth_signal

pytestmark = pytest.mark.gpu

LENS = [37, 64, 65, 300]
N_SLOTS = 9
CHUNKS = (7, 50, 120)
FIELDS = ("rid", "pos_end", "strand")


def whole(ref, r):
    return (r, int(ref.st_offset[r]), int(ref.st_offset[r]) + int(ref.ref_lengths[r]) + 1)


def target_sets(ref, strands):
    """name -> list of (contig, begin, end)"""
    off = [int(x) for x in ref.st_offset]
    sets = {
        # column 0 of (c0, '+'), column 299 of (c3, '+'), column 0 of (c1, '-') and column 64 of (c2, '-'): first and last columns of
        # jobs, each alone in its neighbourhood ((c2, '+') column 1 comes with the last one)
        "first and last columns": [(0, off[0], off[0] + 1), (3, off[3] + 299, off[3] + 300), (1, off[1] + 64, off[1] + 65), (2, off[2] + 1, off[2] + 2)],
        "everything": [whole(ref, r) for r in range(4)],
        "a contig": [whole(ref, 2)],
        "scattered, unsorted, overlapping": [(3, off[3] + 200, off[3] + 290), (3, off[3] + 10, off[3] + 40), (1, off[1] + 3, off[1] + 33), (3, off[3] + 30, off[3] + 64),
                                             (0, off[0] + 36, off[0] + 38)],
    }
    if min(off) > 0:  # coordinates below the offset belong to no column: a valid list with nothing on target
        sets["nothing"] = [(r, 0, off[r]) for r in range(4)]
    return sets


def slot_row(se, sl, strands, n_ref=4):
    return np.concatenate([se.row(sl, r, s)[0] for r in range(n_ref) for s in "+-"[:strands]])


def check_classes(se, slots, targets, ref, strands, what, dead=(), mask=None):
    """Session.classes of `slots` against numpy over the rows; -> the records.  mask: T.mask_of's answer for `targets`, where
    the caller has it already (rows of 10^5 columns)"""
    if mask is None:
        mask = T.mask_of(targets, ref.ref_lengths, ref.st_offset, strands)
    assert se.target_columns() == int(mask.sum()), what
    got = se.classes(slots)
    lens = se.lengths(slots)
    for i, sl in enumerate(slots):
        g = got[i]
        if lens[i] == 0 or sl in dead:
            assert g["valid"] == 0 and np.isinf(g["on_score"]) and np.isinf(g["off_score"]) and g["on_rid"] == -1 and g["off_rid"] == -1, (what, sl, g)
            continue
        assert g["valid"] == 1 and g["n_events"] == lens[i], (what, sl, g)
        want = T.classes_of_rows(slot_row(se, sl, strands, ref.num_ref), mask, ref.ref_lengths, ref.st_offset, strands)
        for side in ("on", "off"):
            assert np.float32(g[f"{side}_score"]).view(np.uint32) == np.float32(want[f"{side}_score"]).view(np.uint32), (what, sl, side, g, want)
            for f in FIELDS:
                assert int(g[f"{side}_{f}"]) == int(want[f"{side}_{f}"]), (what, sl, side, f, g, want)
    return got


def offsets(chunks):
    return np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "no_start"])
@pytest.mark.parametrize("rna", [False, True], ids=["dna", "rna_inv"])
def test_classes_after_every_extend(rna, starts):
    rng = np.random.default_rng(7 + rna)
    ref = _small_ref(rng, LENS, rna)
    flag = (S.RNA | S.INV) if rna else 0
    strands = 1 if rna else 2
    sets = target_sets(ref, strands)
    assert ("nothing" in sets) == rna
    data = {sl: _events(rng, 3 * sum(CHUNKS), True) for sl in range(N_SLOTS)}
    used = dict.fromkeys(range(N_SLOTS), 0)
    with S.Aligner(ref, flag) as al, al.session(N_SLOTS, starts=starts) as se, al.session(N_SLOTS, starts=starts) as twin:
        with pytest.raises(S.SfaError, match="no targets"):
            se.classes([0])
        assert se.target_columns() == 0
        names = list(sets)
        step = 0
        for _ in range(3):
            for n in CHUNKS:
                # slot 8 stays empty until the last round; the others grow, in descending order of the call
                slots = [sl for sl in range(N_SLOTS - 1, -1, -1) if sl != 8 or step >= 6]
                chunks = [data[sl][used[sl]:used[sl] + n] for sl in slots]
                ev, off = np.concatenate(chunks), offsets(chunks)
                name = names[step % len(names)]
                se.set_targets(sets[name])  # (replaced mid-read: the mask does not depend on the slots' state)
                rows = se.extend(slots, ev, off)
                assert rows.tobytes() == twin.extend(slots, ev, off).tobytes(), (name, step)
                for sl in slots:
                    used[sl] += n
                got = check_classes(se, list(range(N_SLOTS - 1, -1, -1)), sets[name], ref, strands, (name, step))
                if name == "everything":
                    assert (got["off_rid"][got["valid"] == 1] == -1).all() and np.isinf(got["off_score"]).all()
                if name == "nothing":
                    assert (got["on_rid"] == -1).all() and np.isinf(got["on_score"]).all() and (got["on_pos_end"] == -1).all() and (got["on_strand"] == 0).all()
                step += 1
        # whole-call refusals, and what a refused call leaves
        with pytest.raises(S.SfaError, match="named twice"):
            se.classes([1, 2, 1])
        with pytest.raises(S.SfaError, match="out of range"):
            se.classes([0, N_SLOTS])
        with pytest.raises(S.SfaError, match="beyond"):
            se.set_targets([(0, 0, 10 ** 6)])
        name = names[0]
        se.set_targets(sets[name])
        check_classes(se, [3, 0, 8], sets[name], ref, strands, "after refusals")
        # a poisoned slot, and a slot after reset (empty until its next chunk)
        bad = np.array([0.25, np.nan, 0.5], np.float32)
        se.extend([2], bad, [0, 3])
        se.reset([5])
        got = check_classes(se, [5, 2, 4], sets[name], ref, strands, "poisoned and reset", dead=(2,))
        assert list(got["valid"]) == [0, 0, 1]
        se.extend([5], data[5][:11], [0, 11])
        got = check_classes(se, [5], sets[name], ref, strands, "after reset")
        assert got["valid"][0] == 1 and got["n_events"][0] == 11
        # switched off
        se.set_targets([])
        assert se.target_columns() == 0
        with pytest.raises(S.SfaError, match="no targets"):
            se.classes([4])


def test_ties_go_to_the_lowest_column():
    """Contig 1 (64 k-mers) is the first 64 k-mers of contig 2 on both strands and the model has two levels: a column's cost depends
    on the columns to its left only, so the two jobs' rows agree column by column and every minimum of one occurs in the other."""
    rng = np.random.default_rng(3)
    lv = lambda n: rng.choice(np.array([-0.5, 0.5], np.float32), n)
    fw = [lv(37), None, lv(65), lv(300)]
    rv = [lv(37), None, lv(65), lv(300)]
    fw[1], rv[1] = fw[2][:64].copy(), rv[2][:64].copy()
    ref = S.RefModel([f"c{i}" for i in range(4)], [n + 5 for n in LENS], LENS, [0] * 4, fw, rv)
    targets = [whole(ref, 1), whole(ref, 2)]
    mask = T.mask_of(targets, ref.ref_lengths, ref.st_offset, 2)
    with S.Aligner(ref, 0) as al, al.session(N_SLOTS) as se:
        se.set_targets(targets)
        n_tied = 0
        starts = [j[3] for j in T.jobs_of(LENS, 2)]
        for n in CHUNKS:
            chunks = [lv(n) for _ in range(N_SLOTS)]
            se.extend(list(range(N_SLOTS)), np.concatenate(chunks), offsets(chunks))
            got = check_classes(se, list(range(N_SLOTS)), targets, ref, 2, ("ties", n))
            for sl in range(N_SLOTS):  # the inputs really tie: the class minimum stands in columns of two jobs, and the lowest won
                row = slot_row(se, sl, 2)
                at = np.flatnonzero(mask & (row == got["on_score"][sl]))
                jobs = {int(np.searchsorted(starts, g, side="right")) - 1 for g in at}
                n_tied += len(jobs) >= 2  # (that the lowest of the tied columns won is check_classes' comparison)
        assert n_tied >= N_SLOTS


def test_raw_mode_and_resweep_refusal():
    rng = np.random.default_rng(11)
    ref = _small_ref(rng, LENS, False)
    sets = target_sets(ref, 2)
    targets = sets["scattered, unsorted, overlapping"]
    with S.Aligner(ref, 0) as al:
        with al.session(N_SLOTS, starts=False) as se:
            se.configure_raw(3, 25, 70)
            se.set_targets(targets)
            sig = {sl: synth_signal(rng, 1500) for sl in range(N_SLOTS)}
            slots = list(range(N_SLOTS - 1))  # (the last slot stays empty)
            for k in range(3):
                chunks = [sig[sl][500 * k:500 * (k + 1)] for sl in slots]
                _, info = se.extend_raw(slots, np.concatenate(chunks), offsets(chunks), [SCALING] * len(slots))
                got = check_classes(se, list(range(N_SLOTS)), targets, ref, 2, ("raw", k))
                assert np.array_equal(got["n_events"][:-1], info["q_events"]) and got["valid"][-1] == 0
            assert (got["valid"][:-1] == 1).all()
        with al.session(2, resweep=True) as se:
            with pytest.raises(S.SfaError, match="RESWEEP"):
                se.set_targets(targets)
            with pytest.raises(S.SfaError, match="no targets"):
                se.classes([0])


def test_spread_session_answers_as_a_plain_one():
    rng = np.random.default_rng(13)
    ref = _small_ref(rng, LENS, False)
    targets = target_sets(ref, 2)["scattered, unsorted, overlapping"]
    data = [_events(rng, 57, True) for _ in range(N_SLOTS)]
    with S.Aligner(ref, 0) as one, S.Aligner(ref, 0, devices=[0, 0]) as many:
        with one.session(N_SLOTS) as plain, many.session(N_SLOTS, spread=True) as spread:
            for se in (plain, spread):
                se.set_targets(targets)
                se.extend(list(range(1, N_SLOTS)), np.concatenate(data[1:]), offsets(data[1:]))  # (slot 0 stays empty)
            assert spread.target_columns() == plain.target_columns() > 0
            order = [7, 0, 8, 1, 2, 6, 3]
            want = check_classes(plain, order, targets, ref, 2, "plain")
            assert spread.classes(order).tobytes() == want.tobytes()
            assert many.profile()["class_ms"] > 0 and one.profile()["class_ms"] > 0
            with pytest.raises(S.SfaError, match="named twice"):
                spread.classes([1, 1])
            spread.set_targets([])
            with pytest.raises(S.SfaError, match="no targets"):
                spread.classes([1])


def test_decision_from_the_device_record():
    """target_decide over a record the device wrote: the layout the host rule reads is the one the kernel writes"""
    rng = np.random.default_rng(17)
    ref = _small_ref(rng, LENS, False)
    with S.Aligner(ref, 0) as al, al.session(2) as se:
        se.set_targets([whole(ref, 3)])
        q = ref.forward[3][100:160].copy()  # a read from the target: cost 0 on target
        se.extend([0], q, [0, len(q)])
        c = se.classes([0])[0]
        assert c["on_score"] == 0 and c["on_rid"] == 3 and c["on_strand"] == ord("+") and c["on_pos_end"] <= 159 and c["off_score"] > 0
        per_event = float(c["off_score"]) / 60
        assert S.target_decide(c, S.ENRICH, 60, per_event * 0.99) == "A" and S.target_decide(c, S.DEPLETE, 60, per_event * 0.99) == "U"
        assert S.target_decide(c, S.ENRICH, 61, per_event * 0.99) is None and S.target_decide(c, S.ENRICH, 60, per_event * 1.01) is None


def test_class_coordinate_is_what_a_finalized_row_reports():
    """The class winner of a read that is also the row's best window: on '+' on_pos_end is the row's pos_end, on '-' it is the
    row's pos_st (the flip swaps the two) -- the values come from the finalize kernels, not from the tests' restatement."""
    rng = np.random.default_rng(19)
    ref = _small_ref(rng, LENS, False, quant=False)
    with S.Aligner(ref, 0) as al, al.session(2) as se:
        se.set_targets([whole(ref, 3)])
        fwd, rev = ref.forward[3][100:160].copy(), ref.reverse[3][40:100].copy()
        rows = se.extend([0, 1], np.concatenate([fwd, rev]), [0, 60, 120])
        c = se.classes([0, 1])
        assert list(rows["rid"]) == [3, 3] and list(rows["strand"]) == [ord("+"), ord("-")] and (rows["score"] == 0).all()
        assert (c["on_score"] == 0).all() and list(c["on_rid"]) == [3, 3] and list(c["on_strand"]) == [ord("+"), ord("-")]
        assert int(c["on_pos_end"][0]) == int(rows["pos_end"][0]) == 159  # columns 100 .. 159 of '+'
        assert int(c["on_pos_end"][1]) == int(rows["pos_st"][1]) == 300 - 99  # columns 40 .. 99 of '-': the end column flipped
        assert int(rows["pos_end"][1]) == 300 - 40


# ---- the real-time front ends: replay(targets=...) and `sigfish-amd realtime --targets` ----
def _tags3(line):
    f = line.rstrip("\n").split("\t")[-3:]
    assert f[0].startswith("tc:A:") and f[1].startswith("ac:A:") and f[2].startswith("tm:f:"), line
    return f[0][5:], f[1][5:], f[2][5:]


@pytest.mark.parametrize("mode", ["enrich", "deplete"])
def test_replay_with_targets_and_the_binary(mode, tmp_path):
    import os
    import subprocess

    from sigfish_amd import realtime, synth
    from tests.realtime_util import BIN, write_model
    from tests.test_session_raw_gpu import META

    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    k = 6
    model = write_model(tmp_path / "syn.model", k, synth.kmer_levels(k, 21))
    levels, _ = S.read_kmer_model(model)
    c0 = synth.random_sequence(905, 1)
    recs = [("c0", c0), ("c1", c0[300:605]), ("c2", synth.random_sequence(62, 3))]
    fasta, blow5, bed, trace_file = (str(tmp_path / n) for n in ("ref.fa", "reads.blow5", "t.bed", "trace.txt"))
    with open(fasta, "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in recs))
    reads = synth.make_dna_raw_reads(recs, levels, k, 12, seed=5, samples=(2000, 9000), kinds=("mapped", "mapped", "random", "mapped", "stalled", "flat"),
                                     meta={**META, "sampling_rate": 4000.0})
    synth.write_blow5(blow5, reads)
    with open(bed, "w") as f:
        f.write("# targets\ntrack name=t\nc0\t100\t700\nc1\t0\t301\n")
    ref = S.RefModel.from_fasta(fasta, levels, k, 0, 70)
    skip, norm, query, min_events, channels, chunk, margin = 3, 25, 70, 30, 4, 800, 0.05
    m = S.ENRICH if mode == "enrich" else S.DEPLETE
    run = subprocess.run([BIN, "realtime", "--kmer-model", model, "--verbose", "0", "--channels", str(channels), "--chunk-samples", str(chunk), "-p", str(skip), "-q", str(query),
                          "--norm-events", str(norm), "--min-events", str(min_events), "--targets", bed, f"--{mode}", "--margin", str(margin), "--trace", trace_file, fasta, blow5],
                         capture_output=True, timeout=300)
    assert run.returncode == 0, run.stderr.decode()
    reads = list(S.Blow5File(blow5))
    targets = S.read_targets(bed, ref.names)
    trace, summary, lines, actions = [], {}, [], []
    with S.Aligner(ref, 0) as al:
        for tick, ch, index, row, info, span, why, cls, action in realtime.replay(al, reads, channels, chunk, skip, norm, query, min_events, 61, trace=trace, targets=targets,
                                                                                  mode=m, margin=margin, summary=summary):
            rid, _, raw = reads[index]
            line = realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why, target=(cls, m, min_events, margin))
            lines.append(line)
            actions.append(action)
            dec = S.target_decide(cls, m, min_events, margin)  # the tags recomputed from the class record
            assert action == (dec if why == "E" else "P") and (why == "E") == (dec is not None), (why, dec, cls)
            if line:
                tc, ac, tm = _tags3(line)
                assert ac == action and tc == ("N" if dec is None else ("T" if (dec == "A") == (m == S.ENRICH) else "O")), line
                mine, other = (cls["on_score"], cls["off_score"]) if m == S.ENRICH else (cls["off_score"], cls["on_score"])
                assert tm == "%.4f" % ((float(other) - float(mine)) / int(cls["n_events"])), line
                if why == "E":
                    assert abs(float(tm)) >= margin
    assert run.stdout.decode() == "".join(lines)
    assert open(trace_file).read().splitlines() == trace
    assert run.stderr.decode().splitlines()[-1] + "\n" == realtime.format_summary(summary)
    assert len(actions) == 12 and set(actions) & {"A", "U"}, actions  # (about this test's own inputs: class decisions occur)
    assert any(" hold " in ln for ln in trace) and sum(v[0] for v in summary.values()) == 12
