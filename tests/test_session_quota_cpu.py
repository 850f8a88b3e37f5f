"""Open and closed groups and quotas without a GPU: the stand-alone program tests/c/quota_rules.cpp, built from
sigfish_amd/csrc/quota_rules.hpp alone with -Wall -Werror and once more under ASan + UBSan (its selftest checks the record against a
per-column brute force, the bitmap's word edges, the tie rule and the quota book); the numpy restatement the GPU test relies on
(tests/quota_oracle.py) against the header's records; the quota book of the header, of the package and of the oracle on one script;
the schedule with a quota as replay.hpp and its Python twin run it (tests/c/replay_quota.cpp, under ASan + UBSan); the tag formatter
of both languages; open_words; the refusals of --quota / quota=, which come before any file, session or device is opened."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib, realtime
from tests import group_oracle as G
from tests import quota_oracle as Q
from tests.realtime_util import BIN, write_model
from tests.test_session_groups_cpu import _ask, _programs
from tests.util import GOLD, ROOT


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return _programs(tmp_path_factory.mktemp("quota_rules"), "quota_rules.cpp", "quota_rules")


@pytest.fixture(scope="module")
def tag_programs(tmp_path_factory):
    return _programs(tmp_path_factory.mktemp("quota_tags"), "quota_tags.cpp", "quota_tags")


@pytest.fixture(scope="module")
def schedule_programs(tmp_path_factory):
    return _programs(tmp_path_factory.mktemp("replay_quota"), "replay_quota.cpp", "replay_quota")


def test_selftest_plain_and_under_sanitizers(programs):
    line = _ask(programs, "selftest\n")[-1].split()
    assert line[:2] == ["selftest", "ok"] and int(line[2]) > 500


# ---- the numpy restatement against the header: row, labels and bitmap in, record out ----
LENS = [1, 31, 32, 33, 64, 65, 300]
OFFS = [0, 7, 0, 100, 3, 0, 1000]
#        targets, n_groups, bitmaps (lists of open groups; None: a null bitmap)
CASES = {
    "overlaps, the lower id closed / open": ([(6, 1010, 1060, 1), (6, 1040, 1090, 0), (4, 8, 33, 1)], 2, [[1], [0], [0, 1], [], None]),
    "an empty group": ([(3, 101, 109, 0), (3, 105, 130, 2)], 4, [[1, 3], [0], [2], None]),
    "nothing in a group": ([], 3, [[0, 1, 2], None]),
    "whole contigs": ([(r, OFFS[r], OFFS[r] + LENS[r] + 1, r % 3) for r in range(7)], 3, [[0], [1, 2], [], None]),
    "every column its own, 65": ([(5, c, c + 1, 64 - c) for c in range(65)], 65, [[31, 32], [63, 64], list(range(0, 65, 2)), [64], list(range(64))]),
    "word edges, 1023": ([(6, 1000 + c, 1001 + c, (31 + 11 * c) % 1023) for c in range(300)], 1023, [[31], [32, 64], list(range(1, 1023, 2)), [1022], None]),
    "word edges, 33": ([(6, 1000 + c, 1001 + c, c % 33) for c in range(300)], 33, [[32], [31], list(range(32))]),
}


def _record_text(strands, t, n_groups, bits, row):
    words = "-1" if bits is None else f"{len(bits)} " + " ".join("%x" % int(w) for w in bits)
    return (f"record {strands} {len(LENS)} " + " ".join(f"{n} {o}" for n, o in zip(LENS, OFFS)) + f" {n_groups} {len(t)} " + " ".join(" ".join(str(x) for x in k) for k in t)
            + f" {words} " + " ".join("%x" % int(u) for u in row.view(np.uint32)) + "\n")


@pytest.mark.parametrize("strands", [1, 2], ids=["rna_one_strand", "dna_two_strands"])
@pytest.mark.parametrize("name", list(CASES))
def test_python_records_equal_the_headers(programs, name, strands):
    t, n_groups, opens = CASES[name]
    rng = np.random.default_rng(len(name) + strands)
    total = sum(LENS) * strands
    label = G.labels_of(t, n_groups, LENS, OFFS, strands)
    rows = [(1 + rng.integers(0, 4, total) / 4).astype(np.float32), rng.random(total).astype(np.float32)]  # ties everywhere; hardly any
    rows.append(np.where(label == min(1, n_groups - 1), np.float32(np.inf), rows[1]))                         # a label whose every column costs +inf
    text, want = "", []
    for row in rows:
        for o in opens:
            bits = None if o is None else Q.bitmap(n_groups, o)
            text += _record_text(strands, t, n_groups, bits, row)
            want.append(Q.record_of_row(row, label, n_groups, bits, LENS, OFFS, strands))
            first = Q.record_of_row(np.full(total, np.inf, np.float32), label, n_groups, bits, LENS, OFFS, strands)
            want[-1]["first"] = (first["on_col"], first["off_col"])
    for line, w in zip(_ask(programs, text), want):
        tag, a, b, *rest = line.split()
        assert tag == "record" and int(a, 16) == int(np.float32(w["on_score"]).view(np.uint32)) and int(b, 16) == int(np.float32(w["off_score"]).view(np.uint32)), (line, w)
        assert [int(x) for x in rest] == [w["on_rid"], w["on_pos_end"], w["off_rid"], w["off_pos_end"], w["on_strand"], w["off_strand"], w["on_group"], w["off_group"], *w["first"]], (line, w)


def test_oracle_on_a_hand_written_row():
    row = np.array([5, 2, 9, 2, 2, np.inf, 2, 7], np.float32)
    label = np.array([3, 0, 3, 1, 2, 3, 0, 3])
    r = Q.record_of_row(row, label, 3, Q.bitmap(3, [1, 2]), [8], [10], 1)
    assert (r["on_col"], r["on_group"], r["on_pos_end"], r["off_col"], r["off_group"]) == (3, 1, 13, 1, 0)  # equal costs: each class its own lowest column
    r = Q.record_of_row(row, label, 3, None, [8], [10], 1)
    assert (r["on_col"], r["on_group"], r["off_col"], r["off_group"], float(r["off_score"])) == (1, 0, 0, 3, 5.0)
    r = Q.record_of_row(row, label, 3, Q.bitmap(3, []), [8], [10], 1)
    assert (r["on_col"], r["on_group"], r["on_rid"], r["on_strand"], r["off_col"]) == (-1, -1, -1, 0, 1) and np.isposinf(r["on_score"])
    r = Q.record_of_row(row, np.array([0, 0, 0, 0, 0, 1, 1, 1]), 2, Q.bitmap(2, [0]), [8], [10], 1)
    assert (r["off_col"], r["off_group"], float(r["off_score"])) == (6, 1, 2.0)
    r = Q.record_of_row(np.full(8, np.inf, np.float32), label, 3, Q.bitmap(3, [2]), [8], [10], 1)
    assert (r["on_col"], r["off_col"]) == (4, 0)  # +inf everywhere: the lowest column of either class


# ---- open_words and the quota book: header, package and oracle on one script ----
def test_open_words():
    for n, want in ((1, 1), (31, 1), (32, 1), (33, 2), (64, 2), (65, 3), (1023, 32)):
        assert S.open_words(n) == want == Q.open_words(n) == len(S.QuotaBook(n).open)


@pytest.mark.parametrize("n_groups,quota", [(1, 1), (33, 2), (65, 3), (1023, 1), (5, 0)])
def test_quota_books_agree(programs, n_groups, quota):
    rng = np.random.default_rng(n_groups)
    script = [int(g) for g in rng.integers(-1, n_groups + 1, 400)] + [n_groups - 1] * 4 + [0, 31 % n_groups, 32 % n_groups, 64 % n_groups] * 3
    tag, *rest = _ask(programs, f"book {n_groups} {quota} {len(script)} " + " ".join(str(g) for g in script) + "\n")[0].split()
    cut = rest.index("|")
    cut2 = rest.index("|", cut + 1)
    changed, counts, words = [int(x) for x in rest[:cut]], [int(x) for x in rest[cut + 1:cut2]], [int(x, 16) for x in rest[cut2 + 1:]]
    for book in (S.QuotaBook(n_groups, quota), Q.QuotaBook(n_groups, quota)):
        assert [int(book.note_accept(g)) for g in script] == changed
        assert [int(w) for w in book.open] == words and list(getattr(book, "accepted", None) or book.count) == counts
        for g in range(n_groups):
            assert book.is_open(g) == (quota == 0 or counts[g] < quota)
        assert not book.is_open(n_groups) and not book.is_open(-1)
    if quota:
        assert sum(changed) == sum(c >= quota for c in counts) > 0  # a group closes once, with the read that fills its quota
    else:
        assert sum(changed) == 0


# ---- the schedule with a quota: replay.hpp under ASan + UBSan against realtime.Schedule ----
def _python_trace(channels, chunk, quota, names, reads):
    class Source:
        nxt = 0

        def take(self, channel):
            if self.nxt >= len(reads):
                return None
            self.nxt += 1
            return reads[self.nxt - 1][0]

    trace, src = [], Source()
    book = S.QuotaBook(len(names), quota)
    sch = realtime.Schedule(channels, chunk, trace, targets=True)
    sch.set_quota(book, names)
    sch.start(src)
    while sch.busy():
        es = sch.begin_tick()
        open_now = [book.is_open(g) for g in range(len(names))]  # the bitmap the tick's call would carry
        reason = ["E" if first + n >= reads[r][1] else ("R" if end else None) for _, r, first, n, end in es]
        line = [why == "E" and bool(reads[r][3]) for (_, r, _, _, _), why in zip(es, reason)]
        on = [reads[r][2] >= 0 and open_now[reads[r][2]] for _, r, _, _, _ in es]
        on_group = [reads[r][2] if o else -1 for (_, r, _, _, _), o in zip(es, on)]
        action = [realtime.action_of(why, "A" if o else "U") if why else None for why, o in zip(reason, on)]
        sch.end_tick(reason, line, src, action, on_group)
    return trace + ["end tick=%d" % sch.tick + "".join(" %s=%d@%d" % (names[g], book.accepted[g], sch.closed_at[g]) for g in range(len(names)))]


def _cpp_trace(programs, channels, chunk, quota, names, reads):
    text = f"{channels} {chunk} {quota} {len(names)} " + " ".join(names) + f" {len(reads)}\n" + "".join(f"{n} {at} {g} {ln}\n" for n, at, g, ln in reads)
    return _ask(programs, text)


NAMES = ["amp1", "orf1ab", "N"]
#          length, decided once this many samples are out, group (-1: background), has a line
READS = [(1000, 300, 0, 1), (1050, 300, 0, 1), (900, 300, 0, 1),  # three reads of amp1 accepted in ONE tick under quota 2: the group overshoots by one
         (450, 100, 0, 1),                                         # amp1 is closed: unblocked
         (400, 200, 1, 1), (700, 10 ** 9, 1, 1),                   # orf1ab: one accepted, one that proceeds to its end (not credited)
         (300, 100, 1, 0),                                         # accepted without a line: not credited
         (615, 200, -1, 1), (500, 100, 1, 1), (333, 100, 1, 1), (800, 100, 2, 1), (100, 50, 0, 1), (350, 100, 1, 1)]


def test_the_schedule_with_a_quota_in_both_languages(schedule_programs):
    got = _python_trace(3, 100, 2, NAMES, READS)
    assert got == _cpp_trace(schedule_programs, 3, 100, 2, NAMES, READS)
    closes = [ln for ln in got if " close " in ln]
    assert closes[0] == "tick 2 close group=amp1 accepted=2" and len(closes) == 2 and closes[1].endswith("close group=orf1ab accepted=2")
    assert got.index("tick 2 decide ch=1 read=1 reason=E line=1 sent=300") + 1 == got.index(closes[0])  # behind the read that filled the quota
    end = got[-1].split()
    assert end[2] == "amp1=3@2" and end[3].startswith("orf1ab=2@") and end[4] == "N=1@-1"  # amp1 overshoots by its closing tick's third read
    # read 3 (amp1, after the close) is unblocked: no hold, its channel takes the next read in the same tick
    assert not any(" hold " in ln and " read=3 " in ln for ln in got) and not any(" hold " in ln and " read=11 " in ln for ln in got)
    # quota 0 / a quota nobody reaches: no close line, and the trace without them is the quota run's schedule where nothing closed
    free = _python_trace(3, 100, 100, NAMES, READS)
    assert free == _cpp_trace(schedule_programs, 3, 100, 100, NAMES, READS) and not any(" close " in ln for ln in free)
    assert free != [ln for ln in got if " close " not in ln]  # (the closures changed the schedule: this script is no vacuous one)


# ---- the tag, hand-written records, both languages ----
def test_quota_tags_in_both_languages(tag_programs):
    records = [(0, "\\tog:Z:amp1"), (2, "\\tog:Z:N"), (-1, "\\tog:Z:*"), (3, "\\tog:Z:*"), (1, "\\tog:Z:orf1ab")]
    lines = _ask(tag_programs, f"{len(NAMES)} " + " ".join(NAMES) + "\n" + "".join(f"{g}\n" for g, _ in records))
    assert len(lines) == len(records)
    for (g, want), line in zip(records, lines):
        assert line == want == realtime.quota_tags(g, NAMES).replace("\t", "\\t")
    summary = {("group", 1): 4, ("group", 3): 2, "quota": 3, ("closed_at", 1): 17}
    assert realtime.format_group_summary(summary, NAMES) == ("[realtime] group amp1: accepted 0 reads quota=3 closed_at=-\n[realtime] group orf1ab: accepted 4 reads quota=3 closed_at=17\n"
                                                             "[realtime] group N: accepted 0 reads quota=3 closed_at=-\n[realtime] group *: accepted 2 reads\n")
    del summary["quota"]  # without a quota: the lines of --by-name
    assert realtime.format_group_summary(summary, NAMES) == ("[realtime] group amp1: accepted 0 reads\n[realtime] group orf1ab: accepted 4 reads\n[realtime] group N: accepted 0 reads\n"
                                                             "[realtime] group *: accepted 2 reads\n")


# ---- the refusals, each naming the fix, before any session, file or device ----
def test_replay_refuses_quota_before_any_session():
    class NoAligner:
        def session(self, *a, **kw):
            raise AssertionError("a session was opened")

    gt = (np.zeros(1, S.GROUP_TARGET_DTYPE), ["a"])
    plain = np.zeros(1, S.TARGET_DTYPE)
    for kw, word in ((dict(targets=plain, mode=S.ENRICH, margin=0.1, quota=2), "by_name=True"),
                     (dict(quota=2), "by_name=True"),
                     (dict(targets=gt, by_name=True, mode=S.DEPLETE, margin=0.1, quota=2), "mode=ENRICH"),
                     (dict(targets=gt, by_name=True, mode=S.ENRICH, margin=0.1, quota=0), ">= 1"),
                     (dict(targets=gt, by_name=True, mode=S.ENRICH, margin=0.1, quota=-3), ">= 1"),
                     (dict(targets=gt, by_name=True, mode=S.ENRICH, margin=0.1, quota=1.5), ">= 1")):
        with pytest.raises(S.SfaError, match=word):
            list(realtime.replay(NoAligner(), [], 2, 100, 3, 25, 70, 30, 5, **kw))


@pytest.mark.parametrize("extra,word", [(["--quota", "2"], "--by-name"), (["--quota", "2", "--targets", "t.bed", "--enrich", "--margin", "0.1"], "--by-name"),
                                        (["--quota", "2", "--targets", "t.bed", "--by-name", "--deplete", "--margin", "0.1"], "--enrich"),
                                        (["--quota", "0", "--targets", "t.bed", "--by-name", "--enrich", "--margin", "0.1"], ">= 1"),
                                        (["--quota", "-1", "--targets", "t.bed", "--by-name", "--enrich", "--margin", "0.1"], ">= 1"),
                                        (["--quota", "two", "--targets", "t.bed", "--by-name", "--enrich", "--margin", "0.1"], ">= 1")])
def test_binary_refuses_quota_before_any_file_or_device(tmp_path, extra, word):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    model = write_model(tmp_path / "syn.model", 6)
    r = subprocess.run([BIN, "realtime", "--kmer-model", model] + extra + [os.path.join(GOLD, "data", "nCoV-2019.reference.fasta"), str(tmp_path / "no_such.blow5")],
                       capture_output=True, timeout=60)
    err = r.stderr.decode()
    assert r.returncode > 0 and r.stdout == b"", (r.returncode, err)
    assert err.count("[sigfish-amd] ERROR:") == 1 and "--quota" in err and word in err, err
    assert "no_such" not in err and "accelerator" not in err and "t.bed" not in err.replace("--targets FILE.bed", ""), err


def test_symbols_are_bound():
    L = _lib.load()
    assert "sfa_session_open_classes" in _lib.SYMBOLS and L.sfa_session_open_classes is not None
    assert S.OPEN_CLASS_DTYPE.itemsize == S.CLASS_DTYPE.itemsize + 8 == 44 and S.OPEN_CLASS_DTYPE.fields["on_group"][1] == 36
    rec = np.zeros(1, S.OPEN_CLASS_DTYPE)
    rec["cls"]["on_score"], rec["cls"]["off_score"], rec["cls"]["on_rid"], rec["cls"]["off_rid"], rec["cls"]["n_events"], rec["cls"]["valid"] = 10, 60, 0, 0, 100, 1
    assert S.target_decide(rec[0]["cls"], S.ENRICH, 100, 0.5) == "A"  # the cls field is what target_decide takes
