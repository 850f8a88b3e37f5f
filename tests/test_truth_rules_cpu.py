"""The host rules of `realtime --truth` without a GPU: the stand-alone program tests/c/truth_rules.cpp, built from
sigfish_amd/csrc/truth_rules.hpp alone with -Wall -Werror and once more under ASan + UBSan (its selftest: overlap by one base at
either end, touching intervals, containment against edge, two groups, a `*` read, an absent read, every refusal of the parser with
its line number, the account's sums, an all-N account in which nothing is divided); the header's parser against api.read_truth on
the same files -- what they accept and the line they refuse; the account's `truth:` lines of both languages on random lists."""
import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime
from tests.test_session_groups_cpu import _ask, _programs

NAMES = ["chrA", "chrB", "c.3"]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return _programs(tmp_path_factory.mktemp("truth_rules"), "truth_rules.cpp", "truth_rules")


def test_selftest_plain_and_under_sanitizers(programs):
    line = _ask(programs, "selftest\n")[-1].split()
    assert line[:2] == ["selftest", "ok"] and int(line[2]) > 9000


def paf(rid, contig, b, e):
    return f"{rid}\t1000\t0\t1000\t+\t{contig}\t5000\t{b}\t{e}\t10\t10\t60\n"


GOOD = paf("r0", "chrA", 100, 200) + "\n" + paf("r1", "*", 0, 0) + paf("r2", "c.3", 0, 2147483647) + "r3\t1\t0\t1\t-\tchrB\t9\t7\t9\r\n" + paf("r 4", "*", "x", "")


def test_both_parsers_read_the_same_table(programs, tmp_path):
    path = tmp_path / "good.paf"
    path.write_bytes(GOOD.encode())
    got = S.read_truth(str(path), NAMES)
    assert got == {"r0": (0, 100, 200), "r1": (-1, 0, 0), "r2": (2, 0, 2147483647), "r3": (1, 7, 9), "r 4": (-1, 0, 0)}
    lines = _ask(programs, f"parse {len(NAMES)} {' '.join(NAMES)} {path} r0 r1 r2 r3 absent\n")
    assert lines[0] == "ok 5"
    for ln in lines[1:]:
        rid, *rest = ln.split()
        assert (rest == ["-"] and rid not in got) or tuple(int(x) for x in rest) == got[rid], ln
    assert lines[-1] == "absent -"


REFUSALS = {
    "eight columns": (paf("a", "chrA", 1, 2) + "b\t1\t0\t1\t+\tchrA\t9\t7\n", 2, "9 tab-separated columns"),
    "blanks are no tabs": ("b c d e f g h i j\n", 1, "9 tab-separated columns"),
    "begin is no number": (paf("a", "chrA", 1, 2) + "\n\n" + paf("b", "chrA", "x", 9), 4, "must be integers"),
    "end is a fraction": (paf("b", "chrA", 1, "9.5"), 1, "must be integers"),
    "a negative begin": (paf("b", "chrA", -1, 9), 1, "must be integers"),
    "an empty end": (paf("b", "chrA", 1, ""), 1, "must be integers"),
    "a signed end": (paf("b", "chrA", 1, "+9"), 1, "must be integers"),
    "beyond 2^31 - 1": (paf("a", "chrA", 1, 2) + paf("b", "chrA", 1, 2147483648), 2, "must be integers"),
    "end == begin": (paf("a", "chrA", 1, 2) + paf("b", "chrA", 9, 9), 2, "[9, 9) is empty"),
    "end < begin": (paf("b", "chrA", 9, 8), 1, "[9, 8) is empty"),
    "an unknown contig": (paf("a", "chrA", 1, 2) + paf("b", "chrC", 1, 2), 2, "'chrC' is not in the reference"),
    "a read id twice": (paf("a", "chrA", 1, 2) + paf("b", "chrB", 1, 2) + paf("a", "chrB", 5, 6), 3, "'a' appears twice"),
    "a read id twice, once nowhere": (paf("a", "chrA", 1, 2) + paf("a", "*", 0, 0), 2, "'a' appears twice"),
    "no read id": (paf("", "chrA", 1, 2), 1, "read id"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_both_parsers_refuse_with_file_and_line(programs, tmp_path, name):
    text, line, word = REFUSALS[name]
    path = tmp_path / "bad.paf"
    path.write_bytes(text.encode())
    got = _ask(programs, f"parse {len(NAMES)} {' '.join(NAMES)} {path}\n")
    assert len(got) == 1 and got[0].startswith(f"error {path}:{line}: ") and word in got[0], got
    with pytest.raises(S.SfaError) as e:
        S.read_truth(str(path), NAMES)
    assert f"{path}:{line}: " in str(e.value) and word in str(e.value), e.value


def test_an_empty_file_is_a_table_without_reads(programs, tmp_path):
    path = tmp_path / "empty.paf"
    path.write_bytes(b"\n\r\n")
    assert S.read_truth(str(path), NAMES) == {} and _ask(programs, f"parse 3 {' '.join(NAMES)} {path} r0\n") == ["ok 0", "r0 -"]


@pytest.mark.parametrize("kind", ["mixed", "all N", "only O", "no T in the file", "empty"])
def test_the_account_prints_the_same_lines_in_both_languages(programs, kind):
    rng = np.random.default_rng(len(kind))
    n = 0 if kind == "empty" else 200
    classes = {"mixed": "TON", "all N": "N", "only O": "O", "no T in the file": "ON", "empty": "T"}[kind]
    acc = realtime.new_truth_account(kind != "only O")
    text, marks = "", []
    for _ in range(n):
        tt, action, tv = (str(rng.choice(list(s))) for s in (classes, "AUP", "CWN"))
        edge, sent, held, length = int(rng.integers(0, 2)), int(rng.integers(0, 10 ** 9)), int(rng.integers(0, 10 ** 9)), int(rng.integers(1, 10 ** 10))
        realtime.note_truth(acc, tt, edge, action, tv, sent, held, length)
        text += f" {tt} {edge} {action} {tv} {sent} {held} {length}"
    if acc["groups"] is not None:
        marks = [str(v) for v in rng.choice(list("CWN"), n // 2)]
        for v in marks:
            acc["groups"][v] += 1
    got = _ask(programs, f"account {int(acc['groups'] is not None)} {n}{text} {len(marks)} {' '.join(marks)}\n")
    assert "".join(ln + "\n" for ln in got) == realtime.format_truth_summary(acc)
    assert sum(acc[c]["reads"] for c in "TON") == n == sum(acc[c][a] for c in "TON" for a in "AUP") == sum(acc[c][v] for c in "TON" for v in "CWN")
    if kind in ("all N", "only O", "no T in the file", "empty"):
        assert got[-1].endswith("enrichment by signal -")  # the ratio is not formed
    else:
        (s_on, s_all), (f_on, f_all), ratio = realtime.truth_enrichment(acc)
        assert got[-1].endswith("enrichment by signal %.4f" % ratio) and abs(ratio - (s_on / s_all) / (f_on / f_all)) < 1e-9 * ratio
