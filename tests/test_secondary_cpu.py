"""Secondary mappings without a GPU: the restatement of the reference's candidate list, the PAF/SAM formatting of secondary rows,
and the command line's refusal of --secondary yes beyond 2048 events."""
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd.api import RESULT_DTYPE
from tests.secondary_oracle import top5, secondary_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref(O, rng, lens, rna):
    fw = [(rng.integers(-6, 7, n) / 4).astype(np.float32) for n in lens]
    rv = None if rna else [(rng.integers(-6, 7, n) / 4).astype(np.float32) for n in lens]
    return O.RefSynth([f"c{i}" for i in range(len(lens))], [n + 5 for n in lens], lens, [0] * len(lens), fw, rv)


@pytest.mark.parametrize("flag", [0, S.RNA, S.RNA | S.DTW, S.RNA | S.INV])
def test_restatement_best_is_primary(oracle, flag):
    """aln[4] of the restated list is the oracle's primary, and aln[3] its score2 (ties included: quantised levels)."""
    rng = np.random.default_rng(5 + flag)
    ref = _ref(oracle, rng, [300, 41, 700], bool(flag & S.RNA))
    for qlen in (7, 25, 64, 130):
        q = (rng.integers(-6, 7, qlen) / 4).astype(np.float32)
        aln = top5(oracle, q, ref, flag)
        want = oracle.dtw_single(q, ref, flag)
        assert aln[4][0] == np.float32(want.score) and aln[3][0] == np.float32(want.score2)
        assert aln[4][1] == want.rid and ord(aln[4][4]) == want.strand
        scores = [a[0] for a in aln]
        assert scores == sorted(scores, reverse=True)
        rows = secondary_rows(oracle, q, np.array([0, qlen]), ref, flag)
        assert (rows["mapq"] == 0).all()
        assert rows[0, 0]["score"] == aln[3][0]


def _row(**kw):
    r = np.zeros(1, RESULT_DTYPE)[0]
    for k, v in kw.items():
        r[k] = v
    return r


def test_paf_row_tags():
    r = _row(rid=0, pos_st=100, pos_end=340, score=12.5, score2=13.25, strand=ord("-"), mapq=0, valid=1)
    p = S.paf_row(r, "read1", "chr1", 10, 5000, 249, 9000, 30000)
    s = S.paf_row(r, "read1", "chr1", 10, 5000, 249, 9000, 30000, tp="S")
    assert "\ttp:A:P\t" in p and "\ttp:A:S\t" in s
    assert s.replace("tp:A:S", "tp:A:P") == p
    cols = s.rstrip("\n").split("\t")
    assert cols[11] == "0" and cols[4] == "-" and cols[-1] == "d2:f:13.25"
    last = _row(rid=0, pos_st=100, pos_end=340, score=12.5, score2=np.inf, strand=ord("+"), valid=1)
    assert S.paf_row(last, "r", "c", 0, 1, 249, 2, 3, tp="S").rstrip("\n").endswith("d2:f:inf")


def test_sam_row_flags():
    rng = np.random.default_rng(3)
    y = rng.normal(size=400).astype(np.float32)
    ev = np.zeros(50, S.EVENT_DTYPE)
    ev["start"] = np.arange(50) * 10
    ev["length"] = 10
    ev["mean"] = y[100:150]
    for strand, want in (("+", 256), ("-", 272)):
        r = _row(rid=0, pos_st=100, pos_end=149, score=0.0, score2=1.0, strand=ord(strand), valid=1)
        line = S.sam_row(r, "rd", "chr", ev, 0, 50, y, 0, 0, secondary=True)
        assert int(line.split("\t")[1]) == want
        prim = S.sam_row(r, "rd", "chr", ev, 0, 50, y, 0, 0)
        assert int(prim.split("\t")[1]) == want - 256
        assert line.split("\t")[2:] == prim.split("\t")[2:]


def test_cli_refuses_long_queries():
    exe = os.path.join(ROOT, "sigfish_amd", "bin", "sigfish-amd")
    if not os.path.exists(exe):
        pytest.skip("command line not built")
    p = subprocess.run([exe, "dtw", "-q", "3000", "--secondary", "yes", "/nonexistent.fa", "/nonexistent.blow5"],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode != 0
    assert "--secondary yes supports -q up to 2048" in p.stderr


# ---- the reference's own candidate lists (tests/golden/secondary, tools/make_secondary_golden.py) -------------------------
import importlib.util  # noqa: E402

from tests.secondary_oracle import load_fixture, rows_from_fixture  # noqa: E402
from tests.util import case_names, load_case  # noqa: E402

SEC_CASES = [n for n in case_names() if load_case(n)["query_size"] <= 2048]


def _generator():
    spec = importlib.util.spec_from_file_location("make_secondary_golden", os.path.join(ROOT, "tools", "make_secondary_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fixture_inventory():
    assert len(SEC_CASES) == 17
    for n in SEC_CASES:
        f = load_fixture(n)
        assert f["rid"].shape == (len(load_case(n)["q_off"]) - 1, 5)


@pytest.mark.parametrize("name", SEC_CASES)
def test_fixture_best_is_the_reference_primary(name):
    """aln[4] of each list is the row the compiled reference printed; aln[3] its score2."""
    c, f = load_case(name), load_fixture(name)
    assert np.array_equal(f["score"][:, 4].view(np.uint32), c["score"].view(np.uint32))
    assert np.array_equal(f["score"][:, 3].view(np.uint32), c["score2"].view(np.uint32))
    assert np.array_equal(f["rid"][:, 4], c["rid"]) and np.array_equal(f["strand"][:, 4], c["strand"].astype(np.uint8))
    assert np.array_equal(f["flip_pos_st"][:, 4], c["pos_st"]) and np.array_equal(f["flip_pos_end"][:, 4], c["pos_end"])


@pytest.mark.parametrize("name", SEC_CASES)
def test_fixtures_reproduce_from_reference(oracle, name):
    if oracle.reference_lib() is None:
        pytest.skip("oracle/_ref/libsigfish_ref.so not built (make -C oracle ref)")
    G = _generator()
    f = G.build_case(G._lib(), name)
    z = load_fixture(name)
    for k, v in f.items():
        assert np.array_equal(z[k], v), k


@pytest.mark.parametrize("name", SEC_CASES)
def test_restatement_matches_fixtures(oracle, name):
    c = load_case(name)
    ref = oracle.gen_ref(oracle.read_fasta(c["fasta"]), c["levels"], c["k"], c["flag"], c["query_size"])
    got = secondary_rows(oracle, c["queries"], c["q_off"], ref, c["flag"])
    assert got.tobytes() == rows_from_fixture(load_fixture(name)).tobytes()


def test_eval_reads_secondary_lines(tmp_path):
    """sigfish-amd eval --secondary yes counts a tp:A:S line that matches the truth; --secondary no does not."""
    exe = os.path.join(ROOT, "sigfish_amd", "bin", "sigfish-amd")
    if not os.path.exists(exe):
        pytest.skip("command line not built")
    truth = tmp_path / "truth.paf"
    truth.write_text("r1\t9000\t10\t5000\t+\tchrA\t30000\t1000\t1250\t200\t250\t60\ttp:A:P\n")
    prim = _row(rid=0, pos_st=20000, pos_end=20250, score=10.0, score2=11.0, strand=ord("+"), mapq=7, valid=1)
    sec = _row(rid=0, pos_st=1000, pos_end=1250, score=11.0, score2=12.0, strand=ord("+"), mapq=0, valid=1)
    test = tmp_path / "test.paf"
    test.write_text(S.paf_row(prim, "r1", "chrA", 10, 5000, 249, 9000, 30000) +
                    S.paf_row(sec, "r1", "chrA", 10, 5000, 249, 9000, 30000, tp="S"))

    def ev(opt):
        p = subprocess.run([exe, "eval", "--secondary", opt, str(truth), str(test)], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr
        return p.stdout

    assert "correct\t1 (50.00%)" in ev("yes") and "\n0\t1\t0\n" in ev("yes")
    assert "correct\t0 (0.00%)" in ev("no")
