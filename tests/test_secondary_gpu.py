"""Secondary mappings on the GPU (option "secondary", sfa_secondary_rows) against the restatement of the reference's candidate list
(tests/secondary_oracle.py): every shape class of the fill, several chunks, mixed lengths, the entry points and two shards."""
import numpy as np
import pytest

import sigfish_amd as S
from tests.secondary_oracle import secondary_rows
from tests.util import device_lists

pytestmark = pytest.mark.gpu


def _small_ref(rng, lens, rna, quant=True):
    def arr(n):
        return (rng.integers(-6, 7, n) / 4).astype(np.float32) if quant else rng.normal(size=n).astype(np.float32)
    fw = [arr(n) for n in lens]
    rv = None if rna else [arr(n) for n in lens]
    return S.RefModel([f"c{i}" for i in range(len(lens))], [n + 5 for n in lens], lens,
                      rng.integers(0, 3, len(lens)) if rna else [0] * len(lens), fw, rv)


def _oref(O, ref):
    return O.RefSynth(ref.names, ref.seq_lengths, ref.ref_lengths, ref.st_offset, ref.forward, ref.reverse)


def assert_sec_equal(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got["valid"], want["valid"]), np.argwhere(got["valid"] != want["valid"])[:8]
    v = want["valid"] == 1
    for f in ("rid", "strand", "pos_st", "pos_end", "mapq"):
        assert np.array_equal(got[f][v], want[f][v]), (f, np.argwhere((got[f] != want[f]) & v)[:8])
    assert np.array_equal(got["score"][v].view(np.uint32), want["score"][v].view(np.uint32))
    assert np.array_equal(got["score2"][v].view(np.uint32), want["score2"][v].view(np.uint32))


def _batch(rng, qlens, quant=True):
    q_off = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int64)
    n = int(q_off[-1])
    q = (rng.integers(-6, 7, n) / 4).astype(np.float32) if quant else rng.normal(size=n).astype(np.float32)
    return q, q_off


CASES = {  # (flag, contig lengths, query lengths)
    "dna_r16": (0, [900, 300, 57], [7, 25, 64, 100, 128, 129, 250, 256, 0]),
    "dna_r32": (0, [2600, 700], [257, 300, 512, 513, 1000, 1024, 1025, 2048]),
    "rna": (S.RNA, [1500, 800, 33], [25, 100, 250, 300, 700]),
    "rna_inv": (S.RNA | S.INV, [1200, 400], [64, 250, 600]),
    "rna_std": (S.RNA | S.DTW, [400, 300, 250, 90], [25, 100, 250, 400]),
    "many_contigs": (0, [160] * 40, [25, 100, 250]),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("seed", range(2))
def test_secondaries_vs_restatement(oracle, case, seed):
    flag, lens, ql = CASES[case]
    rng = np.random.default_rng(100 * seed + len(case))
    ref = _small_ref(rng, lens, bool(flag & S.RNA), quant=seed == 0)
    qlens = np.array(list(ql) * 2)
    rng.shuffle(qlens)
    q, q_off = _batch(rng, qlens, quant=seed == 0)
    with S.Aligner(ref, flag) as al:
        prim_off = al.align_db(q, q_off)
        al.set_secondary(4)
        prim = al.align_db(q, q_off)
        sec = al.secondary_rows()
    assert prim.tobytes() == prim_off.tobytes()  # primaries do not move with the option
    assert_sec_equal(sec, secondary_rows(oracle, q, q_off, _oref(oracle, ref), flag))


def test_fewer_secondaries_and_einval(oracle):
    rng = np.random.default_rng(7)
    ref = _small_ref(rng, [700, 300], False)
    q, q_off = _batch(rng, [100, 250, 64])
    with S.Aligner(ref, 0) as al:
        al.align_db(q, q_off)
        with pytest.raises(S.SfaError):
            al.secondary_rows()
        with pytest.raises(S.SfaError):
            al.set_secondary(5)
        al.set_secondary(2)
        al.align_db(q, q_off)
        sec = al.secondary_rows()
    want = secondary_rows(oracle, q, q_off, _oref(oracle, ref), 0, n_sec=2)
    assert_sec_equal(sec, want)
    assert not sec["valid"][:, 2:].any()


def test_long_reads_have_none(oracle):
    """Reads of more than 2048 events take the row strips: no secondaries, their primaries as without the option."""
    rng = np.random.default_rng(9)
    ref = _small_ref(rng, [5000, 900], False)
    qlens = [250, 2100, 64, 3000, 700]
    q, q_off = _batch(rng, qlens)
    with S.Aligner(ref, 0) as al:
        base = al.align_db(q, q_off)
        al.set_secondary(4)
        prim = al.align_db(q, q_off)
        sec = al.secondary_rows()
    assert prim.tobytes() == base.tobytes()
    assert not sec["valid"][[1, 3]].any()
    want = secondary_rows(oracle, q, q_off, _oref(oracle, ref), 0)
    want[[1, 3]] = sec[[1, 3]]
    assert_sec_equal(sec, want)


def test_entry_points(oracle):
    """align_events and submit/wait carry the secondaries like align_db."""
    rng = np.random.default_rng(11)
    ref = _small_ref(rng, [1500, 400], False)
    qlens = np.array([250, 100, 64, 300, 250])
    q, q_off = _batch(rng, qlens)
    want = secondary_rows(oracle, q, q_off, _oref(oracle, ref), 0)
    with S.Aligner(ref, 0) as al:
        al.set_secondary(4)
        al.submit(q, q_off)
        al.wait()
        assert_sec_equal(al.secondary_rows(), want)
        tables = []
        for i in range(len(qlens)):
            ev = np.zeros(int(qlens[i]) + 3, S.EVENT_DTYPE)
            ev["mean"][3:] = q[q_off[i]:q_off[i + 1]]
            tables.append(ev)
        al.align_events(tables, [3] * len(qlens), [3 + int(x) for x in qlens])
        assert_sec_equal(al.secondary_rows(), want)


@pytest.mark.parametrize("devs", device_lists())
def test_two_shards(oracle, devs):
    if len(devs) < 2:
        pytest.skip("one device list entry")
    rng = np.random.default_rng(13)
    ref = _small_ref(rng, [1200, 300], False)
    qlens = rng.choice([25, 64, 250, 300, 600], size=37)
    q, q_off = _batch(rng, qlens)
    with S.Aligner(ref, 0, devices=devs) as al:
        al.set_secondary(4)
        al.align_db(q, q_off)
        sec = al.secondary_rows()
    assert_sec_equal(sec, secondary_rows(oracle, q, q_off, _oref(oracle, ref), 0))


# ---- the reference's own candidate lists on the golden cases (tests/golden/secondary) -------------------------------------
from tests.secondary_oracle import load_fixture, rows_from_fixture  # noqa: E402
from tests.util import case_names, load_case  # noqa: E402

GOLD_CASES = [n for n in case_names() if load_case(n)["query_size"] <= 2048]


@pytest.mark.parametrize("name", GOLD_CASES)
def test_golden_cases(name):
    c = load_case(name)
    ref = S.RefModel.from_fasta(c["fasta"], c["levels"], c["k"], c["flag"], c["query_size"])
    with S.Aligner(ref, c["flag"]) as al:
        al.set_secondary(4)
        prim = al.align_db(c["queries"], c["q_off"])
        sec = al.secondary_rows()
    assert np.array_equal(prim["score"].view(np.uint32), c["score"].view(np.uint32))
    assert_sec_equal(sec, rows_from_fixture(load_fixture(name)))


def _load_raw(path):
    raws, scal = [], []
    for _, meta, raw in S.Blow5File(path):
        raws.append(raw)
        scal.append([meta["digitisation"], meta["offset"], meta["range"]])
    off = np.concatenate([[0], np.cumsum([len(r) for r in raws])]).astype(np.int64)
    return np.concatenate(raws), off, np.array(scal, np.float64)


def _records(path):
    import struct
    b = open(path, "rb").read()
    (hl,) = struct.unpack_from("<I", b, 64)
    p = 68 + hl
    recs = []
    while b[p:p + 5] != b"5WOLB":
        (sz,) = struct.unpack_from("<Q", b, p)
        recs.append(b[p + 8:p + 8 + sz])
        p += 8 + sz
    return b[9] == 1, b[14] == 1, recs


@pytest.mark.parametrize("devices", [None, [0, 0]])
@pytest.mark.parametrize("name", ["dna_default", "rna_default", "rna_dtw_std", "rna_q1000", "rna_q500_pauto"])
def test_golden_raw_and_blow5(name, devices):
    """sfa_align_raw and sfa_align_blow5 carry the secondaries: the valid reads' rows equal the fixture."""
    c = load_case(name)
    ref = S.RefModel.from_fasta(c["fasta"], c["levels"], c["k"], c["flag"], c["query_size"])
    want = rows_from_fixture(load_fixture(name))
    v = np.asarray(c["read_valid"], bool)
    raw, off, scal = _load_raw(c["blow5"])
    rz, ss, recs = _records(c["blow5"])
    rec_off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    kw = {"devices": devices} if devices else {}
    with S.Aligner(ref, c["flag"], **kw) as al:
        al.set_secondary(4)
        rows, _ = al.align_raw(raw, off, scal, c["prefix_size"], c["query_size"])
        sec = al.secondary_rows()
        assert list(rows["valid"] == 1) == list(v)
        assert not sec["valid"][~v].any()
        assert_sec_equal(sec[v], want)
        got = al.align_blow5(b"".join(recs), rec_off, rz, ss, c["prefix_size"], c["query_size"])
        assert got[0].tobytes() == rows.tobytes()
        assert_sec_equal(al.secondary_rows()[v], want)
