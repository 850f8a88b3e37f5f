"""Contexts from init to destroy, over and over, on every route that owns scratch of its own: the context's buffers, streams and
events free themselves with it (sfa_ctx.hpp), so a cycle that breaks ownership shows here as a wrong row, a failing call or a
fault in a later cycle.  One process, one small batch: three DNA contigs, 13 reads of 0..420 events (one empty) and one of 2 100
events, which takes the row strips."""
import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import synth

pytestmark = pytest.mark.gpu

LENS = [333, 57, 1200]
OPTION_SETS = [{}, {"secondary": 2}, {"column_segments": 4}, {"lds_ckpt": 0}]


@pytest.fixture(scope="module")
def batch(oracle):
    rng = np.random.default_rng(4)
    fw = [rng.normal(size=n).astype(np.float32) for n in LENS]
    rv = [rng.normal(size=n).astype(np.float32) for n in LENS]
    names, seq_lens, offs = [f"c{i}" for i in range(3)], [n + 5 for n in LENS], [0, 0, 0]
    qlens = [int(rng.integers(0, 421)) if i != 5 else 0 for i in range(13)] + [2100]
    q_off = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int64)
    q = rng.normal(size=int(q_off[-1])).astype(np.float32)
    ref = S.RefModel(names, seq_lens, LENS, offs, fw, rv)
    oref = oracle.RefSynth(names, seq_lens, LENS, offs, fw, rv)
    want = oracle.align_batch(q, q_off, oref, 0, threads=4)
    want.setflags(write=False)
    return ref, oref, q, q_off, want


@pytest.fixture(scope="module")
def raw_batch(oracle, batch):
    """Three synthetic raw reads, their query windows by the host stages, and the oracle's rows for those."""
    _, oref, _, _, _ = batch
    reads = synth.make_rna_polya_reads(3, seed=1, kinds=("normal",), body=(3000, 5000))
    raws = [r[5] for r in reads]
    scal = np.array([[r[1], r[2], r[3]] for r in reads], np.float64)
    off = np.concatenate([[0], np.cumsum([len(r) for r in raws])]).astype(np.int64)
    qs = []
    for r, (dig, offset, rng_) in zip(raws, scal):
        meta = dict(digitisation=dig, offset=offset, range=rng_)
        ev = S.detect_events(r, meta, False)
        keep, a, b = S.select_query(ev, r, meta, 50, 250, 0, 0)
        qs.append(ev["mean"][a:b].astype(np.float32) if keep else np.zeros(0, np.float32))
    q_off = np.concatenate([[0], np.cumsum([len(x) for x in qs])]).astype(np.int64)
    want = oracle.align_batch(np.concatenate(qs), q_off, oref, 0, threads=4)
    want.setflags(write=False)
    return np.concatenate(raws), off, scal, want


def _same_rows(got, want):
    assert np.array_equal(got["valid"], want["valid"])
    v = want["valid"] == 1
    assert got[v].tobytes() == want[v].tobytes()


def test_init_align_destroy_cycles(batch, raw_batch):
    """Two cycles under each option set (every call raises unless it returns SFA_OK), event maps and the raw-signal entry point in
    some of them, one cycle on a group context, and a context that is destroyed without ever aligning."""
    ref, _, q, q_off, want = batch
    raw, raw_off, scal, want_raw = raw_batch
    assert want["valid"].any() and want_raw["valid"].any()  # something aligns in both batches
    for si, opts in enumerate(OPTION_SETS):
        for cycle in range(2):
            al = S.Aligner(ref, 0, device=0)
            for k, v in opts.items():
                al.set_option(k, v)
            got = al.align_db(q, q_off)
            _same_rows(got, want)
            if "secondary" in opts:
                sec = al.secondary_rows()
                assert sec.shape == (len(want), 4) and not sec["valid"][:, 2:].any()  # two per read at the most
                assert not sec["valid"][-1].any()  # the long read has none
            if si == 0 and cycle == 1:
                maps = al.event_maps()
                assert len(maps) == len(want)
                assert all(len(m) in (0, r["pos_end"] - r["pos_st"] + 1) for m, r in zip(maps, got) if r["valid"])  # (0: no complete map)
                assert any(len(m) for m in maps)
            if cycle == 0 and si in (1, 3):  # (the raw-signal stages in front of the plain two-pass route and of the LDS-less one)
                rows, info = al.align_raw(raw, raw_off, scal, 50, 250)
                _same_rows(rows, want_raw)
            _same_rows(al.align_db(q, q_off), want)  # the context's scratch is reused, not regrown
            al.close()
    with S.Aligner(ref, 0, devices=[0, 0]) as many:
        assert many.n_devices() == 2
        _same_rows(many.align_db(q, q_off), want)
    S.Aligner(ref, 0, device=0).close()
    S.Aligner(ref, 0, devices=[0, 0]).close()
