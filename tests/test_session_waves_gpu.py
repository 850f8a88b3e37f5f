"""Session sweeps on the GPU, every wave shape: one call that holds full waves, shared waves of chunks of different lengths
(g0 > 0 up to g0 == lq) and lone chunks of all six class shapes, as first chunks and below carried rows (build_matrix,
tests/session_waves.py; its coverage is asserted without a GPU in test_session_waves_cpu.py), over contigs of every length
modulo 4 including 1, 2 and 3 columns.  Checked after every call: the rows against oracle.align_batch, the planner's task and
launch counts against the restated grouping rule, and the CARRIED ROW of every (slot, contig, strand) -- every cost as a uint32
view and every start column against oracle.last_row, which backtracks every column on its own.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import _lib
from tests import session_waves as W
from tests.test_session_gpu import _events, _small_ref, assert_rows

pytestmark = pytest.mark.gpu

REFS = {  # (flag, contig lengths): every residue modulo 4, contigs shorter than a block and than most chunks, one with several windows
    "dna": (0, [1, 2, 3, 5, 62, 63, 64, 301, 1030]),
    "rna_inv": (S.RNA | S.INV, [3, 63, 301, 1030]),  # non-zero ref_st_offset
}


class Want:
    """The oracle's side for one (reference, data): align_batch rows and last rows per prefix, every distinct prefix once (shared
    by the runs with and without start columns)."""

    def __init__(self, O, refname, quant, seed):
        self.O, (self.flag, lens) = O, REFS[refname]
        self.rng = np.random.default_rng(seed)
        self.ref = _small_ref(self.rng, lens, bool(self.flag & S.RNA), quant)
        self.oref = O.RefSynth(self.ref.names, self.ref.seq_lengths, self.ref.ref_lengths, self.ref.st_offset, self.ref.forward, self.ref.reverse)
        self.quant, self._rows, self._last, self.data = quant, {}, {}, {}

    def events(self, slot, n):
        """The slot's events, the same on every run: a longer request extends the shorter one."""
        if slot not in self.data:
            self.data[slot] = _events(np.random.default_rng([slot, self.quant, 5]), 8192, self.quant)
        assert n <= 8192
        return self.data[slot][:n]

    def rows(self, prefixes):
        out = np.zeros(len(prefixes), S.RESULT_DTYPE)
        for i, p in enumerate(prefixes):
            key = p.tobytes()
            if key not in self._rows:
                self._rows[key] = self.O.align_batch(p, np.array([0, len(p)], np.int64), self.oref, self.flag)[0].copy()
            out[i] = self._rows[key]
        return out

    def last(self, prefix):
        key = prefix.tobytes()
        if key not in self._last:
            self._last[key] = self.O.last_rows(prefix, self.oref, self.flag)
        return self._last[key]


_WANT = {}


def _want(O, refname, quant, tag):
    key = (refname, quant, tag)
    if key not in _WANT:
        _WANT[key] = Want(O, refname, quant, [len(refname), quant, len(tag)])
    return _WANT[key]


def assert_carried(se, want, slot, n_events, starts, where):
    """The carried row of every job of `slot` equals the oracle's last row of its first n_events events: costs as bits, start
    columns as integers, at every column."""
    for contig, strand, wc, ws in want.last(want.events(slot, n_events)):
        gc, gs = se.row(slot, contig, strand)
        assert len(gc) == len(wc)
        if starts:
            assert gs.dtype == np.int32 and len(gs) == len(wc)
        else:
            assert gs is None
        bad_c = np.flatnonzero(gc.view(np.uint32) != wc.view(np.uint32))
        bad_s = np.flatnonzero(gs != ws) if starts else bad_c[:0]
        if len(bad_c) or len(bad_s):
            j = int(min(list(bad_c[:1]) + list(bad_s[:1])))
            what = "cost" if j in bad_c else "start column"
            got, exp = (gc[j], wc[j]) if what == "cost" else (gs[j], ws[j])
            raise AssertionError(f"carried row, slot {slot} ({n_events} events), contig {contig} '{strand}', rlen {len(wc)}, column {j}: {what} "
                                 f"got {got!r} want {exp!r} ({len(bad_c)} costs, {len(bad_s)} starts differ; first columns "
                                 f"{bad_c[:8].tolist()} / {bad_s[:8].tolist()}); written by: {where}")


def _row_bytes(se, want, slot, starts):
    out = b""
    for contig in range(len(want.ref.ref_lengths)):
        for strand in ("+",) if want.flag & S.RNA else ("+", "-"):
            c, s = se.row(slot, contig, strand)
            out += c.tobytes() + (s.tobytes() if starts else b"")
    return out


class Run:
    """One session, the events every slot holds, and the checks after every call."""

    def __init__(self, al, se, want, starts):
        self.al, self.se, self.want, self.starts, self.held = al, se, want, starts, {}
        self.n_jobs = len(want.ref.ref_lengths) * (1 if want.flag & S.RNA else 2)

    def call(self, chunks, what):
        """chunks: [(slot, events)] of one extend.  Rows, task and launch counts, carried rows of every named slot."""
        w, held = self.want, self.held
        parts = [w.events(s, held.get(s, 0) + n)[held.get(s, 0):] for s, n in chunks]
        ev_off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
        launches = W.plan_call(chunks, held)
        got = self.se.extend([s for s, n in chunks], np.concatenate(parts), ev_off)
        pr = self.al.profile()
        assert (pr["n_tasks"], pr["fill_launches"]) == W.counts(launches, self.n_jobs), (what, pr["n_tasks"], pr["fill_launches"])
        for s, n in chunks:
            held[s] = held.get(s, 0) + n
        slots = [s for s, n in chunks]
        assert list(self.se.lengths(slots)) == [held[s] for s in slots]
        assert_rows(got, w.rows([w.events(s, held[s]) for s in slots]), self.starts, what)
        for s, n in chunks:
            where = [g.describe(s) for gs in launches for g in gs if s in [p.slot for p in g.pieces]]
            assert_carried(self.se, w, s, held[s], self.starts, f"{what}; {where[-1] if where else 'an earlier call'}")


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "nostart"])
@pytest.mark.parametrize("kind", ["first", "carried"])
@pytest.mark.parametrize("quant", [True, False], ids=["ties", "normal"])
@pytest.mark.parametrize("refname", list(REFS))
def test_wave_matrix(oracle, refname, quant, kind, starts):
    want = _want(oracle, refname, quant, kind)
    m = W.build_matrix(kind)
    idle = (W.ZERO_SLOT, W.UNNAMED_SLOT)
    with S.Aligner(want.ref, want.flag) as al, al.session(W.N_SLOTS, starts=starts) as se:
        run = Run(al, se, want, starts)
        run.call([(s, W.IDLE_EVENTS[s]) for s in idle], "the idle slots' events")
        if kind == "carried":
            run.call(list(zip(m.slots, m.prefix)), "the prefixes")
        for name, lens in (("matrix", m.lens), ("continuation", W.continuation_lengths(m))):
            before = [_row_bytes(se, want, s, starts) for s in idle]
            chunks = list(zip(m.slots, lens))
            chunks.insert(len(chunks) // 2, (W.ZERO_SLOT, 0))
            run.call(chunks, f"{name} call ({kind})")
            # a named slot with a zero-length chunk and a slot that was not named: their carried rows are untouched
            assert [_row_bytes(se, want, s, starts) for s in idle] == before, name
        if not starts:  # the C entry refuses to hand out start columns the session does not carry
            buf_c, buf_s = np.zeros(2048, np.float32), np.zeros(2048, np.int32)
            rc = se._L.sfa_session_row(se._h, m.slots[0], 0, ord("+"), buf_c.ctypes.data_as(_lib.f32p), buf_s.ctypes.data_as(_lib.i32p))
            assert rc == -1 and b"SFA_SESSION_NO_START" in se._L.sfa_last_error()


@pytest.mark.parametrize("starts", [True, False], ids=["starts", "nostart"])
def test_launch_split(oracle, starts):
    """Chunks of 2049 and 4097 events: pieces in two and three launches of one call, the later pieces below the row the earlier
    ones left."""
    want = _want(oracle, "dna", True, "split")
    with S.Aligner(want.ref, want.flag) as al, al.session(W.N_SLOTS, starts=starts) as se:
        Run(al, se, want, starts).call(list(W.SPLIT), "launch split")
        assert al.profile()["fill_launches"] == 3


def test_chunking_leaves_the_same_rows():
    """Fed whole or in random cuts, a read leaves the same row and the same carried rows, and the row is align_db's."""
    rng = np.random.default_rng(99)
    flag, lens = REFS["dna"]
    ref = _small_ref(rng, lens, False, False)
    n = 24
    qlens = rng.integers(300, 2201, n)
    q_off = np.concatenate([[0], np.cumsum(qlens)]).astype(np.int64)
    q = _events(rng, int(q_off[-1]), False)
    slots = [int(s) for s in rng.permutation(40)[:n]]
    with S.Aligner(ref, flag) as al:
        plain = al.align_db(q, q_off)
        with al.session(40) as whole, al.session(40) as cut:
            assert_rows(whole.extend(slots, q, q_off), plain, True, "whole")
            cuts = [np.concatenate([[0], np.sort(rng.choice(np.arange(1, l), size=int(rng.integers(1, 6)), replace=False)), [l]]) for l in qlens]
            last = np.zeros(n, S.RESULT_DTYPE)
            for c in range(max(len(x) for x in cuts) - 1):
                idx = [i for i in range(n) if c + 1 < len(cuts[i])]
                parts = [q[q_off[i] + cuts[i][c]:q_off[i] + cuts[i][c + 1]] for i in idx]
                got = cut.extend([slots[i] for i in idx], np.concatenate(parts), np.concatenate([[0], np.cumsum([len(x) for x in parts])]))
                last[idx] = got
            assert_rows(last, plain, True, "in cuts")
            for sl in slots:
                for contig in range(len(lens)):
                    for strand in "+-":
                        a, b = whole.row(sl, contig, strand), cut.row(sl, contig, strand)
                        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (sl, contig, strand)


def test_row_refusals():
    rng = np.random.default_rng(12)
    dna = _small_ref(rng, [40, 7], False)
    rna = _small_ref(rng, [40, 7], True)
    ev = _events(rng, 30, True)
    L = _lib.load()
    cost, start = np.zeros(64, np.float32), np.zeros(64, np.int32)
    pc, ps = cost.ctypes.data_as(_lib.f32p), start.ctypes.data_as(_lib.i32p)
    assert L.sfa_session_row(None, 0, 0, ord("+"), pc, ps) == -1
    with S.Aligner(dna, 0) as al, al.session(4) as se, al.session(4, starts=False) as nost:
        se.extend([1], ev, [0, 30])
        nost.extend([1], ev, [0, 30])
        assert L.sfa_session_row(se._h, 1, 1, ord("-"), pc, ps) == 7 and L.sfa_session_row(se._h, 1, 0, ord("+"), pc, None) == 40
        assert L.sfa_session_row(se._h, 1, 0, ord("+"), None, ps) == -1        # null cost
        for slot, contig, strand in ((4, 0, "+"), (-1, 0, "+"), (1, 2, "+"), (1, -1, "+"), (1, 0, "x"), (1, 0, 0)):
            with pytest.raises(S.SfaError):
                se.row(slot, contig, strand)
        with pytest.raises(S.SfaError):
            se.row(0, 0, "+")                                                  # a slot without events
        assert L.sfa_session_row(nost._h, 1, 0, ord("+"), pc, ps) == -1        # no start columns carried
        c, s = nost.row(1, 0, "+")
        assert s is None and c.tobytes() == se.row(1, 0, "+")[0].tobytes()
        bad = ev.copy()
        bad[3] = np.nan
        assert se.extend([2, 3], np.concatenate([ev, bad]), [0, 30, 60])["valid"].tolist() == [1, 0]
        with pytest.raises(S.SfaError):
            se.row(3, 0, "+")                                                  # poisoned
        se.reset([1])
        with pytest.raises(S.SfaError):
            se.row(1, 0, "+")                                                  # reset: no events again
        assert len(se.row(2, 1, "-")[0]) == 7
    with S.Aligner(rna, S.RNA | S.INV) as al, al.session(2) as se:
        se.extend([0], ev, [0, 30])
        assert len(se.row(0, 1, "+")[0]) == 7
        with pytest.raises(S.SfaError):
            se.row(0, 0, "-")                                                  # RNA has no '-'
