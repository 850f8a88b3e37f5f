"""ev_stream_kernel (sigfish_amd/csrc/events_stream.hpp) on crafted signals and cuts: the reads of tests/events_edge_cases.py go
through raw-signal sessions cut by the schedules of tests/stream_cuts.py, one slot per (read, schedule) pair, several hundred slots
in the same extend_raw calls (tests/stream_edges.py lays them out; tests/test_stream_edges_cpu.py shows without a GPU that the
layout has the shapes the kernel's edges need).  After EVERY call each named slot's device table is the prefix of the batch
detector's table (events_edge_cases.host_a()) that the host twin fed the same chunks has emitted, and its count, status bits and
normalisation words are what the header documents.  Every comparison is bit for bit; there is no tolerance anywhere."""
import numpy as np
import pytest

import sigfish_amd as S
from tests import events_edge_cases as E
from tests import stream_edges as P
from tests.test_session_gpu import _small_ref
from tests.test_session_raw_gpu import norm_stats, same_events

pytestmark = pytest.mark.gpu

CHEM = [pytest.param(False, id="dna"), pytest.param(True, id="rna")]
SHAPES = [pytest.param("a", id="holds_2048_events"), pytest.param("b", id="small_cap")]
# the content cases that are non-finite or have no spread.  The rule (sfa_session_extend_raw in sigfish_amd.h): a slot calibrates
# once final event skip + norm - 1 exists, and is poisoned by a frozen sd that is zero or not finite or by a query event that is
# not finite.  Sums of squares that overflow give statistics that are infinite or NaN, against which few comparisons of the peak
# picker hold; a signal without spread has both statistics at zero.  Neither ever cuts NORM events, so such a slot is never
# calibrated and never poisoned, its normalisation words stay 0, and what its table holds (nothing, two events of the finish step's
# walk, a dozen events with infinite means) is the batch detector's.  The range_inf reads of the table have a scaling that is not
# finite itself: extend_raw refuses them (test_a_scaling_that_is_not_finite_is_refused), the overflowing read stands in for them.
NEVER_CALIBRATED = (P.OVERFLOW[0], "zero_pa", "constant")


def _bits(x):
    return np.asarray(x, np.float32).reshape(1).view(np.uint32)[0]


def _normalisation(ev, skip, norm):
    """-> None before calibration, or (mean, sd, poisoned) by the rule above"""
    if len(ev) < skip + norm:
        return None
    mean, sd = norm_stats(ev["mean"][skip:skip + norm])
    with np.errstate(all="ignore"):
        q = ((ev["mean"][skip:] - mean) / sd).astype(np.float32)
    return mean, sd, bool(not sd > 0 or not np.isfinite(sd) or not np.isfinite(q).all())


@pytest.mark.parametrize("which", SHAPES)
@pytest.mark.parametrize("rna", CHEM)
def test_tables_bits_and_normalisation_after_every_call(rna, which):
    shape = P.SHAPE_A if which == "a" else P.shape_b(rna)
    skip, norm, query = shape
    cap = skip + query
    batch = P.reads(rna)
    prs, slots, _, n_slots = P.layout(rna, shape)
    calls = P.calls_of(rna, shape)
    twins = [S.EventStream(P.meta(batch[p.read][2]), rna) for p in prs]
    count, ended, was_full = [0] * len(prs), [False] * len(prs), [False] * len(prs)
    seen = dict(full=0, ended=0, calibrated=0, fed_when_full=0, named_when_ended=0, end_without_samples=0, never=0)
    ref = _small_ref(np.random.default_rng(7), [300], rna, quant=False)
    with S.Aligner(ref, (S.RNA | S.INV) if rna else 0) as al, al.session(n_slots) as se:
        se.configure_raw(*shape)
        for c, call in enumerate(calls):
            chunks = [batch[prs[k].read][1][lo:hi] for k, lo, hi, _ in call]
            raw_off = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
            named = [slots[k] for k, _, _, _ in call]
            got, info = se.extend_raw(named, np.concatenate(chunks), raw_off, [batch[prs[k].read][2] for k, _, _, _ in call], [e for _, _, _, e in call])
            for i, (k, lo, hi, end) in enumerate(call):
                p = prs[k]
                what = (f"call {c}", p.name, p.sched, f"entry {i}", f"slot {named[i]}", f"samples {lo}:{hi}", "end" * end)
                seen["fed_when_full"] += was_full[k] and hi > lo
                seen["named_when_ended"] += ended[k]
                seen["end_without_samples"] += end and hi == lo
                if not ended[k]:
                    count[k] += len(twins[k].push(chunks[i]))
                    if end:
                        count[k] += len(twins[k].finish())
                        ended[k] = True
                want = P.expected(rna, p.read, count[k], cap)
                same_events(se.events(named[i]), want, what)
                assert info["n_events"][i] == len(want) and info["n_samples"][i] == hi, what
                st = int(info["status"][i])
                assert bool(st & S.RAW_ENDED) == ended[k], (what, st)
                assert bool(st & S.RAW_FULL) == (len(want) == cap), (what, st)
                was_full[k] = len(want) == cap
                nz = _normalisation(want, skip, norm)
                if p.name.startswith(NEVER_CALIBRATED):
                    assert nz is None, what
                    seen["never"] += 1
                assert bool(st & S.RAW_CALIBRATED) == (nz is not None) and bool(st & S.RAW_POISONED) == (nz is not None and nz[2]), (what, st)
                if nz is None:
                    assert _bits(info["norm_mean"][i]) == 0 and _bits(info["norm_sd"][i]) == 0 and info["q_events"][i] == 0, what
                else:
                    assert not nz[2], what   # (no read of the table with NORM events is poisoned)
                    assert _bits(info["norm_mean"][i]) == _bits(nz[0]) and _bits(info["norm_sd"][i]) == _bits(nz[1]), what
        # ... and at the end every slot still holds its table
        for k, p in enumerate(prs):
            want = P.expected(rna, p.read, count[k], cap)
            same_events(se.events(slots[k]), want, ("at the end", p.name, p.sched))
            seen["full"] += len(want) == cap
            seen["ended"] += ended[k]
            seen["calibrated"] += len(want) >= skip + norm
    # the session went through every state the assertions above are about
    assert seen["ended"] == len(prs) and seen["named_when_ended"] == len(prs) and seen["calibrated"] > len(prs) // 2, seen
    assert seen["full"] >= 9 and seen["fed_when_full"] >= 6 and seen["end_without_samples"] >= 20 and seen["never"] >= 100, seen
    if which == "b":
        kinds = {P.fill_kind(rna, p.read, p.calls, cap) for p in prs}
        assert kinds >= {"mid", "last", "end", "short"}, kinds


@pytest.mark.parametrize("rna", CHEM)
def test_a_scaling_that_is_not_finite_is_refused(rna):
    """... for the whole call, which changes nothing: the other slot of the call goes on where it was"""
    batch, want = P.reads(rna), P.tables(rna)
    names = [b[0] for b in batch]
    _, bad, bad_sc = batch[names.index("range_inf_1600")]
    k = names.index("len_97")
    _, ok, ok_sc = batch[k]
    ref = _small_ref(np.random.default_rng(7), [300], rna, quant=False)
    with S.Aligner(ref, (S.RNA | S.INV) if rna else 0) as al, al.session(3) as se:
        se.configure_raw(*P.SHAPE_A)
        se.extend_raw([2], ok[:50], [0, 50], [ok_sc])
        with pytest.raises(S.SfaError, match="not finite"):
            se.extend_raw([2, 0], np.concatenate([ok[50:], bad]), [0, len(ok) - 50, len(ok) - 50 + len(bad)], [ok_sc, bad_sc], [True, True])
        got, info = se.extend_raw([2, 0], ok[50:], [0, len(ok) - 50, len(ok) - 50], [ok_sc, E.SCALE], [True, False])
        same_events(se.events(2), want[k], "the slot named beside the refused one")
        assert list(info["n_samples"]) == [len(ok), 0] and list(info["n_events"]) == [len(want[k]), 0] and len(se.events(0)) == 0
        assert info["status"][0] == S.RAW_ENDED and info["status"][1] == 0
