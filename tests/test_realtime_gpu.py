"""`sigfish-amd realtime` on the GPU (cli/realtime_main.cpp, sigfish_amd/realtime.py, sfa_session_query_span):
  * with its defaults (normalisation over the whole query, never early) a read's line without the three tags is the line
    `sigfish-amd dtw` prints, i.e. the compiled reference's golden output, whatever the channels and the chunk size;
  * its stdout equals, byte for byte, what the Python replay prints on an Aligner over the same reference, in a run with early,
    full, end-of-read and unmapped decisions, and every early / full row is Aligner.align_db of the host twin's query;
  * Session.query_span equals what Session.events gives; --pace changes no byte of stdout.
No tolerance anywhere."""
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from sigfish_amd import realtime, synth
from tests.realtime_util import BIN, strip_tags, tags, write_model
from tests.test_session_gpu import _small_ref, assert_rows
from tests.test_session_raw_gpu import META, SCALING, Twin, synth_signal
from tests.util import load_case

pytestmark = pytest.mark.gpu

# reads of the fixtures with fewer than p + q events (exempt from the comparison with dtw: never calibrated here, a shortened
# window there).  Every read of both fixtures has at least 830 events, so none is
EXEMPT = {"dna_default": [], "rna_invert": []}


def run_realtime(model, fasta, blow5, *extra):
    r = subprocess.run([BIN, "realtime", "--kmer-model", model, "--verbose", "0", *extra, fasta, blow5], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


@pytest.mark.parametrize("name", ["dna_default", "rna_invert"])
def test_defaults_equal_dtw(name, tmp_path):
    assert os.path.exists(BIN), "build with `make -C sigfish_amd/csrc`"
    c = load_case(name)
    model = write_model(tmp_path / "syn.model", c["k"])
    assert len(EXEMPT[name]) <= 1
    want = sorted((ln + "\n" for ln in c["out_text"].splitlines() if ln.split("\t")[0] not in EXEMPT[name]), key=lambda ln: ln.split("\t")[0])
    for extra in (["--channels", "2", "--chunk-samples", "1600"], ["--channels", "1", "--chunk-samples", "1600"], ["--channels", "8", "--chunk-samples", "1600"],
                  ["--channels", "2", "--chunk-samples", "333"]):
        out = run_realtime(model, c["fasta"], c["blow5"], *[str(a) for a in c["args"]], *extra)
        got = [ln for ln in strip_tags(out) if ln.split("\t")[0] not in EXEMPT[name]]
        assert got == want, (extra, out)
        for ln in out.splitlines():
            ne, ns, why = tags(ln)
            assert ne == c["query_size"] and why == "F" and 0 < ns <= int(ln.split("\t")[1]), ln


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """60 raw reads of 2000 .. 9000 samples over a three-contig DNA reference of 900 / 300 / 57 columns whose second contig
    repeats a stretch of the first: reads from the repeat tie (mapq 0: never early, full at 70 query events), reads from the rest
    of the first contig map alone (early), stalled reads end with 40 .. 65 events (end of read), flat reads have no event
    (unmapped); the random ones fall where they fall."""
    d = tmp_path_factory.mktemp("realtime")
    k = 6
    model = write_model(d / "syn.model", k, synth.kmer_levels(k, 21))
    levels, k_read = S.read_kmer_model(model)  # (as the file's four decimals give them: what the command line reads)
    assert k_read == k
    c0 = synth.random_sequence(905, 1)
    recs = [("c0", c0), ("c1", c0[300:605]), ("c2", synth.random_sequence(62, 3))]
    fasta = str(d / "ref.fa")
    with open(fasta, "w") as f:
        f.write("".join(f">{n}\n{s}\n" for n, s in recs))
    reads = synth.make_dna_raw_reads(recs, levels, k, 60, seed=3, samples=(2000, 9000), kinds=("mapped", "mapped", "random", "mapped", "stalled", "flat"), meta={**META, "sampling_rate": 4000.0})
    blow5 = str(d / "reads.blow5")
    synth.write_blow5(blow5, reads)
    ref = S.RefModel.from_fasta(fasta, levels, k, 0, 70)
    assert list(ref.ref_lengths) == [900, 300, 57]
    return dict(model=model, fasta=fasta, blow5=blow5, ref=ref)


def test_cli_equals_python_replay(synthetic):
    skip, norm, query, min_events, min_mapq, channels, chunk = 3, 25, 70, 30, 5, 7, 800
    out = run_realtime(synthetic["model"], synthetic["fasta"], synthetic["blow5"], "--channels", str(channels), "--chunk-samples", str(chunk), "-p", str(skip), "-q", str(query),
                       "--norm-events", str(norm), "--min-events", str(min_events), "--min-mapq", str(min_mapq))
    reads = list(S.Blow5File(synthetic["blow5"]))
    assert len(reads) == 60 and all(2000 <= len(r[2]) <= 9000 and len(r[2]) % chunk for r in reads)
    ref = synthetic["ref"]
    lines, reasons, unmapped, checks = [], set(), 0, []
    with S.Aligner(ref, 0) as al:
        for tick, ch, index, row, info, span, why in realtime.replay(al, reads, channels, chunk, skip, norm, query, min_events, min_mapq):
            rid, _, raw = reads[index]
            line = realtime.format_line(rid, len(raw), ref.names, ref.seq_lengths, row, info, span, why)
            lines.append(line)
            unmapped += line == ""
            if line:
                reasons.add(why)
                assert tags(line) == (int(info["q_events"]), int(info["n_samples"]), why)
            if line and why in "EF":  # the host twin of the slot, fed the same chunks
                sent = int(info["n_samples"])
                tw = Twin(False, (skip, norm, query))
                for a in range(0, sent, chunk):  # (no read's length is a multiple of the chunk: no empty last chunk to account for)
                    tw.feed(raw[a:a + chunk], a + chunk > len(raw))
                q = tw.query_so_far()
                assert q is not None and len(q) == int(info["q_events"]), (rid, why)
                checks.append((q, row))
        assert out == "".join(lines)
        assert reasons == {"E", "F", "R"} and unmapped >= 1, (reasons, unmapped)  # (about this test's own inputs)
        qs = [q for q, _ in checks]
        want = al.align_db(np.concatenate(qs), np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.int64))
        assert_rows(np.array([row for _, row in checks], S.RESULT_DTYPE), want, True, "early and full rows against align_db")  # (bitwise, field by field)


def test_query_span():
    rng = np.random.default_rng(12)
    ref = _small_ref(rng, [400, 300], False)
    n_slots, skip, norm, query = 40, 3, 25, 70
    sigs = [synth_signal(rng, int(rng.integers(100, 900))) for _ in range(n_slots)]

    def check(se, slots):
        a, b = se.query_span(slots)
        q = se.lengths(slots)
        for i, sl in enumerate(slots):
            ev = se.events(int(sl))
            if q[i] == 0:
                assert (a[i], b[i]) == (0, 0), sl
            else:
                last = ev[skip + int(q[i]) - 1]
                assert a[i] == ev["start"][skip] and b[i] == int(last["start"]) + int(last["length"]), sl
        return q

    with S.Aligner(ref, 0) as al, al.session(n_slots) as se:
        with pytest.raises(S.SfaError):  # not a raw-mode session
            se.query_span([0])
        se.configure_raw(skip, norm, query)
        assert check(se, np.arange(n_slots)).sum() == 0  # nothing sent yet: 0 / 0
        at = [0] * n_slots
        seen_cal = seen_not = seen_full = False
        for call in range(4):  # mixed calls: a changing subset of slots, ragged chunks, some reads ending
            named = [sl for sl in range(n_slots) if (sl + call) % 3 and at[sl] < len(sigs[sl])]
            chunks = []
            for sl in named:
                n = min(len(sigs[sl]) - at[sl], int(rng.integers(40, 300)))
                chunks.append(sigs[sl][at[sl]:at[sl] + n])
                at[sl] += n
            raw_off = np.concatenate([[0], np.cumsum([len(x) for x in chunks])]).astype(np.int64)
            _, info = se.extend_raw(named, np.concatenate(chunks), raw_off, [SCALING] * len(named), [at[sl] == len(sigs[sl]) for sl in named])
            order = rng.permutation(n_slots)  # every slot, named in this call or not, in any order
            q = check(se, order)
            seen_cal |= bool((q > 0).any())
            seen_not |= bool((q == 0).any())
            seen_full |= bool((q == query).any())
            if call == 1:  # a reset slot has no span, whatever its table still holds
                se.reset([5, 6])
                at[5] = at[6] = 0
                a, b = se.query_span([5, 6, 7])
                assert list(a[:2]) == [0, 0] and list(b[:2]) == [0, 0]
        assert seen_cal and seen_not and seen_full
        for bad in ([n_slots], [-1]):
            with pytest.raises(S.SfaError):
                se.query_span(bad)
        a, b = se.query_span([])
        assert len(a) == 0 and len(b) == 0


def test_pace_does_not_change_stdout(tmp_path):
    c = load_case("dna_default")
    model = write_model(tmp_path / "syn.model", c["k"])
    six = str(tmp_path / "six.blow5")
    reads = [(rid, m["digitisation"], m["offset"], m["range"], m["sampling_rate"], raw) for rid, m, raw in S.Blow5File(c["blow5"])]
    synth.write_blow5(six, (reads + reads[:1]))
    outs = [run_realtime(model, c["fasta"], six, "--channels", "3", "--chunk-samples", "1600", "--pace", pace) for pace in ("no", "yes")]
    assert outs[0] == outs[1] and len(outs[0].splitlines()) == 6
