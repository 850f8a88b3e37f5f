"""The command line with --secondary yes on the golden cases: every primary line is the reference's own (tests/golden/cases/*.out)
and behind it come exactly the secondary lines formatted from the reference's candidate list (tests/golden/secondary/, made by
tools/make_secondary_golden.py) -- PAF through paf_row(tp="S"), SAM through sam_row(secondary=True) on the device's query events
-- on every route: device events, host events, records parsed on the GPU, two ranks."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from tests.secondary_oracle import load_fixture, rows_from_fixture
from tests.util import GOLD, ROOT, case_names, load_case

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "sigfish_amd", "bin", "sigfish-amd")
CASES = [n for n in case_names() if load_case(n)["query_size"] <= 2048]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp("models")
    out = {}
    for k in (5, 6):
        lv = np.fromfile(os.path.join(GOLD, "models", f"syn{k}.f32"), np.float32)
        p = d / f"syn{k}.model"
        with open(p, "w") as f:
            f.write(f"#k\t{k}\nkmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\n")
            for kmer, v in zip(itertools.product("ACGT", repeat=k), lv):
                f.write("%s\t%.4f\t1.5000\t1.0\t1.0\n" % ("".join(kmer), v))
        out[k] = str(p)
    return out


def _run(c, models, extra):
    args = [str(a) for a in c["args"]]
    cmd = [BIN, "dtw", "--kmer-model", models[c["k"]], "--verbose", "0", *extra, *args, c["fasta"], c["blow5"]]
    r = subprocess.run(cmd, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


def _load_raw(path):
    raws, scal = [], []
    for _, meta, raw in S.Blow5File(path):
        raws.append(raw)
        scal.append([meta["digitisation"], meta["offset"], meta["range"]])
    off = np.concatenate([[0], np.cumsum([len(r) for r in raws])]).astype(np.int64)
    return np.concatenate(raws), off, np.array(scal, np.float64)


def _expected(c):
    """The reference's primary lines, each followed by its read's secondaries formatted from the fixture."""
    sec = rows_from_fixture(load_fixture(c["name"]))
    ref = S.RefModel.from_fasta(c["fasta"], c["levels"], c["k"], c["flag"], c["query_size"])
    lines = c["out_text"].splitlines(keepends=True)
    head = [ln for ln in lines if ln.startswith("@")]
    prim = [ln for ln in lines if not ln.startswith("@")]
    valid = np.nonzero(c["read_valid"])[0]
    assert len(prim) == len(valid)
    if c["sam"]:
        raw, off, scal = _load_raw(c["blow5"])
        with S.Aligner(ref, c["flag"]) as al:
            _, info, qev = al.align_raw(raw, off, scal, c["prefix_size"], c["query_size"], return_events=True)
    out = list(head)
    for vi, i in enumerate(valid):
        out.append(prim[vi])
        rid_name = str(c["read_ids"][i])
        for k in range(4):
            r = sec[vi, k]
            if not r["valid"]:
                continue
            g = int(r["rid"])
            if c["sam"]:
                y = ref.forward[g] if r["strand"] == ord("+") else ref.reverse[g]
                ql = int(info["qend"][i] - info["qstart"][i])
                out.append(S.sam_row(r, rid_name, ref.names[g], qev[i], 0, ql, y, int(ref.st_offset[g]), c["flag"], secondary=True))
            else:
                end_raw = int(c["ev_start_last"][vi]) + int(c["ev_len_last"][vi])
                out.append(S.paf_row(r, rid_name, ref.names[g], int(c["ev_start_first"][vi]), end_raw,
                                     int(c["qend"][i]) - 1 - int(c["qstart"][i]), int(c["len_raw"][i]),
                                     int(ref.seq_lengths[g]), tp="S"))
    return "".join(out)


@pytest.mark.parametrize("route", [[], ["--host-events"]])
@pytest.mark.parametrize("name", CASES)
def test_secondary_lines_equal_fixture(name, route, models):
    c = load_case(name)
    want = _expected(c)
    assert _run(c, models, route + ["--secondary", "yes"]) == want
    assert _run(c, models, route + ["--secondary", "no"]) == c["out_text"]


@pytest.mark.parametrize("route", [["--gpu-parse"], ["--ranks", "2"], ["--ranks", "2", "--gpu-parse"]])
@pytest.mark.parametrize("name", ["dna_default", "dna_sam", "rna_sam", "rna_dtw_std", "rna_q1000"])
def test_secondary_routes(name, route, models):
    c = load_case(name)
    assert _run(c, models, route + ["--secondary", "yes"]) == _expected(c)


def test_other_values_and_long_queries(models):
    c = load_case("dna_default")
    assert _run(c, models, ["--secondary", "maybe"]) == c["out_text"]  # as the reference: no effect
