"""`sigfish-amd dtw --sam --device-paths` (event maps of a batch from the device) against `--host-paths` (warp paths rebuilt read by
read on the host threads, the default), byte for byte, and against the reference's own SAM of the golden cases that have one: ragged -K,
--secondary yes, two ranks, host events, records parsed on the GPU, and queries beyond 2048 events (rows the library computes on
the host inside the call)."""
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from tests.util import GOLD, ROOT, case_names, load_case

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "sigfish_amd", "bin", "sigfish-amd")
SAM_CASES = [n for n in case_names() if load_case(n)["sam"]]


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


def _run(c, models, extra, args=None):
    args = [str(a) for a in c["args"]] if args is None else args
    cmd = [BIN, "dtw", "--kmer-model", models[c["k"]], "--verbose", "0", *extra, *args, c["fasta"], c["blow5"]]
    r = subprocess.run(cmd, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


ROUTES = {"default": [], "ragged_K": ["-K", "3"], "host_events": ["--host-events"], "gpu_parse": ["--gpu-parse"],
          "ranks2": ["--ranks", "2", "--device", "0,0"], "profile_cpu": ["--profile-cpu=yes"]}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", SAM_CASES)
def test_golden_sam_on_both_routes(name, route, models):
    c = load_case(name)
    dev = _run(c, models, ROUTES[route] + ["--device-paths"])
    host = _run(c, models, ROUTES[route] + ["--host-paths"])
    assert dev == host
    assert dev == c["out_text"]


@functools.lru_cache(maxsize=None)
def _records(name):
    """How many primaries of golden case `name` have a SAM record, from the case's own rows and the per-read host routine
    (S.r2qevent_map, pinned to the reference's path_to_map by tests/test_host_stages.py): every mapped read, except that with --rna
    the ss string mirrors every index about the last reference column's stop, so a read whose warp path leaves that column blank
    (-1/-1: entered without advancing in the query, which the forced end column of --dtw-std makes common) has none -- the
    reference asserts there (r2qevent_map_to_ss, src/sigfish.c:668-669), the writer here refuses the row."""
    c = load_case(name)
    ref = S.RefModel.from_fasta(c["fasta"], c["levels"], c["k"], c["flag"], c["query_size"])
    rna = bool(c["flag"] & S.RNA)
    rows = np.zeros(len(c["score"]), S.RESULT_DTYPE)
    for f in ("rid", "pos_st", "pos_end", "score", "score2", "strand", "mapq"):
        rows[f] = c[f]
    rows["valid"] = 1
    n, vi = 0, 0
    for i, (rid, meta, raw) in enumerate(S.Blow5File(c["blow5"])):
        if not c["read_valid"][i]:
            continue
        ev = S.detect_events(raw, meta, rna)
        keep, qs, qe = S.select_query(ev, raw, meta, c["prefix_size"], c["query_size"], c["flag"], 0)
        assert keep and (qs, qe) == (int(c["qstart"][i]), int(c["qend"][i]))
        r = rows[vi]
        vi += 1
        if r["rid"] < 0:
            continue
        j = int(r["rid"])
        pairs = S.r2qevent_map(r, ev, qs, qe, ref.forward[j] if r["strand"] == ord("+") else ref.reverse[j], int(ref.st_offset[j]), c["flag"])
        n += not (rna and pairs[-1, 1] < 0)
    assert vi == len(rows)
    return n


@pytest.mark.parametrize("name", ["dna_default", "dna_q700", "rna_default", "rna_invert", "rna_dtw_std", "rna_full_ref_dtw_std",
                                  "rna_q1000", "rna_q500_pauto"])
@pytest.mark.parametrize("extra", [[], ["--secondary", "yes", "-K", "3"]], ids=["primaries", "secondaries_ragged_K"])
def test_sam_of_the_other_cases_equals_host_paths(name, extra, models):
    c = load_case(name)
    args = [str(a) for a in c["args"]] + ["--sam"]
    dev = _run(c, models, extra + ["--device-paths"], args)
    assert dev == _run(c, models, extra + ["--host-paths"], args)
    flags = [int(l.split("\t")[1]) for l in dev.splitlines() if not l.startswith("@")]
    # one record per primary that has one, whatever else is printed behind it
    assert sum(not f & 256 for f in flags) == _records(name)
    if name not in ("rna_dtw_std", "rna_full_ref_dtw_std"):  # a free end column is never entered sideways: every mapped read has its record
        assert _records(name) == int(c["read_valid"].sum())
    assert extra or not any(f & 256 for f in flags)


@pytest.mark.parametrize("extra", [[], ["--ranks", "2", "--device", "0,0"], ["--host-events"]], ids=["one", "ranks2", "host_events"])
def test_long_queries_take_the_host_rows(extra, models):
    """-q 2500 on the long-signal fixture: reads of more than 2048 events are computed by the host routine inside the library call."""
    c = load_case("rna_q2500")
    args = [str(a) for a in c["args"]] + ["--sam"]
    dev = _run(c, models, extra + ["--device-paths"], args)
    assert dev == _run(c, models, extra + ["--host-paths"], args)
    assert sum(not l.startswith("@") for l in dev.splitlines()) == int(c["read_valid"].sum())
