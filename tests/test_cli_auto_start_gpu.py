"""The command line with the RNA automatic query start (--rna -q 500 -p -1) on its device route: events, adaptor and
poly-A search on the GPU (and the records decoded there with --gpu-parse) print byte for byte what the host route
(--host-events) prints, the stderr summary (prefix fail / ignored / too short) included."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from sigfish_amd import synth
from tests.util import GOLD, ROOT, write_blow5

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "sigfish_amd", "bin", "sigfish-amd")
FASTA = os.path.join(GOLD, "data", "rnasequin_sequences_2.4.fa")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("pauto")
    lv = np.fromfile(os.path.join(GOLD, "models", "syn5.f32"), np.float32)
    model = d / "syn5.model"
    with open(model, "w") as f:
        f.write("#k\t5\nkmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\n")
        for kmer, v in zip(itertools.product("ACGT", repeat=5), lv):
            f.write("%s\t%.4f\t1.5000\t1.0\t1.0\n" % ("".join(kmer), v))
    out = {}
    for kit, pore in (("unknown", 0), ("sqk-rna004", 2)):
        reads = synth.make_rna_polya_reads(400, seed=101 + pore, pore=pore)
        attrs = (("experiment_type", "rna"), ("sequencing_kit", kit))
        for press in ("zlib_svb", "none"):
            p = str(d / f"{kit}_{press}.blow5")
            write_blow5(p, reads, attrs=attrs, compress=press == "zlib_svb")
            out[f"{kit}_{press}.blow5"] = p
        # SLOW5 ASCII writes its doubles without an exponent: the reads with a range beyond fp32 (1e39) stay in the BLOW5 files
        finite = str(d / f"{kit}_finite.blow5")
        write_blow5(finite, [r for r in reads if not r[0].endswith("nonfinite")], attrs=attrs)
        p = str(d / f"{kit}.slow5")
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_blow5.py"), finite, p, "--copies", "1",
                        "--ascii", "--keep-ids"], check=True, capture_output=True)
        out[f"{kit}.slow5"] = p
    return str(model), out


def _run(model, path, extra):
    cmd = [BIN, "dtw", "--kmer-model", model, "--verbose", "3", "--rna", "-q", "500", "-p", "-1", *extra, FASTA, path]
    r = subprocess.run(cmd, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    counts = [tuple(int(x) for x in m) for m in
              re.findall(r"total entries: (\d+)\tprefix fail: (\d+)\tignored: (\d+)\ttoo short: (\d+)", r.stderr.decode())]
    assert counts, r.stderr.decode()
    return r.stdout.decode(), tuple(int(x) for x in np.sum(counts, axis=0))


NAMES = ["unknown_zlib_svb.blow5", "unknown_none.blow5", "unknown.slow5", "sqk-rna004_zlib_svb.blow5", "sqk-rna004_none.blow5", "sqk-rna004.slow5"]


@pytest.mark.parametrize("name", NAMES)
def test_device_route_prints_what_the_host_route_prints(name, files):
    model, paths = files
    want_out, want_counts = _run(model, paths[name], ["--host-events"])
    assert want_out.count("\n") > 100
    assert want_counts[0] > 380 and want_counts[1] > 20, want_counts  # (some reads fall back: the comparison is not vacuous)
    variants = [[], ["--ranks", "2"]]
    if name.endswith(".blow5"):
        variants.append(["--gpu-parse"])
    for extra in variants:
        out, counts = _run(model, paths[name], extra)
        assert out == want_out, extra
        assert counts == want_counts, (extra, counts, want_counts)


@pytest.mark.parametrize("name", ["unknown_zlib_svb.blow5", "sqk-rna004_none.blow5", "sqk-rna004.slow5"])
def test_sam_device_route_prints_what_the_host_route_prints(name, files):
    model, paths = files
    want_out, want_counts = _run(model, paths[name], ["--host-events", "--sam"])
    assert want_out.count("\n") > 100
    variants = [["--sam"]] + ([["--sam", "--gpu-parse"]] if name.endswith(".blow5") else [])
    for extra in variants:
        out, counts = _run(model, paths[name], extra)
        assert out == want_out, extra
        assert counts == want_counts, extra
