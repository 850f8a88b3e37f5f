"""`dtw -q 3000 --secondary yes --secondary-strips` on the long random-signal DNA file (tests/golden/random/rnd_dnalong.blow5, six
reads of 3000 query events): the primary lines are the bytes of the same command without --secondary (which are the reference's,
rnd_dnalong_q3000.out), and behind each come the tp:A:S lines formatted from the library's own rows for the same events -- PAF
through paf_row(tp="S"), SAM through sam_row(secondary=True) on the device's query events -- with two ranks and with --sam
--device-paths, where the secondaries' ss strings come from sfa_event_maps in row strips."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import sigfish_amd as S
from tests.util import GOLD, ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "sigfish_amd", "bin", "sigfish-amd")
FASTA = os.path.join(GOLD, "data", "nCoV-2019.reference.fasta")
BLOW5 = os.path.join(GOLD, "random", "rnd_dnalong.blow5")
K, Q, P = 6, 3000, 50


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    lv = np.fromfile(os.path.join(GOLD, "models", f"syn{K}.f32"), np.float32)
    p = tmp_path_factory.mktemp("models") / f"syn{K}.model"
    with open(p, "w") as f:
        f.write(f"#k\t{K}\nkmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\n")
        for kmer, v in zip(itertools.product("ACGT", repeat=K), lv):
            f.write("%s\t%.4f\t1.5000\t1.0\t1.0\n" % ("".join(kmer), v))
    return str(p), lv


def _run(model, extra):
    cmd = [BIN, "dtw", "--kmer-model", model[0], "--verbose", "0", "-q", str(Q), *extra, FASTA, BLOW5]
    r = subprocess.run(cmd, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode()


@pytest.fixture(scope="module")
def library(model):
    """ids, rows, secondaries, query infos and query events of the file's reads from the library, and the reference"""
    ids, raws, scal = [], [], []
    for rid, meta, raw in S.Blow5File(BLOW5):
        ids.append(rid)
        raws.append(raw)
        scal.append([meta["digitisation"], meta["offset"], meta["range"]])
    off = np.concatenate([[0], np.cumsum([len(r) for r in raws])]).astype(np.int64)
    ref = S.RefModel.from_fasta(FASTA, model[1], K, 0, Q)
    with S.Aligner(ref, 0) as al:
        al.set_secondary(4)
        al.set_option("secondary_strips", 1)
        rows, info, qev = al.align_raw(np.concatenate(raws), off, np.array(scal, np.float64), P, Q, return_events=True)
        sec = al.secondary_rows()
    assert (info["qend"] - info["qstart"] > 2048).all() and sec["valid"][rows["valid"] == 1].all()
    return ids, [len(r) for r in raws], rows, sec, info, qev, ref


def _secondary_lines(library, i, sam):
    ids, n_raw, rows, sec, info, qev, ref = library
    out = []
    for r in sec[i]:
        if not r["valid"]:
            continue
        g = int(r["rid"])
        if sam:
            y = ref.forward[g] if r["strand"] == ord("+") else ref.reverse[g]
            out.append(S.sam_row(r, str(ids[i]), ref.names[g], qev[i], 0, int(info["qend"][i] - info["qstart"][i]), y, int(ref.st_offset[g]), 0, secondary=True))
        else:
            out.append(S.paf_row(r, str(ids[i]), ref.names[g], int(info["start_raw_idx"][i]), int(info["end_raw_idx"][i]),
                                 int(info["qend"][i]) - 1 - int(info["qstart"][i]), n_raw[i], int(ref.seq_lengths[g]), tp="S"))
    return out


@pytest.mark.parametrize("route", [["--ranks", "2"], ["--sam", "--device-paths"]], ids=["ranks2", "sam_device_paths"])
def test_long_query_secondary_lines(route, model, library):
    sam = "--sam" in route
    plain = _run(model, route)
    if not sam:
        assert plain == open(os.path.join(GOLD, "random", "rnd_dnalong_q3000.out")).read()
    got = _run(model, route + ["--secondary", "yes", "--secondary-strips"])
    head = [ln for ln in plain.splitlines(keepends=True) if ln.startswith("@")]
    prim = [ln for ln in plain.splitlines(keepends=True) if not ln.startswith("@")]
    ids, rows = library[0], library[2]
    valid = [i for i in range(len(ids)) if rows["valid"][i] and rows["rid"][i] >= 0]
    assert len(prim) == len(valid)
    want = list(head)
    for ln, i in zip(prim, valid):
        assert ln.startswith(str(ids[i]) + "\t")
        want.append(ln)  # the primary line: the bytes printed without --secondary
        want += _secondary_lines(library, i, sam)
    assert got == "".join(want)
    assert len(want) - len(head) == 5 * len(valid)  # every read's four secondaries were printed
