"""Shared by the tests of `sigfish-amd realtime` (not product code): k-mer model files of the golden cases, PAF text helpers."""
import itertools
import os

import numpy as np

from tests.util import GOLD, ROOT

BIN = os.path.join(ROOT, "sigfish_amd", "bin", "sigfish-amd")
TAGS = 3  # ne:i, ns:i, dc:A at the end of every line


def write_model(path, k, levels=None):
    """the k-mer model file of the golden cases (tests/golden/models/syn<k>.f32), or of `levels`, as --kmer-model reads it"""
    lv = np.fromfile(os.path.join(GOLD, "models", f"syn{k}.f32"), np.float32) if levels is None else levels
    with open(path, "w") as f:
        f.write(f"#k\t{k}\nkmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\n")
        for kmer, v in zip(itertools.product("ACGT", repeat=k), lv):
            f.write("%s\t%.4f\t1.5000\t1.0\t1.0\n" % ("".join(kmer), v))
    return str(path)


def strip_tags(text):
    """the lines without their three realtime tags, sorted by read id"""
    lines = ["\t".join(ln.split("\t")[:-TAGS]) + "\n" for ln in text.splitlines()]
    return sorted(lines, key=lambda ln: ln.split("\t")[0])


def tags(line):
    f = line.rstrip("\n").split("\t")[-TAGS:]
    assert f[0].startswith("ne:i:") and f[1].startswith("ns:i:") and f[2].startswith("dc:A:"), line
    return int(f[0][5:]), int(f[1][5:]), f[2][5:]
