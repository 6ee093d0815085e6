#!/usr/bin/env python
"""Generate the HiC-Pro converter fixtures under tests/golden/hicpro/ by running the REAL reference.

    python tests/golden/make_golden_hicpro.py <path to the reference's fithic/utils/HiCPro2FitHiC.py>

The reference module is loaded by path and its unmodified outputfithicform() runs on the inputs made below; the inputs and the
three decompressed outputs are stored gzipped, as DATA (no reference source text is stored).  Not collected by pytest; the
tests read only what this script wrote.

  hp1  five bins on two chromosomes, short last bins; a diagonal line, a `7.0` count, a NaN bias; -r 0
  hp2  three chromosomes, 300 bins at 10 kb, 40 000 matrix lines sorted by (i, j) (0.6 MB of text: lines straddle the 16 KB scan
       blocks), diagonal lines, `.000000` counts, a bias file with NaNs; run with -r 0, and with -r 10000 on a bed whose first line
       is a shorter bin
  hp3  bed indices that start at 7, out of order, with a gap no matrix line uses and one index listed twice (the later line
       wins); a matrix with \\r\\n, mixed tabs and blanks, leading blanks and no newline at the end; no bias file
"""
import contextlib
import gzip
import importlib.util
import io
import json
import os
import sys
import tempfile

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hicpro")


def load_reference(path):
    spec = importlib.util.spec_from_file_location("HiCPro2FitHiC_reference", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bed_text(chroms, res, first_end=None):
    """chroms: [(name, length)] -> fixed-size bins, the last one of a chromosome short; indices from 1"""
    lines, index = [], 1
    for name, length in chroms:
        for start in range(0, length, res):
            lines.append("%s\t%d\t%d\t%d\n" % (name, start, min(start + res, length), index))
            index += 1
    if first_end is not None:                                        # the first line as a shorter bin
        t = lines[0].split("\t")
        lines[0] = "\t".join([t[0], t[1], str(first_end), t[3]])
    return "".join(lines), index - 1


def hp1():
    bed = "chr1\t0\t1000\t1\nchr1\t1000\t2000\t2\nchr1\t2000\t2500\t3\nchr2\t0\t1000\t4\nchr2\t1000\t1300\t5\n"
    matrix = "1\t1\t4\n1\t2\t7.0\n2\t4\t3\n3\t5\t12\n4\t4\t1\n"
    bias = "0.8\n1.25\nnan\n1.1\n0.95\n"
    return dict(bed=bed.encode(), matrix=matrix.encode(), bias=bias.encode())


def hp2():
    rng = np.random.default_rng(20260117)
    chroms = [("chrA", 1195000), ("chrB", 1000000), ("chrC", 798500)]
    bed, n = bed_text(chroms, 10000)
    bed_short, _ = bed_text(chroms, 10000, first_end=6000)
    assert n == 300
    iu, ju = np.triu_indices(n)                                      # every cell i <= j, in (i, j) order
    keep = np.sort(rng.choice(len(iu), 40000, replace=False))
    decay = 1.0 / (1.0 + np.abs(iu[keep] - ju[keep]))                # counts fall off with the distance, as Hi-C counts do
    count = np.maximum(1, (rng.pareto(1.2, len(keep)) * 40000 * decay).astype(np.int64)) % 1000000
    style = rng.random(len(keep))
    lines = []
    for k, c, s in zip(keep, count, style):
        text = "%d" % c if s < 0.5 else ("%d.000000" % c if s < 0.9 else "%d.0" % c)
        lines.append("%d\t%d\t%s\n" % (iu[k] + 1, ju[k] + 1, text))
    matrix = "".join(lines)
    assert len(matrix) > 30 * 16384 and (iu[keep] == ju[keep]).sum() > 50
    b = np.exp(0.3 * rng.standard_normal(n))
    bias = "".join("nan\n" if rng.random() < 0.04 else "%s\n" % repr(float(v)) for v in b)
    assert 3 < bias.count("nan") < 40
    return dict(bed=bed.encode(), bed_short=bed_short.encode(), matrix=matrix.encode(), bias=bias.encode())


def hp3():
    bed = ("chrX\t0\t5000\t7\nchrX\t10000\t15000\t9\nchrX\t5000\t10000\t8\nchrY\t0\t5000\t12\nchrY\t5000\t10000\t13\n"
           "chrX\t99000\t104000\t9\n")
    matrix = b"7 8 3\r\n  9\t12   5\r\n13 13 2\r\n \t7\t13 1.000\r\n12\t 12\t 40\r\n8 9 6"
    return dict(bed=bed.encode(), matrix=matrix)


def main():
    ref = load_reference(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    inputs = {"hp1": hp1(), "hp2": hp2(), "hp3": hp3()}
    for case, files in inputs.items():
        for kind, data in files.items():
            with gzip.GzipFile(os.path.join(OUT, "%s.%s.gz" % (case, kind)), "wb", mtime=0) as f:
                f.write(data)
    runs = [dict(name="hp1", bed="hp1.bed.gz", matrix="hp1.matrix.gz", bias="hp1.bias.gz", res=0),
            dict(name="hp2_r0", bed="hp2.bed.gz", matrix="hp2.matrix.gz", bias="hp2.bias.gz", res=0),
            dict(name="hp2_r10000", bed="hp2.bed_short.gz", matrix="hp2.matrix.gz", bias="hp2.bias.gz", res=10000),
            dict(name="hp3", bed="hp3.bed.gz", matrix="hp3.matrix.gz", bias=None, res=0)]
    for run in runs:
        with tempfile.TemporaryDirectory() as tmp:
            paths = {}
            for kind in ("bed", "matrix", "bias"):
                if run[kind] is None:
                    paths[kind] = None
                    continue
                paths[kind] = os.path.join(tmp, kind)
                with gzip.open(os.path.join(OUT, run[kind]), "rb") as f, open(paths[kind], "wb") as g:
                    g.write(f.read())
            outs = {k: os.path.join(tmp, k + ".gz") for k in ("contacts", "fragments", "bias")}
            with contextlib.redirect_stdout(io.StringIO()) as said:
                ref.outputfithicform(paths["bed"], paths["matrix"], outs["contacts"], outs["fragments"], paths["bias"],
                                     outs["bias"] if paths["bias"] else None, run["res"])
            run["stdout"] = said.getvalue()
            for kind, path in outs.items():
                if kind == "bias" and paths["bias"] is None:
                    continue
                with gzip.open(path, "rb") as f:
                    data = f.read()
                with gzip.GzipFile(os.path.join(OUT, "%s.%s.out.gz" % (run["name"], kind)), "wb", mtime=0) as f:
                    f.write(data)
        print("  wrote %s" % run["name"])
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(runs, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
