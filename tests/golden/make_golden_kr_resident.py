#!/usr/bin/env python
"""Generate the end-to-end fixture of `fithic --kr` under tests/golden/kr_resident/ by running the REAL reference.

    python tests/golden/make_golden_kr_resident.py <path to the reference checkout (the directory that holds fithic/)>

The protocol's two steps run unmodified on the bundled hESC chr1 40 kb set (tests/golden/data): fithic/utils/HiCKRy.py with
-x 0.12 writes a bias file, then fithic/fithic.py reads it with -t (-r 40000 -p 2 -x All).  Stored as DATA (no reference source
text is stored):

    bias.npy            the bias vector HiCKRy wrote, one double per fragment line (-1 at the removed rows)
    pass1_columns.npz   every STRIDE-th row (rows 0, STRIDE, 2 STRIDE, ...) of the pass-1 significances file: fragmentMid1,
                        fragmentMid2, contactCount as integers, p-value and q-value parsed as doubles
    pass1_text.txt.gz   the same rows' bias1, bias2 and ExpCC columns as the text the reference printed
    cases.json          the arguments, the stride, the number of rows of the whole file, the names of its two chromosome columns

The whole file has 7.8e5 rows (50 MB of text): the stride keeps every stored file far below the size limit for committed files.
Not collected by pytest; the tests read only what this script wrote.
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "kr_resident")
DATA = os.path.join(HERE, "data")
RES, PASSES, PERC, LIB, MODE, STRIDE = 40000, 2, "0.12", "kr", "All", 61


def main():
    ref = os.path.abspath(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    env = dict(os.environ, LC_ALL="C", MPLBACKEND="Agg")
    inputs = dict(contacts="hESC_chr1_w40000.contacts.gz", frags="hESC_chr1_w40000.frags.gz")
    con, frg = os.path.join(DATA, inputs["contacts"]), os.path.join(DATA, inputs["frags"])
    with tempfile.TemporaryDirectory() as tmp:
        bias_path, run = os.path.join(tmp, "bias.gz"), os.path.join(tmp, "run")
        subprocess.run([sys.executable, os.path.join(ref, "fithic", "utils", "HiCKRy.py"), "-i", con, "-f", frg, "-o", bias_path, "-x", PERC],
                       check=True, stdout=subprocess.DEVNULL, env=env, cwd=tmp)
        subprocess.run([sys.executable, os.path.join(ref, "fithic", "fithic.py"), "-i", con, "-f", frg, "-t", bias_path, "-o", run,
                        "-r", str(RES), "-p", str(PASSES), "-x", MODE, "-l", LIB], check=True, stdout=subprocess.DEVNULL, env=env, cwd=tmp)
        with gzip.open(bias_path, "rt") as f:
            bias_lines = [ln.split() for ln in f]
        with gzip.open(os.path.join(run, "%s.spline_pass1.res%d.significances.txt.gz" % (LIB, RES)), "rt") as f:
            header = f.readline().rstrip("\n").split("\t")
            rows = [ln.rstrip("\n").split("\t") for ln in f]
    kept = rows[::STRIDE]
    np.save(os.path.join(OUT, "bias.npy"), np.array([float(w[2]) for w in bias_lines], np.float64))
    np.savez_compressed(os.path.join(OUT, "pass1_columns.npz"), mid1=np.array([int(w[1]) for w in kept], np.int32),
                        mid2=np.array([int(w[3]) for w in kept], np.int32), count=np.array([int(w[4]) for w in kept], np.int32),
                        p=np.array([float(w[5]) for w in kept], np.float64), q=np.array([float(w[6]) for w in kept], np.float64))
    with gzip.GzipFile(os.path.join(OUT, "pass1_text.txt.gz"), "wb", mtime=0) as f:
        f.write("".join("%s\t%s\t%s\n" % (w[7], w[8], w[9]) for w in kept).encode())
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(dict(inputs=inputs, res=RES, passes=PASSES, perc=PERC, mode=MODE, lib=LIB, stride=STRIDE, header=header, rows=len(rows),
                       stored_rows=len(kept), chr1=sorted({w[0] for w in rows}), chr2=sorted({w[2] for w in rows}),
                       bias_lines=len(bias_lines), bias_removed=sum(1 for w in bias_lines if float(w[2]) == -1.0)), f, indent=1)
        f.write("\n")
    print("  wrote kr_resident: %d bias lines, %d of %d rows of the pass-1 file (stride %d)" % (len(bias_lines), len(kept), len(rows), STRIDE))


if __name__ == "__main__":
    main()
