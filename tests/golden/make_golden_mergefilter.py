#!/usr/bin/env python
"""Generate the merge-filter fixtures under tests/golden/mergefilter/ by running the REAL reference.

    python tests/golden/make_golden_mergefilter.py <path to the reference's fithic/utils directory>

utils/merge-filter.sh runs unmodified under LC_ALL=C, with UTILITYFOLDER exported as that directory plus a trailing slash (the
script builds the path of CombineNearbyInteraction.py from it), on the inputs made below.  The inputs, the decompressed
fithic_subset.gz and the decompressed merged file are stored as DATA (no reference source text is stored); cases.json records
the awk the script ran with, because the selection is awk's and awk implementations differ in what they take for a number.
Not collected by pytest; the tests read only what this script wrote.

  mfa        three chromosomes of clusters with a header line, 10 columns, mixed tabs and blanks, q spread across fdr = 0.05 with
             rows exactly at the threshold, one mantissa unit below and one above it, an exact-zero q, three-digit exponents
  mfq_1e-5   the quirks, no header: a data row on line 1 (the script drops it), subnormal q, 2.225074e-308 (a number to mawk)
  mfq_5      and 2.225073e-308 (a string), the same input at fdr = 1e-5 and at fdr = 5
  mfn        no newline after the last line, which is kept
  mfe        no row passes: what the script leaves behind then
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mergefilter")
HEADER = "chr1 fragmentMid1 chr2 fragmentMid2 contactCount p-value q-value bias1 bias2 ExpCC"
RES = 5000


def row(k, chrom, b1, b2, cc, q, chrom2=None, p=None):
    sep = ["\t", " ", "  ", "\t ", " \t"][k % 5]
    q = q if isinstance(q, str) else "%e" % q
    p = p or ("%e" % (float(q) / 50 if float(q) < float("inf") else 1e-9))
    cols = [chrom, "%d" % (b1 * RES + RES // 2), chrom2 or chrom, "%d" % (b2 * RES + RES // 2), "%d" % cc, p, q, "%.6f" % (0.8 + (k % 7) / 20),
            "%.6f" % (1.3 - (k % 5) / 20), "%.6f" % (cc / 3 + 0.25)]
    return sep.join(cols)


def clusters(rng, chroms, per_chrom, q_of):
    """rows of clusters of neighbouring cells: (chrom, bin1, bin2, count, q)"""
    rows, seen = [], set()
    for c, chrom in enumerate(chroms):
        for g in range(per_chrom):
            b1, b2 = 20 + 37 * g + 3 * c, 60 + 41 * g + 5 * c
            shape = [(0, 0), (0, 1), (1, 0), (1, 1), (-1, 0), (0, -1), (2, 1), (-1, -1), (1, 2), (3, 3), (0, 5), (-4, 0), (6, 6)][: 5 + (g * 3 + c) % 9]
            for d1, d2 in shape:
                cell = (chrom, b1 + d1, b2 + d2)
                if cell in seen:
                    continue
                seen.add(cell)
                rows.append((chrom, b1 + d1, b2 + d2, int(rng.integers(5, 400)), q_of(rng, len(rows))))
    return rows


def mfa():
    rng = np.random.default_rng(3)

    def q_of(rng, k):
        special = {3: "5.000000e-02", 4: "4.999999e-02", 5: "5.000001e-02", 9: "0.000000e+00", 12: "3.251000e-112", 17: "7.300000e-101",
                   21: "5.000000e-02", 30: "1.000000e+00", 33: "4.999999e-02", 40: "5.000001e-02"}
        if k in special:
            return special[k]
        return float(10 ** rng.uniform(-6, 0))                        # about a quarter of the rows lie above 0.05
    lines = [HEADER.replace(" ", "\t")]
    for k, (chrom, b1, b2, cc, q) in enumerate(clusters(rng, ["chr1", "chr2", "chrX"], 7, q_of)):
        lines.append(row(k, chrom, b1, b2, cc, q))
        if k % 23 == 7:                                               # a contact between two chromosomes that passes
            lines.append(row(k + 1, chrom, b1, b2 + 9, cc, "1.250000e-04", chrom2="chr9"))
    return ("\n".join(lines) + "\n").encode()


def mfq():
    rng = np.random.default_rng(4)

    def q_of(rng, k):
        special = {0: "1.000000e-07", 2: "1.000000e-320", 3: "2.225074e-308", 4: "2.225073e-308", 6: "9.000000e-315", 8: "4.940656e-324",
                   10: "1.000000e-05", 11: "1.000001e-05", 12: "9.999999e-06", 14: "5.000000e+00", 15: "5.000001e+00", 16: "4.999999e+00",
                   20: "0.000000e+00", 25: "2.225074e-308", 26: "2.225073e-308", 27: "1.000000e-310"}
        if k in special:
            return special[k]
        return float(10 ** rng.uniform(-9, 1))
    rows = clusters(rng, ["chr2", "chr10", "chr3"], 6, q_of)
    return ("\n".join(row(k, *r) for k, r in enumerate(rows)) + "\n").encode()


def mfn():
    rng = np.random.default_rng(5)
    rows = clusters(rng, ["chr4", "chr5", "chr6"], 5, lambda rng, k: float(10 ** rng.uniform(-5, 0)))
    lines = [HEADER] + [row(k, *r) for k, r in enumerate(rows)]
    lines.append(row(1, "chr6", 900, 950, 77, "1.000000e-03"))        # the last line is kept and lacks its newline
    return "\n".join(lines).encode()


def mfe():
    rng = np.random.default_rng(6)
    rows = clusters(rng, ["chr1", "chr2", "chr3"], 4, lambda rng, k: float(10 ** rng.uniform(-1.2, 0)))
    return ("\n".join([HEADER] + [row(k, *r) for k, r in enumerate(rows)]) + "\n").encode()


def run_script(utils, data, fdr, env):
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "sig.gz")
        with gzip.open(src, "wb") as f:
            f.write(data)
        out = os.path.join(tmp, "out", "merged.gz")
        subprocess.run(["bash", os.path.join(utils, "merge-filter.sh"), src, str(RES), out, fdr, "ignored"], env=env, cwd=tmp,
                       capture_output=True, check=True)
        with gzip.open(os.path.join(tmp, "out", "fithic_subset.gz"), "rb") as f:
            subset = f.read()
        with gzip.open(out, "rb") as f:
            return subset, f.read()


def store(name, data):
    with gzip.GzipFile(os.path.join(OUT, name), "wb", mtime=0) as f:
        f.write(data)


def main():
    utils = os.path.abspath(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    env = dict(os.environ, LC_ALL="C", UTILITYFOLDER=utils.rstrip("/") + "/")
    awk = subprocess.run(["awk", "-W", "version"], capture_output=True, env=env).stdout.decode().splitlines()
    runs = []
    for name, make, fdr in (("mfa", mfa, "0.05"), ("mfq_1e-5", mfq, "1e-5"), ("mfq_5", mfq, "5"), ("mfn", mfn, "0.05"), ("mfe", mfe, "0.05")):
        data = make()
        source = name.split("_")[0] + ".in.gz"
        store(source, data)
        subset, merged = run_script(utils, data, fdr, env)
        store(name + ".subset.gz", subset)
        store(name + ".merged.gz", merged)
        runs.append(dict(name=name, input=source, fdr=fdr, res=RES, subset=name + ".subset.gz", merged=name + ".merged.gz"))
        print("  wrote %s: %d lines in, %d kept, %d merged" % (name, len(data.splitlines()), subset.count(b"\n"), len(merged.splitlines()) - 1))
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(dict(awk=awk[0] if awk else "unknown", locale="LC_ALL=C", runs=runs), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
