#!/usr/bin/env python
"""Generate the interact-track fixtures under tests/golden/ucsc/ by running the REAL reference.

    python tests/golden/make_golden_ucsc.py <path to the reference's fithic/utils directory>

utils/visualize-UCSC.sh runs unmodified under LC_ALL=C on the inputs made below.  The inputs and the files the script wrote are
stored as DATA, gzipped (no reference source text is stored); cases.json records the awk the script ran with, because the
selection and the score's text are awk's and its libm's.  Not collected by pytest; the tests read only what this script wrote.

  uca        a real-shaped file: the fithic header line, tabs, three chromosomes, rows between two chromosomes, q spread
             across 0.05 with rows exactly at the threshold, one mantissa unit below and one above it
  ucq_1e-5   the quirks: zeros, every 1.000000e-k for k = 1..307, q at and next to 1 and above it, subnormal and overflowing
  ucq_5      fields (kept at 1e-5 by the string comparison), midpoints 0, 007 and 999999999; one input, two thresholds
  ucn        no newline after the last line, which is kept
  uce        no row passes: the two fixed lines
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ucsc")
HEADER = "chr1\tfragmentMid1\tchr2\tfragmentMid2\tcontactCount\tp-value\tq-value\tbias1\tbias2\tExpCC"
RES = 5000


def row(k, chrom, b1, b2, cc, q, chrom2=None, sep="\t", mids=None):
    q = q if isinstance(q, str) else "%e" % q
    m1, m2 = mids or ("%d" % (b1 * RES + RES // 2), "%d" % (b2 * RES + RES // 2))
    return sep.join([chrom, m1, chrom2 or chrom, m2, "%d" % cc, "1.000000e-09", q, "%.6f" % (0.8 + (k % 7) / 20), "%.6f" % (1.3 - (k % 5) / 20),
                     "%.6f" % (cc / 3 + 0.25)])


def uca():
    rng = np.random.default_rng(13)
    special = {3: "5.000000e-02", 4: "4.999999e-02", 5: "5.000001e-02", 9: "0.000000e+00", 12: "3.251000e-112", 17: "7.300000e-101",
               21: "5.000000e-02", 30: "1.000000e+00", 33: "4.999999e-02", 40: "5.000001e-02", 41: "1.000000e-03"}
    lines = [HEADER]
    for k in range(90):
        chrom = ["chr1", "chr2", "chrX"][k // 30]
        q = special.get(k, float(10 ** rng.uniform(-6, 0)))
        lines.append(row(k, chrom, 20 + 3 * k, 60 + 5 * k, int(rng.integers(5, 400)), q, chrom2="chr9" if k % 11 == 7 else None))
    return ("\n".join(lines) + "\n").encode()


def ucq():
    rng = np.random.default_rng(14)
    fields = ["0.000000e+00", "0.000000e-05"] + ["1.000000e-%02d" % k for k in range(1, 308)]
    fields += ["1.000000e+00", "9.999999e-01", "1.000001e+00", "2.000000e+00", "1.234567e+02", "1.000000e-320", "4.940656e-324", "1.000000e+309"]
    fields += ["%e" % float(10 ** rng.uniform(-9, 1)) for _ in range(40)]
    lines = [row(k, "chr%d" % (2 + k % 3), 7 + k, 90 + 2 * k, 5 + k % 50, f, sep=["\t", " ", "  ", " \t"][k % 4]) for k, f in enumerate(fields)]
    lines.append(row(1, "chr2", 0, 0, 9, "3.300000e-07", mids=("0", "007")))
    lines.append(row(2, "chr2", 0, 0, 9, "4.400000e-08", mids=("999999999", "0")))
    lines.append(row(3, "chr3", 0, 0, 9, "0.000000e+00", mids=("007", "999999999")))
    return ("\n".join(lines) + "\n").encode()


def ucn():
    rng = np.random.default_rng(15)
    lines = [HEADER.replace("\t", " ")] + [row(k, "chr4", 10 + k, 40 + k, 30 + k, float(10 ** rng.uniform(-5, 0)), sep=" ") for k in range(40)]
    lines.append(row(1, "chr6", 900, 950, 77, "1.000000e-03"))        # the last line is kept and lacks its newline
    return "\n".join(lines).encode()


def uce():
    rng = np.random.default_rng(16)
    return ("\n".join([HEADER] + [row(k, "chr1", 10 + k, 40 + k, 30 + k, float(10 ** rng.uniform(-1.2, 0))) for k in range(40)]) + "\n").encode()


def run_script(utils, data, qval, env):
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "sig.gz"), os.path.join(tmp, "track.txt")
        with gzip.open(src, "wb") as f:
            f.write(data)
        subprocess.run(["bash", os.path.join(utils, "visualize-UCSC.sh"), src, out, qval], env=env, cwd=tmp, capture_output=True, check=True)
        with open(out, "rb") as f:
            return f.read()


def store(name, data):
    with gzip.GzipFile(os.path.join(OUT, name), "wb", mtime=0) as f:
        f.write(data)


def main():
    utils = os.path.abspath(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    env = dict(os.environ, LC_ALL="C")
    awk = subprocess.run(["awk", "-W", "version"], capture_output=True, env=env).stdout.decode().splitlines()
    runs = []
    for name, make, qval in (("uca", uca, "0.05"), ("ucq_1e-5", ucq, "1e-5"), ("ucq_5", ucq, "5"), ("ucn", ucn, "0.05"), ("uce", uce, "0.05")):
        data = make()
        source = name.split("_")[0] + ".in.gz"
        store(source, data)
        made = run_script(utils, data, qval, env)
        store(name + ".track.gz", made)
        runs.append(dict(name=name, input=source, qval=qval, track=name + ".track.gz"))
        print("  wrote %s: %d lines in, %d track lines" % (name, len(data.splitlines()), made.count(b"\n") - 2))
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(dict(awk=awk[0] if awk else "unknown", locale="LC_ALL=C", runs=runs), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
