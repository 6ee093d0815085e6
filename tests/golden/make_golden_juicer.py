#!/usr/bin/env python
"""Generate the Juicer dump fixtures under tests/golden/juicer/ by running the REAL reference.

    python tests/golden/make_golden_juicer.py <path to the reference's fithic/utils directory>

Verbatim runs: utils/createFitHiCContacts-hic_old.sh runs unmodified under LC_ALL=C on the dump texts made below.
Midpoint runs: utils/createFitHiCContacts-hic.py runs unmodified; PYTHONPATH points at a temporary directory into which this script
writes its own small stand-in `hicstraw` module (HICSTRAW below: a HiCFile with the three getters, and a straw() that returns the
records read from the dump TEXT, the counts passed through numpy.float32 as the real binding holds them).  The inputs and the
files the reference wrote are stored as DATA, gzipped (no reference source text is stored); cases.json records the awk the script
ran with.  Not collected by pytest; the tests read only what this script wrote.

  jva              verbatim, a regular dump of chromosome 1 against itself
  jvq_01_1e3       verbatim, the quirks: mixed and leading blanks, a fourth token, one- and two-token lines, an empty line, a blank
  jvq_chrX         line, `12.50`, a count in exponent form; one input, the names 01 / 1e3 and chrX / chrX
  jvn              verbatim, no newline after the last line
  jve              verbatim, an empty file
  jma_r5000        midpoint, a regular dump, even R
  jmx_r5000        midpoint, CHR1 != CHR2: counts 1, 0, 16777216, `17`, `17.0`, `017`, bin 0 and the largest bin of the grid whose
  jmo_r10001       midpoint fits int32; the same with an odd R (int(R/2) rounds down)
  jmr_r2           midpoint, R = 2: the bin 2147483646 whose midpoint is 2^31 - 1 exactly
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "juicer")
INT32_MAX = (1 << 31) - 1

HICSTRAW = '''"""stand-in for hicstraw: the records come from the text `juicer_tools dump` prints"""
import os

import numpy


class _Record:
    def __init__(self, x, y, c):
        self.binX, self.binY, self.counts = int(x), int(y), numpy.float32(c)


class HiCFile:
    def __init__(self, path):
        self.path = path

    def getChromosomes(self):
        return []

    def getGenomeID(self):
        return "dump"

    def getResolutions(self):
        return [int(os.environ["HICSTRAW_STANDIN_RESOLUTION"])]


def straw(datatype, norm, path, chr1, chr2, unit, resolution):
    with open(path) as f:
        return [_Record(*line.split()) for line in f]
'''


def regular(seed, res, n):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.integers(0, 400, n)) * res
    y = x + rng.integers(0, 60, n) * res
    return "".join("%d\t%d\t%d\n" % (a, b, c) for a, b, c in zip(x, y, rng.integers(1, 900, n))).encode()


def quirks():
    return (b"0\t5000\t3\n" b"5000 10000 12.50\n" b"  10000\t \t15000   7\n" b"\t15000\t20000\t1\n" b"20000 25000 4 extra tokens here\n"
            b"25000\n" b"30000 35000\n" b"\n" b" \t \n" b"35000\t40000\t1e3\n" b"a\tb\tc\n" b"40000\t45000\t0.333   \n" b"45000  50000\t\t2\t\n")


def largest_bin(res):
    return (INT32_MAX - res // 2) // res * res


def edges(res):
    top = largest_bin(res)
    rows = [(0, 0, "1"), (0, res, "0"), (res, 3 * res, "16777216"), (2 * res, 2 * res, "17"), (2 * res, 4 * res, "17.0"), (3 * res, 9 * res, "017"),
            (0, top, "5"), (top, top, "2.000"), (7 * res, top - res, "16777215")]
    return "".join("%d\t%d\t%s\n" % r for r in rows).encode()


def run_old_script(utils, data, chr1, chr2, env):
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "dump.txt"), os.path.join(tmp, "out.gz")
        with open(src, "wb") as f:
            f.write(data)
        subprocess.run(["bash", os.path.join(utils, "createFitHiCContacts-hic_old.sh"), src, chr1, chr2, out], env=env, cwd=tmp,
                       capture_output=True, check=True)
        return gzip.open(out, "rb").read()


def run_py(utils, data, chr1, chr2, res, env):
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "dump.txt"), os.path.join(tmp, "out.txt")
        with open(src, "wb") as f:
            f.write(data)
        with open(os.path.join(tmp, "hicstraw.py"), "w") as f:
            f.write(HICSTRAW)
        r = subprocess.run([sys.executable, os.path.join(utils, "createFitHiCContacts-hic.py"), "--HiCFile", src, "--CHR1", chr1, "--CHR2", chr2,
                            "--resolution", str(res), "--datatype", "observed", "--Norm", "NONE", "--outFile", out],
                           env=dict(env, PYTHONPATH=tmp, HICSTRAW_STANDIN_RESOLUTION=str(res)), cwd=tmp, capture_output=True, check=True)
        with open(out, "rb") as f:
            return f.read(), r.stdout.decode().replace(os.path.realpath(tmp), "<tmp>")


def store(name, data):
    with gzip.GzipFile(os.path.join(OUT, name), "wb", mtime=0) as f:
        f.write(data)


def main():
    utils = os.path.abspath(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    env = dict(os.environ, LC_ALL="C")
    awk = subprocess.run(["awk", "-W", "version"], capture_output=True, env=env).stdout.decode().splitlines()
    runs = []
    last = regular(22, 5000, 30)
    for name, source, data, chr1, chr2 in (("jva", "jva", regular(21, 5000, 80), "1", "1"), ("jvq_01_1e3", "jvq", quirks(), "01", "1e3"),
                                           ("jvq_chrX", "jvq", quirks(), "chrX", "chrX"), ("jvn", "jvn", last[:-1], "chr2", "chr10"),
                                           ("jve", "jve", b"", "1", "2")):
        store(source + ".in.gz", data)
        made = run_old_script(utils, data, chr1, chr2, env)
        store(name + ".out.gz", made)
        runs.append(dict(name=name, mode="verbatim", input=source + ".in.gz", chr1=chr1, chr2=chr2, resolution=None, output=name + ".out.gz"))
        print("  wrote %s: %d bytes in, %d lines out" % (name, len(data), made.count(b"\n")))
    for name, data, chr1, chr2, res in (("jma_r5000", regular(23, 5000, 80), "1", "1", 5000), ("jmx_r5000", edges(5000), "1", "X", 5000),
                                        ("jmo_r10001", edges(10001), "2", "X", 10001),
                                        ("jmr_r2", b"0\t2147483646\t3\n2147483646\t2147483646\t1.0\n", "7", "7", 2)):
        store(name + ".in.gz", data)
        made, stdout = run_py(utils, data, chr1, chr2, res, env)
        store(name + ".out.gz", made)
        runs.append(dict(name=name, mode="midpoint", input=name + ".in.gz", chr1=chr1, chr2=chr2, resolution=res, output=name + ".out.gz",
                         stdout=stdout))
        print("  wrote %s: %d bytes in, %d lines out" % (name, len(data), made.count(b"\n")))
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(dict(awk=awk[0] if awk else "unknown", locale="LC_ALL=C", runs=runs), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
