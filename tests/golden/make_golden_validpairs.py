#!/usr/bin/env python
"""Generate the validPairs fixtures under tests/golden/validpairs/ by running the REAL reference.

    python tests/golden/make_golden_validpairs.py <path to the reference's fithic/utils directory>

utils/validPairs2FitHiC-fixedSize.sh and utils/createFitHiCFragments-fixedsize.py run unmodified, under LC_ALL=C, on the inputs
made below; the inputs, the decompressed outputs and what the programs printed are stored as DATA (no reference source text is
stored).  The script calls `bc` for one product (2 * resolution); where the machine has no bc, a stand-in that multiplies two
integers is written into a temporary directory that is put on PATH, and cases.json says so.  The awk the script ran with is
recorded there too: awk implementations differ in how they print large numbers and compare fields.  Not collected by pytest; the
tests read only what this script wrote.

  vpa  tab-separated lines as HiC-Pro writes them: pairs either side of the (pos1-pos2)^2 > 2*res edge, ends in both orders,
       chr2 / chr10 (string order) and 2 / 10 / X (numeric, then string), names of 5 and 6 bytes, chrM as a chromosome, inside a
       read name and in a trailing column, bin starts whose text order is not their numeric order, position 0, duplicates
  vpb  the same kinds of lines with extra columns, mixed tabs and blanks, leading blanks, \\r\\n line ends, no newline at the end
Each set is made for, and run at, res 10000 and res 50; vpa at 10000 also runs from a gzipped copy (zcat -f).
"""
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "validpairs")
BC_STAND_IN = "#!/bin/sh\n# stands in for `echo \"A*B\" | bc`: one product of two integers\nIFS='*' read a b\necho $((a * b))\n"


def edge(res):
    """the largest distance the script drops and the smallest it keeps: d*d > 2*res"""
    d = 0
    while (d + 1) ** 2 <= 2 * res:
        d += 1
    return d, d + 1


def pair_lines(res):
    """(name1, pos1, name2, pos2) of the pairs of one set; positions scale with res so that both resolutions bin alike"""
    lo, hi = edge(res)
    r = res
    rows = []
    for base in (0, 3 * r + 7, 12 * r + r // 2):                      # either side of the edge, both orders of the ends
        rows += [("chr1", base, "chr1", base + lo), ("chr1", base + lo, "chr1", base), ("chr1", base, "chr1", base + hi),
                 ("chr1", base + hi, "chr1", base), ("chr1", base + hi + 1, "chr1", base)]
    rows += [("chr1", 0, "chr1", 0), ("chr1", 0, "chr2", 0), ("chr2", 0, "chr1", 5)]                   # position 0
    for a, b in (("chr2", "chr10"), ("chr10", "chr2"), ("2", "10"), ("10", "2"), ("10", "X"), ("X", "10"), ("2", "X"), ("X", "2"),
                 ("chrX", "chr9"), ("chr9", "chrX"), ("9", "chr1"), ("chr1", "9"), ("_alt", "chr1"), ("Y", "X")):
        rows += [(a, 2 * r + 5, b, 10 * r + 9), (a, 10 * r + 9, b, 2 * r + 5)]
    for k in (2, 10, 100, 20, 1, 11, 9, 99, 1000, 19):                # bin starts k*res: "100000" sorts before "20000"
        rows += [("chr3", k * r + 1, "chr3", (k + 30) * r + 2), ("chr3", (k + 30) * r + 3, "chr3", k * r + 4), ("chr4", k * r, "chr3", 7 * r)]
    rows += [("chr10", 5 * r, "chr10", 9 * r), ("chr11_", 5 * r, "chr10", 9 * r), ("chr10", 5 * r, "chrUn_1", 9 * r),      # 5 and 6 bytes
             ("chrM", 100, "chr1", 5 * r), ("chr1", 5 * r, "chrM", 100), ("chrM", 100, "chrM", 9 * r)]
    rows += [("chr5", 7 * r + 1, "chr6", 8 * r + 2)] * 12 + [("chr6", 8 * r + 3, "chr5", 7 * r + 4)] * 5               # duplicates
    rows += [("chr5", 7 * r + k, "chr5", 20 * r + 2 * k) for k in range(40)]
    return rows


def vpa(res):
    out = []
    for k, (n1, p1, n2, p2) in enumerate(pair_lines(res)):
        read = "read%d" % k
        tail = "\t%d\tfrag%d\tfrag%d\t42\t42" % (abs(p2 - p1), k, k + 1)
        if k % 37 == 5:
            read = "SRR.chrM.%d" % k                                  # chrM inside the read name
        if k % 41 == 7:
            tail += "\tchrM_tag"                                      # chrM in a trailing column
        out.append("%s\t%s\t%d\t%s\t%s\t%d\t%s%s\n" % (read, n1, p1, "+-"[k % 2], n2, p2, "-+"[k % 3 % 2], tail))
    return "".join(out).encode()


def vpb(res):
    out = []
    for k, (n1, p1, n2, p2) in enumerate(pair_lines(res)):
        sep = ["\t", " ", "  ", " \t", "\t\t "][k % 5]
        lead = ["", " ", "\t"][k % 3]
        extra = ["", sep + "x", sep + "x" + sep + "y z", sep + "has_chrM_inside" if k % 29 == 3 else ""][k % 4]
        end = "\r\n" if k % 2 else "\n"
        out.append(lead + sep.join(["r%d" % k, n1, "%d" % p1, "+", n2, "%d" % p2]) + extra + end)
    text = "".join(out)
    return text.rstrip("\r\n").encode()                               # no newline at the end


def run_script(utils, data, res, env):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.validPairs")
        with open(path, "wb") as f:
            f.write(data)
        r = subprocess.run(["bash", os.path.join(utils, "validPairs2FitHiC-fixedSize.sh"), str(res), "lib", path, tmp], env=env,
                           capture_output=True, check=True)
        with gzip.open(os.path.join(tmp, "lib_fithic.contactCounts.gz"), "rb") as f:
            return f.read(), r.stdout.decode()


def run_fragments(utils, lens, res, env):
    with tempfile.TemporaryDirectory() as tmp:
        tmp = os.path.realpath(tmp)
        path, out = os.path.join(tmp, "chrom.sizes"), os.path.join(tmp, "frags.gz")
        with open(path, "w") as f:
            f.write(lens)
        r = subprocess.run([sys.executable, os.path.join(utils, "createFitHiCFragments-fixedsize.py"), "--chrLens", path, "--outFile", out,
                            "--resolution", str(res)], env=env, capture_output=True, check=True)
        with gzip.open(out, "rb") as f:
            return f.read(), r.stdout.decode().replace(tmp, "<DIR>")


def store(name, data):
    with gzip.GzipFile(os.path.join(OUT, name), "wb", mtime=0) as f:
        f.write(data)


def main():
    utils = sys.argv[1]
    os.makedirs(OUT, exist_ok=True)
    env = dict(os.environ, LC_ALL="C")
    with tempfile.TemporaryDirectory() as bindir:
        bc = "the machine's bc"
        if shutil.which("bc") is None:
            with open(os.path.join(bindir, "bc"), "w") as f:
                f.write(BC_STAND_IN)
            os.chmod(os.path.join(bindir, "bc"), 0o755)
            env["PATH"] = bindir + os.pathsep + env.get("PATH", "")
            bc = "a stand-in written by make_golden_validpairs.py (multiplies two integers)"
        awk = subprocess.run(["awk", "-W", "version"], capture_output=True, env=env).stdout.decode().splitlines()
        runs = []
        for res in (10000, 50):
            for name, make in (("vpa", vpa), ("vpb", vpb)):
                data = make(res)
                case = "%s_r%d" % (name, res)
                store(case + ".in.gz", data)
                out, said = run_script(utils, data, res, env)
                store(case + ".out.gz", out)
                runs.append(dict(name=case, input=case + ".in.gz", res=res, output=case + ".out.gz", stdout=said, gzipped_input=False))
                if case == "vpa_r10000":                              # the same text, handed over gzipped: zcat -f
                    out_gz, said = run_script(utils, gzip.compress(data, mtime=0), res, env)
                    assert out_gz == out
                    runs.append(dict(name=case + "_gz", input=case + ".in.gz", res=res, output=case + ".out.gz", stdout=said, gzipped_input=True))
                print("  wrote %s: %d bytes in, %d lines out" % (case, len(data), out.count(b"\n")))
        frags = []
        for name, res, lens in (("fr1", 10000, "chrA\t50000\nchrB\t45001\n3 9999\nchrD\t10000\n"), ("fr2", 25, "chr1\t60\nchr2\t75\nchr3\t1\n"),
                                ("fr3", 50, "chrX 149\n")):
            out, said = run_fragments(utils, lens, res, env)
            store(name + ".frags.out.gz", out)
            frags.append(dict(name=name, res=res, chr_lens=lens, output=name + ".frags.out.gz", stdout=said))
            print("  wrote %s" % name)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(dict(awk=awk[0] if awk else "unknown", locale="LC_ALL=C", bc=bc, runs=runs, fragments=frags), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
