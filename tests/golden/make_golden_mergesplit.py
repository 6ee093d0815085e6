#!/usr/bin/env python
"""Generate the per-chromosome merge-filter fixtures under tests/golden/mergesplit/ by running the REAL reference.

    python tests/golden/make_golden_mergesplit.py <path to the reference's fithic/utils directory>

utils/merge-filter-parallelized.sh runs unmodified under LC_ALL=C in a scratch directory, with relative paths typed (sig.gz,
out, utils/ - a link to that directory - so that the job lines hold nothing of the machine they were made on).  Every job line
the script wrote is then run as it stands, which calls the real CombineNearbyInteraction.py.  Stored as DATA (no reference
source text is stored): the inputs, and per run one <name>.tree.json that maps every directory the script made to its
decompressed subset, its job text and its decompressed postmerged file (null when the job failed and left none).  cases.json
records the awk the script ran with.  Not collected by pytest; the tests read only what this script wrote.

  msa        a header fithic would write, three sorted chromosomes of clusters (make_golden_mergefilter's shapes), blanks and
             tabs mixed after the first tab, trans rows, rows at, one mantissa unit below and one above fdr = 0.05
  msu_1e-5   chromosomes interleaved line by line, names 1 2 X 2L 10_random nan NAN, the chromosome Y only in trans rows (an
  msu_5      empty subset), the header's chr1 in no data row (an empty directory), the subnormal and overflow quirks of mfq;
             the same input at fdr = 1e-5 and at fdr = 5
  msn        a data row on line 1 whose chromosome occurs nowhere else, no newline after the last line
  mse        no row passes
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_mergefilter import HEADER, RES, clusters  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mergesplit")


def row(k, chrom, b1, b2, cc, q, chrom2=None):
    """one row: a tab after the chromosome, then this row's own mix of blanks and tabs"""
    sep = ["\t", " ", "  ", "\t ", " \t"][k % 5]
    q = q if isinstance(q, str) else "%e" % q
    p = "%e" % (float(q) / 50 if float(q) < float("inf") else 1e-9)
    cols = ["%d" % (b1 * RES + RES // 2), chrom2 or chrom, "%d" % (b2 * RES + RES // 2), "%d" % cc, p, q, "%.6f" % (0.8 + (k % 7) / 20),
            "%.6f" % (1.3 - (k % 5) / 20), "%.6f" % (cc / 3 + 0.25)]
    return chrom + "\t" + sep.join(cols)


def msa():
    rng = np.random.default_rng(13)

    def q_of(rng, k):
        special = {3: "5.000000e-02", 4: "4.999999e-02", 5: "5.000001e-02", 9: "0.000000e+00", 12: "3.251000e-112", 21: "5.000000e-02",
                   30: "1.000000e+00", 33: "4.999999e-02", 40: "5.000001e-02", 70: "5.000000e-02", 71: "5.000001e-02", 120: "4.999999e-02"}
        return special[k] if k in special else float(10 ** rng.uniform(-6, 0))
    lines = [HEADER.replace(" ", "\t")]
    for k, (chrom, b1, b2, cc, q) in enumerate(clusters(rng, ["chr1", "chr2", "chrX"], 6, q_of)):
        lines.append(row(k, chrom, b1, b2, cc, q))
        if k % 19 == 7:                                               # contacts between two chromosomes that pass: they go nowhere
            lines.append(row(k + 1, chrom, b1, b2 + 9, cc, "1.250000e-04", chrom2="chr2" if chrom != "chr2" else "chrX"))
    return ("\n".join(lines) + "\n").encode()


def msu():
    rng = np.random.default_rng(14)

    def q_of(rng, k):
        special = {0: "1.000000e-07", 2: "1.000000e-320", 3: "2.225074e-308", 4: "2.225073e-308", 6: "9.000000e-315", 8: "4.940656e-324",
                   10: "1.000000e-05", 11: "1.000001e-05", 12: "9.999999e-06", 14: "5.000000e+00", 15: "5.000001e+00", 16: "4.999999e+00",
                   20: "0.000000e+00", 25: "2.225074e-308", 26: "2.225073e-308", 27: "1.000000e-310", 31: "1.000000e+309",
                   32: "5.000000e+400", 33: "4.999999e+999"}
        return special[k] if k in special else float(10 ** rng.uniform(-9, 1))
    names = ["1", "2", "X", "2L", "10_random", "nan", "NAN"]
    per = {}
    for r in clusters(rng, names, 3, q_of):
        per.setdefault(r[0], []).append(r)
    lines, k = [HEADER.replace(" ", "\t")], 0
    for i in range(max(len(v) for v in per.values())):                # line by line: no two neighbours share a chromosome
        for name in names:
            if i < len(per[name]):
                lines.append(row(k, *per[name][i]))
                k += 1
        if i % 4 == 1:                                                # Y is seen in field 1 only with another chromosome in field 3
            lines.append(row(k, "Y", 30 + i, 90 + i, 50 + i, "1.000000e-08", chrom2="X"))
            k += 1
    return ("\n".join(lines) + "\n").encode()


def msn():
    rng = np.random.default_rng(15)
    rows = clusters(rng, ["chr4", "chr5", "chr6"], 4, lambda rng, k: float(10 ** rng.uniform(-5, 0)))
    lines = [row(2, "chr9", 10, 30, 40, "1.000000e-06")] + [row(k, *r) for k, r in enumerate(rows)]
    lines.append(row(1, "chr6", 900, 950, 77, "1.000000e-03"))        # the last line is kept and lacks its newline
    return "\n".join(lines).encode()


def mse():
    rng = np.random.default_rng(16)
    rows = clusters(rng, ["chr1", "chr2", "chr3"], 3, lambda rng, k: float(10 ** rng.uniform(-1.2, 0)))
    return ("\n".join([HEADER.replace(" ", "\t")] + [row(k, *r) for k, r in enumerate(rows)]) + "\n").encode()


def run_script(utils, data, fdr, env):
    """-> {directory name: {"subset": text, "job": text, "merged": text or None}} and what else the script left in OUTDIR"""
    with tempfile.TemporaryDirectory() as tmp:
        with gzip.open(os.path.join(tmp, "sig.gz"), "wb") as f:
            f.write(data)
        os.symlink(utils, os.path.join(tmp, "utils"))
        subprocess.run(["bash", "utils/merge-filter-parallelized.sh", "sig.gz", str(RES), "out", fdr, "utils/"], env=env, cwd=tmp,
                       capture_output=True, check=True)
        out = os.path.join(tmp, "out")
        tree, stray = {}, sorted(n for n in os.listdir(out) if not os.path.isdir(os.path.join(out, n)))
        for name in sorted(os.listdir(out)):
            folder = os.path.join(out, name)
            if not os.path.isdir(folder):
                continue
            job = os.path.join(folder, "fithic_%s.job" % name)
            done = subprocess.run(["bash", job], env=env, cwd=tmp, capture_output=True)
            merged_path = os.path.join(folder, "postmerged_fithic_%s.gz" % name)
            merged = None
            if done.returncode == 0 and os.path.exists(merged_path):
                with gzip.open(merged_path, "rb") as f:
                    merged = f.read().decode("latin-1")
            with gzip.open(os.path.join(folder, "subset_fithic_%s.gz" % name), "rb") as f:
                subset = f.read().decode("latin-1")
            with open(job) as f:
                job_text = f.read()
            files = sorted(os.listdir(folder))
            tree[name] = dict(subset=subset, job=job_text, merged=merged, job_exit=done.returncode, files=files)
        return tree, stray


def main():
    utils = os.path.abspath(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    env = dict(os.environ, LC_ALL="C")
    awk = subprocess.run(["awk", "-W", "version"], capture_output=True, env=env).stdout.decode().splitlines()
    runs = []
    for name, make, fdr in (("msa", msa, "0.05"), ("msu_1e-5", msu, "1e-5"), ("msu_5", msu, "5"), ("msn", msn, "0.05"), ("mse", mse, "0.05")):
        data = make()
        source = name.split("_")[0] + ".in.gz"
        with gzip.GzipFile(os.path.join(OUT, source), "wb", mtime=0) as f:
            f.write(data)
        tree, stray = run_script(utils, data, fdr, env)
        with open(os.path.join(OUT, name + ".tree.json"), "w") as f:
            json.dump(tree, f, indent=1, sort_keys=True)
            f.write("\n")
        runs.append(dict(name=name, input=source, fdr=fdr, res=RES, tree=name + ".tree.json", outdir="out", utilityfolder="utils/",
                         left_in_outdir=stray))
        print("  wrote %s: %d lines in; %s" % (name, len(data.splitlines()), ", ".join(
            "%s %d kept%s" % (c, t["subset"].count("\n"), "" if t["merged"] is not None else " (job failed)") for c, t in sorted(tree.items()))))
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(dict(awk=awk[0] if awk else "unknown", locale="LC_ALL=C", runs=runs), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
