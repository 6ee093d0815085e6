#!/usr/bin/env python3
"""Stage times of the FDR subset (fithic_amd.mergefilter, csrc/fhx_sigselect.hip) on a synthetic significances text: rows as
`fithic` writes them (10 tab-separated columns, about 95 bytes), q in %e form.  One JSON line on stdout.

    python profiles/mergefilter_time.py [--lines 4000000]           read + upload / newline scan / select / gather / copy out on
                                                                    GPU 0 (the second of two runs), at about 1 % kept (fdr 0.05)
                                                                    and again at 100 % kept (fdr 5)
    python profiles/mergefilter_time.py --reference SCRIPT          no GPU: the filter pipeline of the reference's merge-filter.sh
                         [--lines 1000000]                          (zcat | awk | awk | gzip, its line 22, taken from SCRIPT as
                                                                    it stands) on a gzipped copy of the same text, one CPU core

The five native stages are the host clocks fhx_ms_stage_seconds returns (taken around stream synchronisations).
"""
import argparse
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_input(path, lines):
    """a header and `lines` rows; about 1 % of the q values lie at or below 0.05"""
    import numpy as np
    rng = np.random.default_rng(7)
    with open(path, "wb") as f:
        f.write(b"chr1\tfragmentMid1\tchr2\tfragmentMid2\tcontactCount\tp-value\tq-value\tbias1\tbias2\tExpCC\n")
        for lo in range(0, lines, 1 << 18):
            n = min(1 << 18, lines - lo)
            c = rng.integers(1, 23, n)
            b1 = rng.integers(0, 40000, n)
            b2 = b1 + rng.integers(4, 400, n)
            cc = rng.integers(1, 200, n)
            q = np.where(rng.random(n) < 0.01, 10 ** rng.uniform(-12, -1.31, n), rng.uniform(0.06, 1.0, n))
            f.write(b"".join(b"chr%d\t%d\tchr%d\t%d\t%d\t%e\t%e\t%.6f\t%.6f\t%.6f\n"
                             % (c[k], b1[k] * 5000 + 2500, c[k], b2[k] * 5000 + 2500, cc[k], q[k] / 40, q[k], 0.9, 1.1, cc[k] / 3) for k in range(n)))
    return os.path.getsize(path)


def reference_seconds(script, lines):
    with open(script) as f:
        pipeline = [ln for ln in f if ln.startswith("zcat ") and "fithic_subset.gz" in ln]
    if len(pipeline) != 1:
        sys.exit("%s: the filter pipeline (zcat ... > $outdir/fithic_subset.gz) was not found" % script)
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "sig.txt")
        nbytes = make_input(src, lines)
        with open(src, "rb") as f, gzip.open(src + ".gz", "wb", compresslevel=1) as g:
            shutil.copyfileobj(f, g)
        env = dict(os.environ, LC_ALL="C", inputFile=src + ".gz", fdr="0.05", outdir=tmp)
        cmd = ["bash", "-c", pipeline[0]]
        if shutil.which("taskset"):
            cmd = ["taskset", "-c", "0"] + cmd
        t0 = time.perf_counter()
        subprocess.run(cmd, env=env, check=True)
        dt = time.perf_counter() - t0
        with gzip.open(os.path.join(tmp, "fithic_subset.gz"), "rb") as f:
            kept = sum(chunk.count(b"\n") for chunk in iter(lambda: f.read(1 << 24), b""))
    return {"metric": "merge-filter.sh filter pipeline (reference, one CPU core)", "lines": lines, "bytes": nbytes, "kept": kept, "seconds": dt,
            "seconds_per_million_lines": dt / lines * 1e6}


def measure(lines):
    from fithic_amd import mergefilter
    out = {"metric": "significances -> FDR subset (fithic_amd.mergefilter)", "lines": lines}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "sig.txt")
        out["bytes"] = make_input(src, lines)
        for name, fdr in (("kept_1_percent", "0.05"), ("kept_100_percent", "5")):
            runs = []
            for _ in range(2):                                       # the first run pays for the pinned buffers and the code objects
                t0 = time.perf_counter()
                got = mergefilter.select(src, fdr)
                runs.append(dict(got.stage_seconds(), call=time.perf_counter() - t0))
            out[name] = {"fdr": fdr, "kept": got.n_kept, "subset_bytes": len(got.subset_text()), "seconds": runs[1], "first_call_seconds": runs[0],
                         "select_bytes_per_second": out["bytes"] / runs[1]["select"], "gather_bytes_per_second": len(got.subset_text()) / max(runs[1]["gather"], 1e-9)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="path of the reference's merge-filter.sh: time its filter pipeline on one CPU core instead")
    ap.add_argument("--lines", type=int, default=None)
    args = ap.parse_args()
    out = reference_seconds(args.reference, args.lines or 1000000) if args.reference else measure(args.lines or 4000000)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
