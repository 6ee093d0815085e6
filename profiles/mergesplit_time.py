#!/usr/bin/env python3
"""Stage times of the per-chromosome FDR subsets (fithic_amd.mergefilter_parallel, csrc/fhx_sigsplit.inc) on a synthetic
significances text: rows as `fithic` writes them (10 tab-separated columns, about 95 bytes), q in %e form, 24 chromosomes.  One JSON
line on stdout.

    python profiles/mergesplit_time.py [--lines 4000000]            read + upload / newline scan / names + select / sort + gather /
                                                                    copy out on GPU 0 (the second of two runs), at about 1 % kept
                                                                    (fdr 0.05) and at 100 % kept (fdr 5), on a file sorted by
                                                                    chromosome and on one with the chromosomes interleaved line by
                                                                    line; beside each, mergefilter.select on the same file, and
                                                                    the ratio of the two calls
    python profiles/mergesplit_time.py --reference SCRIPT           no GPU: the reference's merge-filter-parallelized.sh as it
                         [--lines 1000000]                          stands (one pipeline over the whole file per chromosome) on a
                                                                    gzipped copy of the sorted text, one CPU core

The five native stages are the host clocks fhx_ms_split_stage_seconds returns (taken around stream synchronisations).
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

NAMES = [b"chr%d" % k for k in range(1, 23)] + [b"chrX", b"chrY"]


def make_input(path, lines, interleaved):
    """a header and `lines` cis rows over 24 chromosomes, sorted by chromosome or interleaved line by line; about 1 % of the q values
    lie at or below 0.05"""
    import numpy as np
    rng = np.random.default_rng(7)
    with open(path, "wb") as f:
        f.write(b"chr1\tfragmentMid1\tchr2\tfragmentMid2\tcontactCount\tp-value\tq-value\tbias1\tbias2\tExpCC\n")
        for lo in range(0, lines, 1 << 18):
            n = min(1 << 18, lines - lo)
            row = np.arange(lo, lo + n)
            c = row % 24 if interleaved else row * 24 // lines
            b1 = rng.integers(0, 40000, n)
            b2 = b1 + rng.integers(4, 400, n)
            cc = rng.integers(1, 200, n)
            q = np.where(rng.random(n) < 0.01, 10 ** rng.uniform(-12, -1.31, n), rng.uniform(0.06, 1.0, n))
            f.write(b"".join(b"%s\t%d\t%s\t%d\t%d\t%e\t%e\t%.6f\t%.6f\t%.6f\n"
                             % (NAMES[c[k]], b1[k] * 5000 + 2500, NAMES[c[k]], b2[k] * 5000 + 2500, cc[k], q[k] / 40, q[k], 0.9, 1.1, cc[k] / 3)
                             for k in range(n)))
    return os.path.getsize(path)


def reference_seconds(script, lines):
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "sig.txt")
        nbytes = make_input(src, lines, interleaved=False)
        with open(src, "rb") as f, gzip.open(src + ".gz", "wb", compresslevel=1) as g:
            shutil.copyfileobj(f, g)
        cmd = ["bash", os.path.abspath(script), "sig.txt.gz", "5000", "out", "0.05", "utils/"]
        if shutil.which("taskset"):
            cmd = ["taskset", "-c", "0"] + cmd
        t0 = time.perf_counter()
        subprocess.run(cmd, env=dict(os.environ, LC_ALL="C"), cwd=tmp, check=True)
        dt = time.perf_counter() - t0
        folders = sorted(os.listdir(os.path.join(tmp, "out")))
        kept = 0
        for c in folders:
            with gzip.open(os.path.join(tmp, "out", c, "subset_fithic_%s.gz" % c), "rb") as f:
                kept += sum(chunk.count(b"\n") for chunk in iter(lambda: f.read(1 << 24), b""))
    return {"metric": "merge-filter-parallelized.sh (reference, one CPU core; the job files are written, not run)", "lines": lines, "bytes": nbytes,
            "chromosomes": len(folders), "kept": kept, "seconds": dt, "seconds_per_million_lines": dt / lines * 1e6}


def measure(lines):
    from fithic_amd import mergefilter, mergefilter_parallel
    out = {"metric": "significances -> per-chromosome FDR subsets (fithic_amd.mergefilter_parallel)", "lines": lines}
    with tempfile.TemporaryDirectory() as tmp:
        for layout in ("file_sorted", "line_interleaved"):
            src = os.path.join(tmp, layout + ".txt")
            out["bytes"] = make_input(src, lines, layout == "line_interleaved")
            for name, fdr in (("kept_1_percent", "0.05"), ("kept_100_percent", "5")):
                runs, selects = [], []
                for _ in range(2):                                   # the first run pays for the pinned buffers, the sorter and the code objects
                    t0 = time.perf_counter()
                    got = mergefilter_parallel.split(src, fdr)
                    runs.append(dict(got.stage_seconds(), call=time.perf_counter() - t0))
                    t0 = time.perf_counter()
                    one = mergefilter.select(src, fdr)
                    selects.append(dict(one.stage_seconds(), call=time.perf_counter() - t0))
                kept = sum(got.n_kept(c) for c in got.chromosomes)
                assert kept == one.n_kept
                out[layout + "." + name] = {"fdr": fdr, "chromosomes": len(got.chromosomes), "kept": kept, "split_seconds": runs[1],
                                            "split_first_call_seconds": runs[0], "select_seconds": selects[1],
                                            "split_over_select": sum(runs[1][k] for k in runs[1] if k != "call") /
                                            sum(selects[1][k] for k in selects[1] if k != "call"),
                                            "sort_gather_under_upload": runs[1]["sort_gather"] < runs[1]["read_upload"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="path of the reference's merge-filter-parallelized.sh: time it on one CPU core instead")
    ap.add_argument("--lines", type=int, default=None)
    args = ap.parse_args()
    out = reference_seconds(args.reference, args.lines or 1000000) if args.reference else measure(args.lines or 4000000)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
