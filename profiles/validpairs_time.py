#!/usr/bin/env python3
"""Stage times of the validPairs path (fithic_amd.validpairs, csrc/fhx_validpairs.hip) on a synthetic allValidPairs file: read
pairs on three chromosomes of 150 Mb with a heavy-tailed distance, lines of about 100 bytes as HiC-Pro writes them.  One JSON
line on stdout.

    python profiles/validpairs_time.py [--lines 4000000]            read + upload / newline scan / parse / names + keys / sort /
                                                                    cells / fetch + write, on GPU 0 (the second of two runs)
    python profiles/validpairs_time.py --reference SCRIPT           no GPU: the reference's validPairs2FitHiC-fixedSize.sh on the
                         [--lines 1000000]                          first --lines lines of the same file, pinned to one CPU core

The six native stages are the host clocks fhx_vp_stage_seconds returns (taken around stream synchronisations).
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES = 10000


def make_input(path, lines):
    import numpy as np
    rng = np.random.default_rng(7)
    with open(path, "wb") as f:
        for lo in range(0, lines, 1 << 18):
            n = min(1 << 18, lines - lo)
            c1 = rng.integers(1, 4, n)
            c2 = np.where(rng.random(n) < 0.9, c1, rng.integers(1, 4, n))
            p1 = rng.integers(0, 150000000, n)
            p2 = np.where(c1 == c2, np.minimum(p1 + (rng.pareto(1.1, n) * 20000).astype(np.int64) % 100000000, 149999999), rng.integers(0, 150000000, n))
            f.write(b"".join(b"SRR1658570.%d\tchr%d\t%d\t+\tchr%d\t%d\t-\t%d\tHIC_chr%d_%d\tHIC_chr%d_%d\t42\t42\n"
                             % (lo + k, c1[k], p1[k], c2[k], p2[k], abs(p2[k] - p1[k]), c1[k], p1[k] // 4000, c2[k], p2[k] // 4000) for k in range(n)))
    return os.path.getsize(path)


def reference_seconds(script, lines):
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "s.allValidPairs")
        nbytes = make_input(src, lines)
        env = dict(os.environ, LC_ALL="C")
        if shutil.which("bc") is None:                               # the script asks bc for 2 * resolution
            with open(os.path.join(tmp, "bc"), "w") as f:
                f.write("#!/bin/sh\nIFS='*' read a b\necho $((a * b))\n")
            os.chmod(os.path.join(tmp, "bc"), 0o755)
            env["PATH"] = tmp + os.pathsep + env["PATH"]
        cmd = ["bash", script, str(RES), "lib", src, tmp]
        if shutil.which("taskset"):
            cmd = ["taskset", "-c", "0"] + cmd
        t0 = time.perf_counter()
        subprocess.run(cmd, env=env, check=True, stdout=subprocess.DEVNULL)
        dt = time.perf_counter() - t0
    return {"metric": "validPairs2FitHiC-fixedSize.sh (reference, one CPU core)", "lines": lines, "bytes": nbytes, "seconds": dt,
            "seconds_per_million_lines": dt / lines * 1e6}


def measure(lines):
    from fithic_amd import validpairs
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "s.allValidPairs")
        nbytes = make_input(src, lines)
        runs = []
        for _ in range(2):                                           # the first run pays for the pinned buffers and the code objects
            t0 = time.perf_counter()
            with validpairs.read(src, RES) as data:
                t_read = time.perf_counter() - t0
                stages, counts = data.stage_seconds(), data.counts()
                t0 = time.perf_counter()
                data.write(os.path.join(tmp, "lib_fithic.contactCounts.gz"))
                t_write = time.perf_counter() - t0
            runs.append(dict(stages, call=t_read, fetch_and_write=t_write))
    return {"metric": "allValidPairs -> contact counts (fithic_amd.validpairs)", "bytes": nbytes, **counts, "seconds": runs[1],
            "first_call_seconds": runs[0], "parse_lines_per_second": counts["lines"] / runs[1]["parse"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="path of the reference's validPairs2FitHiC-fixedSize.sh: time it on one CPU core instead")
    ap.add_argument("--lines", type=int, default=None)
    args = ap.parse_args()
    out = reference_seconds(args.reference, args.lines or 1000000) if args.reference else measure(args.lines or 4000000)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
