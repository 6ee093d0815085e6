#!/usr/bin/env python3
"""Stage times of the fragment binning (fithic_amd.fragpairs, csrc/fhx_fragpairs.hip) on the synthetic allValidPairs file of
profiles/validpairs_time.py - read pairs on three chromosomes of 150 Mb with a heavy-tailed distance, lines of about 100 bytes -
over a table of 8e5 fragments cut at uniformly random sites.  One JSON line on stdout.

    python profiles/fragpairs_time.py [--lines 4000000] [--fragments 800000] [--fixed-size]

read + upload / newline scan / parse / sort / cells / table upload are the host clocks fhx_fp_stage_seconds returns (taken around
stream synchronisations), of the second of two runs.  --fixed-size also bins the SAME file with fithic_amd.validpairs at 10 kb in
the same process, so that fp_parse (a hash probe and a bisection per end) stands beside vp_parse (a division per end) on one text.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LENGTH = 150000000


def make_table(fragments):
    import numpy as np
    from fithic_amd import fragpairs
    rng = np.random.default_rng(11)
    per = [fragments // 3, fragments // 3, fragments - 2 * (fragments // 3)]
    ends = [np.r_[np.sort(rng.integers(1, LENGTH, n - 1)), LENGTH].astype(np.int32) for n in per]
    return fragpairs.Table([b"chr1", b"chr2", b"chr3"], np.r_[0, np.cumsum(per)], np.concatenate(ends))


def timed(read, write_to):
    runs = []
    for _ in range(2):                                               # the first run pays for the pinned buffers and the code objects
        t0 = time.perf_counter()
        with read() as data:
            t_read = time.perf_counter() - t0
            stages, counts = data.stage_seconds(), data.counts()
            t0 = time.perf_counter()
            data.write(write_to)
            t_write = time.perf_counter() - t0
        runs.append(dict(stages, call=t_read, fetch_and_write=t_write))
    return dict(counts, seconds=runs[1], first_call_seconds=runs[0], parse_lines_per_second=counts["lines"] / runs[1]["parse"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=4000000)
    ap.add_argument("--fragments", type=int, default=800000)
    ap.add_argument("--fixed-size", action="store_true", help="also bin the same file with fithic_amd.validpairs at 10 kb")
    args = ap.parse_args()
    import validpairs_time
    from fithic_amd import fragpairs, validpairs
    table = make_table(args.fragments)
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "s.allValidPairs")
        nbytes = validpairs_time.make_input(src, args.lines)
        out = {"metric": "allValidPairs -> contact counts between restriction fragments (fithic_amd.fragpairs)", "bytes": nbytes,
               "fragments": len(table), "coarse_index": "none", **timed(lambda: fragpairs.read(src, table), os.path.join(tmp, "frag.gz"))}
        if args.fixed_size:
            out["fixed_size"] = {"metric": "allValidPairs -> contact counts (fithic_amd.validpairs), the same file", "res": validpairs_time.RES,
                                 **timed(lambda: validpairs.read(src, validpairs_time.RES), os.path.join(tmp, "fixed.gz"))}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
