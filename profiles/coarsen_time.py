#!/usr/bin/env python3
"""Stage times of the coarsening (fithic_amd.coarsen, csrc/fhx_coarsen.hip) from a resident ValidPairs, on the synthetic
allValidPairs file of profiles/validpairs_time.py (the one profiles/fragpairs_time.py bins): the file is binned once at 10 kb and
its cells, which stay in HBM, are summed onto 2 and 8 times coarser bins.  Beside each stands the only other route to the same
cells: validpairs.read(path, N * R) on the same file, another pass over the text.  One JSON line on stdout.

    python profiles/coarsen_time.py [--lines 4000000] [--runs 5]

upload / keys / sort / heads_sums / cells / plan are the host clocks fhx_cz_stage_seconds returns (taken around stream
synchronisations); `call` is coarsen.read as a whole (the host plan, a new handle and the plan's upload included), `reread_call`
validpairs.read as a whole.  Every figure is the median of --runs calls after one call that is not counted (it pays for the code
objects and the pinned buffers).  The two routes do not give the same cells on every input - the script's distance filter sits in
front of the binning - so the cell counts of both are printed, not compared.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LENGTH = 150000000                                                   # of each of the file's three chromosomes


def median_of(runs):
    return {k: statistics.median(r[k] for r in runs) for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=4000000)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import validpairs_time
    from fithic_amd import coarsen, tables, validpairs
    res = validpairs_time.RES
    out = {"metric": "resident contact counts -> N-fold coarser bins (fithic_amd.coarsen) beside validpairs.read at N * R", "res": res,
           "runs": args.runs, "factors": {}}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "s.allValidPairs")
        out["bytes"] = validpairs_time.make_input(src, args.lines)
        with validpairs.read(src, res) as fine:
            out["fine_cells"] = len(fine)
            n_bins = LENGTH // res + 1
            table = (np.repeat(np.arange(len(fine.names)), n_bins).astype(np.int32),
                     np.tile(np.arange(n_bins, dtype=np.int64) * res + res // 2, len(fine.names)).astype(np.int32),
                     np.ones(n_bins * len(fine.names), np.int32))
            out["fine_loci"] = len(table[1])
            for factor in (2, 8):
                resident, reread = [], []
                for k in range(args.runs + 1):
                    chroms = tables.ChromIndex()
                    t0 = time.perf_counter()
                    with coarsen.read(fine, table, factor, res, chroms) as data:
                        call = time.perf_counter() - t0
                        resident.append(dict(data.stage_seconds(), call=call))
                        cells = len(data)
                    t0 = time.perf_counter()
                    with validpairs.read(src, res * factor) as direct:
                        call = time.perf_counter() - t0
                        reread.append(dict(direct.stage_seconds(), reread_call=call))
                        reread_cells = len(direct)
                out["factors"][str(factor)] = {"cells": cells, "seconds": median_of(resident[1:]), "reread_cells": reread_cells,
                                               "reread_seconds": median_of(reread[1:])}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
