#!/usr/bin/env python3
"""Stage times of the HiC-Pro converter (fithic_amd.hicpro, csrc/fhx_hicpro.hip) on a synthetic sorted matrix of synth.py's C2
shape (one 249 Mb chromosome at 40 kb, no distance bounds: 1.26e7 lines `i<TAB>j<TAB>count`).  One JSON line on stdout.

    python profiles/hicpro_time.py                          upload / scan / parse + accumulate / fetch + contacts write /
                                                            fragments + bias, on GPU 0
    python profiles/hicpro_time.py --reference PATH         no GPU: the reference's HiCPro2FitHiC.py (loaded from PATH) on the
                         [--lines 1000000]                  first --lines lines of the same matrix, for the CPU comparison

The three native stages are the ones fhx_hp_parse_matrix reports under FHX_TIMING=1 (host clock around stream synchronisations).
"""
import argparse
import contextlib
import gzip
import io
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES, LENGTH, KEEP = 40000, 249250621, 0.52                           # bench.py's C2


def make_inputs(tmp, lines=None):
    """bed, matrix, bias files of the C2 shape -> (paths, number of matrix lines, matrix bytes)"""
    import numpy as np
    import pandas as pd
    import torch
    from fithic_amd import synth
    genome = synth.Genome(RES, [LENGTH])
    n = genome.n_loci[0]
    amp = synth.solve_amplitude(KEEP, 1, n - 1)
    device = "cuda" if torch.cuda.is_available() else "cpu"
    _, mid1, _, mid2, count = synth.cis_contacts(genome, 0, 0, n - 1, amp, device=device)
    i = (mid1.cpu().numpy() // RES + 1)[:lines]
    j = (mid2.cpu().numpy() // RES + 1)[:lines]
    c = count.cpu().numpy()[:lines]
    paths = [os.path.join(tmp, name) for name in ("c2_abs.bed", "c2.matrix", "c2.biases")]
    with open(paths[0], "w") as f:
        f.write("".join("chr1\t%d\t%d\t%d\n" % (k * RES, min((k + 1) * RES, LENGTH), k + 1) for k in range(n)))
    pd.DataFrame({"i": i, "j": j, "c": c}).to_csv(paths[1], sep="\t", header=False, index=False)
    b = genome.bias(0)
    b[np.arange(n) % 97 == 5] = np.nan
    with open(paths[2], "w") as f:
        f.write("".join("nan\n" if v != v else "%r\n" % float(v) for v in b))
    return paths, len(i), os.path.getsize(paths[1])


def reference_seconds(path, lines):
    import importlib.util
    spec = importlib.util.spec_from_file_location("HiCPro2FitHiC_reference", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    with tempfile.TemporaryDirectory() as tmp:
        (bed, matrix, bias), n, nbytes = make_inputs(tmp, lines)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            ref.outputfithicform(bed, matrix, os.path.join(tmp, "c.gz"), os.path.join(tmp, "f.gz"), bias, os.path.join(tmp, "b.gz"), 0)
        dt = time.perf_counter() - t0
    return {"metric": "HiCPro2FitHiC.py (reference, one CPU core)", "lines": n, "matrix_bytes": nbytes, "seconds": dt, "lines_per_second": n / dt}


def measure():
    os.environ["FHX_TIMING"] = "1"
    from fithic_amd import _capi, hicpro
    with tempfile.TemporaryDirectory() as tmp:
        (bed, matrix, bias), n, nbytes = make_inputs(tmp)
        with open(matrix, "rb") as f:                                # the file is in the page cache, as after HiC-Pro wrote it
            while f.read(1 << 26):
                pass
        b = hicpro.read_bed(bed)
        hp = _capi.HpContext(0)
        hp.load_bins(b.index_base, b.chr_id, b.mid)
        native = []
        for run in range(2):                                         # the first run pays for the pinned buffers and the code objects
            log = os.path.join(tmp, "stderr.txt")
            sys.stderr.flush()
            saved = os.dup(2)
            fd = os.open(log, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
            os.dup2(fd, 2)
            try:
                t0 = time.perf_counter()
                rows = hp.parse_matrix(matrix)
                t_call = time.perf_counter() - t0
            finally:
                os.dup2(saved, 2)
                os.close(fd)
                os.close(saved)
            m = re.search(r"upload ([0-9.]+) s; scan ([0-9.]+) s; parse \+ accumulate ([0-9.]+) s", open(log).read())
            native.append(dict(upload=float(m.group(1)), scan=float(m.group(2)), parse_accumulate=float(m.group(3)), call=t_call))
        assert rows == n
        t0 = time.perf_counter()
        cols = hp.fetch_rows()
        t_fetch = time.perf_counter() - t0
        t0 = time.perf_counter()
        _capi.host_write_contacts(os.path.join(tmp, "fithic.interactionCounts.gz"), b.chroms.names, *cols)
        t_write = time.perf_counter() - t0
        t0 = time.perf_counter()
        frag = hicpro.fragments_lines(b, hp.totals())
        with gzip.open(os.path.join(tmp, "fithic.fragmentMappability.gz"), "wt") as f:
            f.write("".join(frag))
        text = hicpro.bias_lines(b, hicpro.convert_bias(bias))
        with gzip.open(os.path.join(tmp, "fithic.biases.gz"), "wt") as f:
            f.write("".join(text))
        t_small = time.perf_counter() - t0
        hp.close()
    s = native[1]
    return {"metric": "HiC-Pro matrix -> Fit-Hi-C inputs (fithic_amd.hicpro)", "lines": n, "matrix_bytes": nbytes, "bins": b.n_slots,
            "seconds": {"upload": s["upload"], "scan": s["scan"], "parse_accumulate": s["parse_accumulate"], "fetch": t_fetch,
                        "contacts_write": t_write, "fragments_and_bias": t_small},
            "first_call_seconds": native[0], "parse_matrix_call_seconds": s["call"],
            "scan_bytes_per_second": nbytes / s["scan"], "parse_bytes_per_second": nbytes / s["parse_accumulate"],
            "parse_lines_per_second": n / s["parse_accumulate"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="path of the reference's HiCPro2FitHiC.py: time it on the CPU instead")
    ap.add_argument("--lines", type=int, default=1000000)
    args = ap.parse_args()
    out = reference_seconds(args.reference, args.lines) if args.reference else measure()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
