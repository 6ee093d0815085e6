#!/usr/bin/env python3
"""The FDR subset of a pass, two routes on the same rows of the same GPU 0, one JSON line per run on stdout:

  parent   the pass writes <prefix>.significances.txt.gz (fhx_write_significances_device: format + deflate + copy out + write),
           then fithic_amd.mergefilter.select reads it back (inflate + upload + newline scan + select + gather): wall time of
           both and select's stage_seconds
  direct   Engine.significant on the resident q (csrc/fhx_sigresident.hip): wall time of the call and the host clocks the
           library takes around its stages under FHX_TIMING (decide, rank scans, rows + ExpCC/bias, measure + format, copy out)

    python profiles/significant_time.py [--shape synth4m|C3] [--fdr 0.05] [--tmp DIR]

synth4m is the C3 generator (5 kb loci, -L 20000 -U 2000000) on two chromosomes that give about 4e6 contact rows, the size
profiles/mergefilter_time.py uses; C3 is the whole genome of bench.py (1.48e8 rows, 3.8 GB of gzip in --tmp).  Both routes must
give the same bytes or the script stops.  The second of two runs of each route is reported (the first pays for code objects
and pinned buffers)."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"synth4m": [40_000_000, 36_600_000], "C3": None}
STAGES = ("decide", "rank_scans", "rows_extras", "measure_format", "copy_out")
_LINE = re.compile(r"decide ([0-9.]+) s; rank scans ([0-9.]+) s; rows \+ ExpCC/bias ([0-9.]+) s; measure \+ format ([0-9.]+) s; copy out ([0-9.]+) s")


def library_stderr(call):
    """call() with the process's stderr in a file -> (its result, what the library printed)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            out = call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return out, f.read().decode("latin-1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="synth4m")
    ap.add_argument("--fdr", default="0.05")
    ap.add_argument("--tmp", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from fithic_amd import mergefilter, synth
    from fithic_amd.engine import Engine
    cfg = dict(bench.CONFIGS["C3"])
    device = torch.device("cuda", 0)
    genome = synth.Genome(cfg["res"], SHAPES[args.shape])
    cols, n, _, _ = bench.build_rows(synth, torch, cfg, genome, list(range(len(genome))), 0, 1, device)
    eng = Engine(0)
    eng.configure(cfg["res"], cfg["L"], cfg["U"], n_bins=100, mapp_thres=1, mode=cfg["mode"])
    eng.load_fragments(*genome.fragments(), genome.sort_rank())
    eng.load_bias(*genome.bias_table())
    eng.load_contacts_device([t.data_ptr() for t in cols], n)
    eng.run_pass(collect=False)
    eng.ctx.sync()
    base = {"shape": args.shape, "rows": n, "fdr": args.fdr}
    with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
        path = os.path.join(tmp, "pass.significances.txt.gz")
        for _ in range(2):
            t0 = time.perf_counter()
            emitted, _ = eng.ctx.write_significances_device(path, genome.names)
            t1 = time.perf_counter()
            chosen = mergefilter.select(path, args.fdr)
            t2 = time.perf_counter()
        parent = dict(base, route="parent: write the file, select from it", emitted=emitted, kept=chosen.n_kept,
                      kept_fraction=chosen.n_kept / max(emitted, 1), file_bytes=os.path.getsize(path), write_seconds=t1 - t0,
                      select_seconds=t2 - t1, seconds=t2 - t0, select_stage_seconds=chosen.stage_seconds())
    print(json.dumps(parent), flush=True)
    for bracket in (True, False):
        os.environ.pop("FHX_SR_NO_BRACKET", None)
        if not bracket:
            os.environ["FHX_SR_NO_BRACKET"] = "1"
        os.environ["FHX_TIMING"] = "1"
        for _ in range(2):
            t0 = time.perf_counter()
            got, said = library_stderr(lambda: eng.significant(args.fdr, genome.names))
            dt = time.perf_counter() - t0
        del os.environ["FHX_TIMING"]
        if got.subset_text() != chosen.subset_text() or (got.n_lines, got.n_kept) != (chosen.n_lines, chosen.n_kept):
            sys.exit("the two routes differ")
        m = _LINE.search(said)
        print(json.dumps(dict(base, route="direct: resident q" + ("" if bracket else ", every q formatted (FHX_SR_NO_BRACKET=1)"),
                              emitted=got.n_lines - 1, kept=got.n_kept, kept_fraction=got.n_kept / max(got.n_lines - 1, 1), seconds=dt,
                              stage_seconds=dict(zip(STAGES, map(float, m.groups()))) if m else None, subset_bytes=len(got.subset_text()))),
              flush=True)
    os.environ.pop("FHX_SR_NO_BRACKET", None)
    eng.close()


if __name__ == "__main__":
    main()
