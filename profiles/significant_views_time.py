#!/usr/bin/env python3
"""The UCSC interact track and the per-chromosome FDR subsets of a pass, two routes on the same rows of the same GPU 0, one JSON
line per run on stdout:

  parent   the pass writes <prefix>.significances.txt.gz (fhx_write_significances_device: format + deflate + copy out + write),
           then fithic_amd.ucsc.track / fithic_amd.mergefilter_parallel.split read it back (inflate + upload + newline scan + the
           product's kernels): wall time of the write and of each product, and the product's stage_seconds
  direct   Engine.track / Engine.split on the resident q (csrc/fhx_sigresident_track.inc, fhx_sigresident_split.inc): wall time
           of the call and the host clocks the library takes around its stages under FHX_TIMING

    python profiles/significant_views_time.py [--shape synth4m|C3] [--fdr 0.05] [--tmp DIR]

The shapes are profiles/significant_time.py's: synth4m is the C3 generator on two chromosomes that give about 4e6 contact rows, C3
the whole genome of bench.py (1.48e8 rows, 3.8 GB of gzip in --tmp).  Both routes must give the same bytes or the script stops.
The second of two runs of each route is reported (the first pays for code objects, pinned buffers and the sort context)."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from significant_time import SHAPES, library_stderr  # noqa: E402

_SECONDS = re.compile(r"([a-zA-Z +/]+?) ([0-9.]+) s(?:;|\n|$)")


def stage_seconds(said, call):
    """{stage: seconds} of the line the library printed for `call`"""
    for line in said.splitlines():
        if line.startswith(call + ":"):
            return {name.strip().replace(" ", "_"): float(sec) for name, sec in _SECONDS.findall(line[line.index(": decide ") + 2:] + "\n")}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="synth4m")
    ap.add_argument("--fdr", default="0.05")
    ap.add_argument("--tmp", default=None)
    args = ap.parse_args()
    import torch
    import bench
    from fithic_amd import mergefilter_parallel, synth, ucsc
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
            lines = ucsc.track(path, args.fdr)
            t2 = time.perf_counter()
            parts = mergefilter_parallel.split(path, args.fdr)
            t3 = time.perf_counter()
        common = dict(base, emitted=emitted, file_bytes=os.path.getsize(path), write_seconds=t1 - t0)
    print(json.dumps(dict(common, route="parent track: write the file, ucsc.track of it", kept=lines.n_kept, deferred=lines.n_deferred,
                          product_seconds=t2 - t1, seconds=(t1 - t0) + (t2 - t1), product_stage_seconds=lines.stage_seconds())), flush=True)
    print(json.dumps(dict(common, route="parent split: write the file, mergefilter_parallel.split of it",
                          kept=sum(parts.n_kept(c) for c in parts.chromosomes), names=len(parts.chromosomes), product_seconds=t3 - t2,
                          seconds=(t1 - t0) + (t3 - t2), product_stage_seconds=parts.stage_seconds())), flush=True)
    os.environ["FHX_TIMING"] = "1"
    for _ in range(2):
        t0 = time.perf_counter()
        got, said = library_stderr(lambda: eng.track(args.fdr, genome.names))
        dt = time.perf_counter() - t0
    if got.text() != lines.text() or (got.n_lines, got.n_kept, got.n_deferred) != (lines.n_lines, lines.n_kept, lines.n_deferred):
        sys.exit("the two routes of the track differ")
    print(json.dumps(dict(base, route="direct track: resident q", emitted=got.n_lines - 1, kept=got.n_kept, deferred=got.n_deferred, seconds=dt,
                          stage_seconds=stage_seconds(said, "fhx_significant_track"), track_bytes=len(got.text()))), flush=True)
    for _ in range(2):
        t0 = time.perf_counter()
        got, said = library_stderr(lambda: eng.split(args.fdr, genome.names))
        dt = time.perf_counter() - t0
    if got.chromosomes != parts.chromosomes or got.n_lines != parts.n_lines or any(got.subset_text(c) != parts.subset_text(c) for c in parts.chromosomes):
        sys.exit("the two routes of the split differ")
    print(json.dumps(dict(base, route="direct split: resident q", emitted=got.n_lines - 1, kept=sum(got.n_kept(c) for c in got.chromosomes),
                          names=len(got.chromosomes), seconds=dt, stage_seconds=stage_seconds(said, "fhx_significant_split"),
                          subset_bytes=sum(len(got.subset_text(c)) for c in got.chromosomes))), flush=True)
    del os.environ["FHX_TIMING"]
    eng.close()


if __name__ == "__main__":
    main()
