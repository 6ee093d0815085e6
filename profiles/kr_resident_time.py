#!/usr/bin/env python
"""Time of the Knight-Ruiz biases inside a `fithic --kr` run against the protocol's two steps, on the C3-synth map (22 hg19
autosomes at 5 kb, 1.48e8 contact rows) or its first chromosomes, on one MI355X.

    python profiles/kr_resident_time.py [--chroms K] [--rounds R] [--dir DIR] [--reuse] [--no-cli]

  assembly   the matrix alone, alternating, R rounds: hickry.loadfastfithicInteractions on the two files (inflate + parse on the
             host cores, five columns uploaded, fhx_kr_load_pairs) against fhx_kr_load_loci + fhx_kr_load_pairs_resident on an engine
             that holds the rows from its own ingest.  The file route's code is the one the parent commit has.  The library's own
             stage clocks of the resident entry (FHX_TIMING=1) are printed once.
  cli        wall and stage clocks, alternating, R rounds: `fithic --kr -p 1` against `python -m fithic_amd.hickry` followed by
             `fithic -t -p 1` with its file; the output files of the two are compared.
Medians and the spread (min .. max) are printed as one JSON line per comparison.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_inputs(out, chroms):
    import numpy as np
    import pandas as pd
    import torch
    import bench
    from fithic_amd import synth, _capi
    cfg = dict(bench.CONFIGS["C3"])
    genome = synth.Genome(cfg["res"], synth.HG19_AUTOSOMES[:chroms] if chroms < 22 else None)
    cols_t, n, _, _ = bench.build_rows(synth, torch, cfg, genome, list(range(len(genome))), 0, 1, torch.device("cuda", 0))
    cols = [t[:n].cpu().numpy() for t in cols_t]
    del cols_t
    torch.cuda.empty_cache()
    _capi.host_write_contacts(out + "/contacts.gz", genome.names, *cols, gzip_level=1)
    names = np.array(genome.names)
    f_chr, f_mid, f_hits = genome.fragments()
    pd.DataFrame({0: names[f_chr], 1: 0, 2: f_mid, 3: f_hits, 4: 1}).to_csv(out + "/frags.gz", sep="\t", header=False, index=False, compression="gzip")
    open(out + "/rows.txt", "w").write(str(n))
    return n


def spread(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values), runs=len(values))


def assembly(out, res, rounds):
    import contextlib
    import io
    from fithic_amd import _capi, hickry, tables
    from fithic_amd.engine import Engine
    con, frg = out + "/contacts.gz", out + "/frags.gz"
    chroms = tables.ChromIndex()
    eng = Engine(0)

    def engine_of():
        eng.configure(res)
        return eng
    t0 = time.perf_counter()
    rows = tables.load_contacts(con, chroms, engine_of)
    t_ingest = time.perf_counter() - t0
    fc, fm, _ = tables.read_fragments(frg, chroms)
    t_file, t_res, shapes = [], [], set()
    for k in range(rounds + 1):                        # round 0 warms both routes up and is not counted
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            M, _ = hickry.loadfastfithicInteractions(con, frg)
        dt_file = time.perf_counter() - t0
        shapes.add(M.kr.shape()[:2])
        M.kr.close()
        kr = _capi.KrContext(0)
        if k == 1:
            os.environ["FHX_TIMING"] = "1"
        t0 = time.perf_counter()
        kr.load_loci(fc, fm)
        kr.load_pairs_resident(eng.ctx)
        dt_res = time.perf_counter() - t0
        os.environ.pop("FHX_TIMING", None)
        shapes.add(kr.shape()[:2])
        kr.close()
        if k:
            t_file.append(dt_file)
            t_res.append(dt_res)
    eng.close()
    assert len(shapes) == 1, shapes
    (n, nnz), = shapes
    print(json.dumps(dict(what="assembly of the Knight-Ruiz matrix", rows=len(rows), loci=n, cells=nnz, engine_ingest_seconds=t_ingest,
                          file_route_seconds=spread(t_file), resident_route_seconds=spread(t_res),
                          ratio_of_medians=statistics.median(t_file) / statistics.median(t_res))))


def md5_gz(path):
    pr = subprocess.run("gzip -dc %s | md5sum" % path, shell=True, executable="/bin/bash", capture_output=True, text=True)
    return pr.stdout.split()[0]


def cli(out, res, cfg, rounds):
    base = [sys.executable, "-m", "fithic_amd", "-i", out + "/contacts.gz", "-f", out + "/frags.gz", "-r", str(res), "-L", str(cfg["L"]),
            "-U", str(cfg["U"]), "-p", "1"]
    env = dict(os.environ, FHX_TIMING="1")
    walls = {"one": [], "two": [], "two_hickry": [], "two_fithic": []}
    stages = {}
    for k in range(rounds):
        t0 = time.time()
        r1 = subprocess.run(base + ["-o", out + "/one", "--kr", "--kr-output", out + "/one_bias.gz"], cwd=ROOT, capture_output=True, text=True, env=env)
        walls["one"].append(time.time() - t0)
        t0 = time.time()
        rh = subprocess.run([sys.executable, "-m", "fithic_amd.hickry", "-i", out + "/contacts.gz", "-f", out + "/frags.gz", "-o", out + "/two_bias.gz"],
                            cwd=ROOT, capture_output=True, text=True, env=env)
        walls["two_hickry"].append(time.time() - t0)
        t1 = time.time()
        r2 = subprocess.run(base + ["-o", out + "/two", "-t", out + "/two_bias.gz"], cwd=ROOT, capture_output=True, text=True, env=env)
        walls["two_fithic"].append(time.time() - t1)
        walls["two"].append(time.time() - t0)
        for tag, r in (("one", r1), ("hickry", rh), ("two", r2)):
            if r.returncode != 0:
                print(tag, "failed:", r.stderr[-2000:])
                return
            stages[tag] = [ln for ln in r.stdout.splitlines() + r.stderr.splitlines()
                           if ln.startswith("stage") or ln.startswith("fhx_kr_") or "took" in ln]
    sig = "/FitHiC.spline_pass1.res%d.significances.txt.gz" % res
    same = md5_gz(out + "/one" + sig) == md5_gz(out + "/two" + sig) and md5_gz(out + "/one_bias.gz") == md5_gz(out + "/two_bias.gz")
    same_log = open(out + "/one/FitHiC.fithic.log").read().replace(out + "/one", "") == open(out + "/two/FitHiC.fithic.log").read().replace(out + "/two", "")
    print(json.dumps(dict(what="fithic --kr -p 1 against hickry + fithic -t -p 1 (wall seconds)", one_command=spread(walls["one"]),
                          two_steps=spread(walls["two"]), of_which_hickry=spread(walls["two_hickry"]), of_which_fithic=spread(walls["two_fithic"]),
                          saved_seconds_of_medians=statistics.median(walls["two"]) - statistics.median(walls["one"]),
                          significances_and_bias_files_equal=same, logs_equal=same_log)))
    for tag in ("one", "hickry", "two"):
        print("  last run, %s:" % {"one": "fithic --kr", "hickry": "hickry", "two": "fithic -t"}[tag])
        for ln in stages[tag]:
            print("    " + ln)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chroms", type=int, default=22)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dir", default="/tmp/kr_resident_time")
    ap.add_argument("--reuse", action="store_true")
    ap.add_argument("--no-cli", action="store_true")
    args = ap.parse_args()
    import bench
    cfg = dict(bench.CONFIGS["C3"])
    out = args.dir
    os.makedirs(out, exist_ok=True)
    if not (args.reuse and all(os.path.exists(out + "/" + f) for f in ("contacts.gz", "frags.gz", "rows.txt"))):
        t0 = time.time()
        n = write_inputs(out, args.chroms)
        print("wrote %d contact rows (%.1f MB gz) in %.1f s; usable host cores %d" %
              (n, os.path.getsize(out + "/contacts.gz") / 1e6, time.time() - t0, len(os.sched_getaffinity(0))))
    sys.stdout.flush()
    assembly(out, cfg["res"], args.rounds)
    sys.stdout.flush()
    if not args.no_cli:
        cli(out, cfg["res"], cfg, args.rounds)


if __name__ == "__main__":
    main()
