#!/usr/bin/env python
"""Generate the end-to-end fixture of `fithic --significant FDR --significant-track --significant-split` under
tests/golden/significant_views/ by running the REAL reference.

    python tests/golden/make_golden_significant_views.py <path to the reference checkout (the directory that holds fithic/)>

The run is make_golden_significant.py's: the reference's fithic/fithic.py unmodified on the bundled hESC chr1 40 kb set (-r 40000
-p 2, bias file).  That it is the same run is asserted first: the reference's merge-filter.sh on the last pass's file at 1e-20
must reproduce the committed tests/golden/significant/fithic_subset.gz.  Then, under LC_ALL=C and on the same file at 1e-20,
fithic/utils/visualize-UCSC.sh and fithic/utils/merge-filter-parallelized.sh run unmodified.  Stored as DATA (no reference source
text is stored): the track, gzipped; the list the script makes (`chromosomes.used`, which it removes at its end: the same
`zcat | cut -f1 | sort | uniq` is run once more, and checked against the directories the script made); per listed name its job
line (the run's directory written as {OUTDIR}) and the md5 of its decompressed subset; cases.json, with the awk the scripts ran
with, because the selection and the score are awk's.  Not collected by pytest; the tests read only what this script wrote.
"""
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "significant_views")
SIGNIFICANT = os.path.join(HERE, "significant")
DATA = os.path.join(HERE, "data")


def main():
    ref = os.path.abspath(sys.argv[1])
    utils = os.path.join(ref, "fithic", "utils")
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(SIGNIFICANT, "cases.json")) as f:
        base = json.load(f)
    res, passes, fdr, lib, inputs = base["res"], base["passes"], base["fdr"], base["lib"], base["inputs"]
    env = dict(os.environ, LC_ALL="C", UTILITYFOLDER=utils.rstrip("/") + "/", MPLBACKEND="Agg")
    awk = subprocess.run(["awk", "-W", "version"], capture_output=True, env=env).stdout.decode().splitlines()
    with tempfile.TemporaryDirectory() as tmp:
        run = os.path.join(tmp, "run")
        subprocess.run([sys.executable, os.path.join(ref, "fithic", "fithic.py"), "-i", os.path.join(DATA, inputs["contacts"]),
                        "-f", os.path.join(DATA, inputs["frags"]), "-t", os.path.join(DATA, inputs["bias"]), "-o", run, "-r", str(res),
                        "-p", str(passes), "-l", lib], check=True, stdout=subprocess.DEVNULL, env=env, cwd=tmp)
        sig = os.path.join(run, "%s.spline_pass%d.res%d.significances.txt.gz" % (lib, passes, res))
        with gzip.open(sig, "rb") as f:
            sig_text = f.read()
        assert hashlib.md5(sig_text).hexdigest() == base["significances_md5"], "not the run of make_golden_significant.py"
        # the same run: the one-file script reproduces the committed subset
        subprocess.run(["bash", os.path.join(utils, "merge-filter.sh"), sig, str(res), os.path.join(tmp, "out", "merged.gz"), fdr, "ignored"],
                       env=env, cwd=tmp, capture_output=True, check=True)
        with gzip.open(os.path.join(tmp, "out", "fithic_subset.gz"), "rb") as f, gzip.open(os.path.join(SIGNIFICANT, base["subset"]), "rb") as g:
            subset = f.read()
            assert subset == g.read(), "merge-filter.sh does not reproduce tests/golden/significant/" + base["subset"]
        # the track
        track_path = os.path.join(tmp, "track.txt")
        subprocess.run(["bash", os.path.join(utils, "visualize-UCSC.sh"), sig, track_path, fdr], env=env, cwd=tmp, capture_output=True, check=True)
        with open(track_path, "rb") as f:
            track = f.read()
        # the tree
        outdir = os.path.join(tmp, "split")
        subprocess.run(["bash", os.path.join(utils, "merge-filter-parallelized.sh"), sig, str(res), outdir, fdr, ""], env=env, cwd=tmp,
                       capture_output=True, check=True)
        used = subprocess.run("zcat %s | cut -f1 | sort | uniq" % sig, shell=True, env=env, capture_output=True, check=True).stdout
        listed = used.decode().split("\n")[:-1]
        assert sorted(os.listdir(outdir)) == sorted(listed), (os.listdir(outdir), listed)
        chromosomes = {}
        for name in listed:
            with gzip.open(os.path.join(outdir, name, "subset_fithic_%s.gz" % name), "rb") as f:
                part = f.read()
            with open(os.path.join(outdir, name, "fithic_%s.job" % name)) as f:
                job = f.read()
            chromosomes[name] = dict(subset_md5=hashlib.md5(part).hexdigest(), subset_lines=part.count(b"\n"), job=job.replace(outdir, "{OUTDIR}"))
    with gzip.GzipFile(os.path.join(OUT, "track.txt.gz"), "wb", mtime=0) as f:
        f.write(track)
    with open(os.path.join(OUT, "chromosomes.used"), "wb") as f:
        f.write(used)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(dict(awk=awk[0] if awk else "unknown", locale="LC_ALL=C", inputs=inputs, res=res, passes=passes, fdr=fdr, lib=lib,
                       track="track.txt.gz", track_lines=track.count(b"\n"), track_md5=hashlib.md5(track).hexdigest(),
                       chromosomes_used="chromosomes.used", chromosomes=chromosomes), f, indent=1)
        f.write("\n")
    print("  wrote significant_views: %d track lines, %s" % (track.count(b"\n"), {k: v["subset_lines"] for k, v in chromosomes.items()}))


if __name__ == "__main__":
    main()
