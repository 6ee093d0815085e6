#!/usr/bin/env python
"""Generate the end-to-end fixture of `fithic --significant` under tests/golden/significant/ by running the REAL reference.

    python tests/golden/make_golden_significant.py <path to the reference checkout (the directory that holds fithic/)>

The reference's fithic/fithic.py runs unmodified on the bundled hESC chr1 40 kb set (tests/golden/data: contacts, fragments and
bias file; -r 40000 -p 2), then its fithic/utils/merge-filter.sh runs unmodified under LC_ALL=C (UTILITYFOLDER exported as the
utils directory plus a trailing slash) on the LAST pass's significances file at fdr = 1e-20 - about 6.5e3 rows pass, which the
script's CombineNearbyInteraction.py merges in half a minute.  The decompressed fithic_subset.gz and the decompressed merged file
are stored as DATA (no reference source text is stored); cases.json records the arguments, the counts and the awk the script ran
with, because the selection is awk's.  Not collected by pytest; the tests read only what this script wrote.
"""
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "significant")
DATA = os.path.join(HERE, "data")
RES, PASSES, FDR, LIB = 40000, 2, "1e-20", "hesc"


def store(name, data):
    with gzip.GzipFile(os.path.join(OUT, name), "wb", mtime=0) as f:
        f.write(data)


def main():
    ref = os.path.abspath(sys.argv[1])
    utils = os.path.join(ref, "fithic", "utils")
    os.makedirs(OUT, exist_ok=True)
    env = dict(os.environ, LC_ALL="C", UTILITYFOLDER=utils.rstrip("/") + "/", MPLBACKEND="Agg")
    awk = subprocess.run(["awk", "-W", "version"], capture_output=True, env=env).stdout.decode().splitlines()
    inputs = dict(contacts="hESC_chr1_w40000.contacts.gz", frags="hESC_chr1_w40000.frags.gz", bias="hESC_chr1_w40000.bias.gz")
    with tempfile.TemporaryDirectory() as tmp:
        run = os.path.join(tmp, "run")
        subprocess.run([sys.executable, os.path.join(ref, "fithic", "fithic.py"), "-i", os.path.join(DATA, inputs["contacts"]),
                        "-f", os.path.join(DATA, inputs["frags"]), "-t", os.path.join(DATA, inputs["bias"]), "-o", run, "-r", str(RES),
                        "-p", str(PASSES), "-l", LIB], check=True, stdout=subprocess.DEVNULL, env=env, cwd=tmp)
        sig = os.path.join(run, "%s.spline_pass%d.res%d.significances.txt.gz" % (LIB, PASSES, RES))
        with gzip.open(sig, "rb") as f:
            sig_text = f.read()
        merged_path = os.path.join(tmp, "out", "merged.gz")
        subprocess.run(["bash", os.path.join(utils, "merge-filter.sh"), sig, str(RES), merged_path, FDR, "ignored"], env=env, cwd=tmp,
                       capture_output=True, check=True)
        with gzip.open(os.path.join(tmp, "out", "fithic_subset.gz"), "rb") as f:
            subset = f.read()
        with gzip.open(merged_path, "rb") as f:
            merged = f.read()
    store("fithic_subset.gz", subset)
    store("merged.gz", merged)
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(dict(awk=awk[0] if awk else "unknown", locale="LC_ALL=C", inputs=inputs, res=RES, passes=PASSES, fdr=FDR, lib=LIB,
                       significances_lines=sig_text.count(b"\n"), significances_md5=hashlib.md5(sig_text).hexdigest(),
                       kept=subset.count(b"\n"), merged_records=len(merged.splitlines()) - 1, subset="fithic_subset.gz", merged="merged.gz"),
                  f, indent=1)
        f.write("\n")
    print("  wrote significant: %d lines in the last pass's file, %d kept, %d merged" % (sig_text.count(b"\n"), subset.count(b"\n"),
                                                                                       len(merged.splitlines()) - 1))


if __name__ == "__main__":
    main()
