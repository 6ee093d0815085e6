#!/usr/bin/env python
"""Generate the digest fixtures under tests/golden/digest/.

    python tests/golden/make_golden_digest.py <path to the reference's fithic/utils directory>

Step 1 of createFitHiCFragments-nonfixedsize.sh fetches HiC-Pro's digest_genome.py from the network and is never run: the bed
file of every run comes from the model (tests/digest_model.py, held to hand-written expectations by tests/test_digest_host.py).
Step 2 is the REAL loop: the lines of the reference's script from the one that begins `currChr=` to the end are copied into a
temporary script (checked to hold none of wget, http, python2), which runs under bash in a temporary directory with the model's
bed as bedfile.txt and `outfile` set.  What it leaves (the gunzipped $outfile.gz) and what it prints are stored as DATA, gzipped;
no reference source text is stored.  Not collected by pytest; the tests read only what this script wrote.

  dga   HindIII on three wrapped contigs of random bases with planted sites, one of them across a line end
  dgq   ^GATC on the quirks: text before the first header, a description behind the name, mixed case, N in the genome, \\r\\n
        lines, empty lines, an empty contig, a site at 0 and one that ends the contig, no newline after the last line
  dg2   BglII and DpnII together: A^GATCT and ^GATC cut every `agatct` at the same place, so equal sites, also across a line end
  dgn   G^ANTC, the N expanded, on gaatc / gantc / GAcTC and names with . _ -
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import digest_model as dm  # noqa: E402

OUT = os.path.join(HERE, "digest")


def wrapped(seq, width=60):
    return "".join(seq[k:k + width] + "\n" for k in range(0, len(seq), width))


def regular():
    rng = np.random.default_rng(31)
    text = ""
    for name, n in (("chr1", 1500), ("chr2", 733), ("chrX", 1201)):
        seq = "".join("ACGT"[k] for k in rng.integers(0, 4, n))
        for at in (57, 300, n - 6):                                     # 57: AAGCTT lies across the first line end
            seq = seq[:at] + "AAGCTT" + seq[at + 6:]
        text += ">%s\n%s" % (name, wrapped(seq))
    return text.encode()


def quirks():
    return (b"GATCGATC\nthis-is-not-a-contig\n>one first contig\nGATCaagaTCGA\r\ntcNGATC\r\n\r\n\nGAnTCgatc\n>empty\n>two\tdesc\n\nnnnn\n"
            b"gAtCgatC\n>three\nGA\nT\nC\n\nGATCGAT")


def doubles():
    return b">a\naagatcttagatctgatcgatc\naagatc\nt\n>b\ngatcagatct\n"


def expanded():
    return b">c.1_x-y\ngaatc\ngantc\nGAcTC\n>c2\nGAGTCGATTCG\nANTC\n"


def real_loop(utils, bed):
    """-> (the bytes of $outfile, stdout) of the script's own lines from `currChr=` on"""
    with open(os.path.join(utils, "createFitHiCFragments-nonfixedsize.sh")) as f:
        lines = f.readlines()
    first = [k for k, line in enumerate(lines) if line.startswith("currChr=")][0]
    tail = "".join(lines[first:])
    assert not any(word in tail for word in ("wget", "http", "python2")), tail
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "bedfile.txt"), "wb") as f:
            f.write(bed)
        with open(os.path.join(tmp, "loop.sh"), "w") as f:
            f.write(tail)
        r = subprocess.run(["bash", "loop.sh"], cwd=tmp, env=dict(os.environ, LC_ALL="C", outfile="frags"), capture_output=True, check=True)
        assert not os.path.exists(os.path.join(tmp, "bedfile.txt")) and not os.path.exists(os.path.join(tmp, "frags"))
        with gzip.open(os.path.join(tmp, "frags.gz"), "rb") as f:
            return f.read(), r.stdout.decode()


def store(name, data):
    with gzip.GzipFile(os.path.join(OUT, name), "wb", mtime=0) as f:
        f.write(data)


def main():
    utils = os.path.abspath(sys.argv[1])
    os.makedirs(OUT, exist_ok=True)
    runs = []
    for name, data, sites in (("dga", regular(), ["HindIII"]), ("dgq", quirks(), ["^GATC"]), ("dg2", doubles(), ["bglii", "DPNII"]),
                              ("dgn", expanded(), ["G^ANTC"])):
        assert dm.refusal(data) is None, (name, dm.refusal(data))
        bed = dm.bed(data, sites)
        made, said = real_loop(utils, bed)
        store(name + ".fa.gz", data)
        store(name + ".bed.gz", bed)
        store(name + ".frags.gz", made)
        runs.append(dict(name=name, sites=sites, fasta=name + ".fa.gz", bed=name + ".bed.gz", fragments=name + ".frags.gz", stdout=said))
        print("  wrote %s: %d bytes in, %d fragments" % (name, len(data), made.count(b"\n")))
    with open(os.path.join(OUT, "cases.json"), "w") as f:
        json.dump(dict(locale="LC_ALL=C", runs=runs), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
