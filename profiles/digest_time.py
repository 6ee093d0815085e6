#!/usr/bin/env python3
"""Stage times of the digest path (fithic_amd.digest, csrc/fhx_digest.hip) on a synthetic genome: uniform random bases, 60-column
lines, 24 contigs of equal size.  One JSON line on stdout.

    python profiles/digest_time.py [--bases 3000000000] [--site hindiii] [--site ^GATC ...] [--keep-dir DIR]

The stages are the host clocks fhx_dg_stage_seconds returns (taken around stream synchronisations) of the second of two runs -
the first pays for the pinned buffers and the code objects - plus the two writers.  newline_scan is scan_text<TextModeBytes> with
its scan_tiles on the same text in the same call: the tree's yardstick for one streaming read of a text.  class_pass and sites
are the path's own kernels (dg_class; dg_walk counting, then storing).  file_read_seconds is a plain read of the same file into
host memory, page cache warm, for the share of the call that is I/O.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONTIGS, WIDTH = 24, 60


def make_genome(path, bases):
    import numpy as np
    rng = np.random.default_rng(20)
    letters = np.frombuffer(b"ACGT", np.uint8)
    per = bases // CONTIGS
    with open(path, "wb") as f:
        for c in range(CONTIGS):
            f.write(b">chr%d synthetic\n" % (c + 1))
            left = per
            while left > 0:
                n = min(left, WIDTH << 20)
                rows = -(-n // WIDTH)
                block = np.full((rows, WIDTH + 1), 10, np.uint8)
                block[:, :WIDTH] = letters[rng.integers(0, 4, rows * WIDTH, dtype=np.uint8)].reshape(rows, WIDTH)
                raw = block.tobytes()
                if n % WIDTH:                                        # the contig's last, shorter line
                    raw = raw[:len(raw) - 1 - (WIDTH - n % WIDTH)] + b"\n"
                f.write(raw)
                left -= n
    return os.path.getsize(path), per * CONTIGS


def file_read_seconds(path):
    t0 = time.perf_counter()
    with open(path, "rb", buffering=0) as f:
        buf = bytearray(64 << 20)
        while f.readinto(buf):
            pass
    return time.perf_counter() - t0


def measure(bases, sites, keep_dir):
    from fithic_amd import _capi, digest
    motifs = digest.parse_sites(sites)
    with tempfile.TemporaryDirectory(dir=keep_dir) as tmp:
        src = os.path.join(tmp, "genome.fa")
        nbytes, made = make_genome(src, bases)
        file_read_seconds(src)                                       # warm
        t_read = file_read_seconds(src)
        dg = _capi.DgContext(0)
        try:
            runs = []
            for _ in range(2):
                t0 = time.perf_counter()
                dg.digest_file(src, motifs)
                contig, position = dg.fetch_sites()
                runs.append(dict(dg.stage_seconds(), call=time.perf_counter() - t0))
            counts, lengths, names = dg.counts(), dg.lengths(), dg.names()
        finally:
            dg.close()
        t0 = time.perf_counter()
        _capi.dg_write_fragments(os.path.join(tmp, "frags.gz"), lengths, contig, position)
        t_frags = time.perf_counter() - t0
        t0 = time.perf_counter()
        _capi.dg_write_bed(os.path.join(tmp, "frags.bed"), names, lengths, contig, position)
        t_bed = time.perf_counter() - t0
    s = runs[1]
    kernels = s["class_pass"] + s["sites"]
    return {"metric": "FASTA -> cut sites -> fragments of fithic -r 0 (fithic_amd.digest)", "sites": sites, "motifs": len(motifs),
            "bases": made, "bytes": nbytes, "counts": counts, "seconds": s, "first_call_seconds": runs[0],
            "write_fragments_seconds": t_frags, "write_bed_seconds": t_bed, "file_read_seconds": t_read,
            "scan_text_bytes_per_second": nbytes / s["newline_scan"], "class_and_sites_bytes_per_second": nbytes / kernels,
            "class_and_sites_over_scan_text": kernels / s["newline_scan"], "call_over_file_read": s["call"] / t_read}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=3000000000)
    ap.add_argument("--site", action="append", help="a cut site or an enzyme's name; may be repeated (default: hindiii)")
    ap.add_argument("--keep-dir", help="make the temporary directory here (a file system with room for the genome)")
    args = ap.parse_args()
    print(json.dumps(measure(args.bases, args.site or ["hindiii"], args.keep_dir)), flush=True)


if __name__ == "__main__":
    main()
