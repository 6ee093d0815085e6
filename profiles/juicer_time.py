#!/usr/bin/env python3
"""Stage times of the Juicer dump path (fithic_amd.juicer, csrc/fhx_juicer.hip) on a synthetic dump: the records of a 5 kb map of
one chromosome of 250 Mb with a heavy-tailed distance, `binX \\t binY \\t count` as `juicer_tools dump observed NONE` prints them,
about 21 bytes a line.  One JSON line on stdout.

    python profiles/juicer_time.py [--lines 8000000]                read + upload / newline scan / parse / format / copy out of
                                                                    both modes on GPU 0 (the second of two runs), and the host's gzip
    python profiles/juicer_time.py --reference SCRIPT               no GPU: the reference's createFitHiCContacts-hic_old.sh on the
                         [--lines 1000000]                          first --lines lines of the same dump, pinned to one CPU core

The five native stages are the host clocks fhx_jc_stage_seconds returns (taken around stream synchronisations); jc_parse's bytes
are the dump's, jc_format's the output's.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RES = 5000


def make_input(path, lines):
    import numpy as np
    rng = np.random.default_rng(9)
    with open(path, "wb") as f:
        for lo in range(0, lines, 1 << 18):
            n = min(1 << 18, lines - lo)
            x = rng.integers(0, 50000, n)
            y = np.minimum(x + (rng.pareto(1.1, n) * 4).astype(np.int64) % 50000, 49999)
            c = 1 + (rng.pareto(1.3, n) * 3).astype(np.int64) % 100000
            f.write(b"".join(b"%d\t%d\t%d\n" % (x[k] * RES, y[k] * RES, c[k]) for k in range(n)))
    return os.path.getsize(path)


def reference_seconds(script, lines):
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "dump.txt")
        nbytes = make_input(src, lines)
        cmd = ["bash", script, src, "1", "1", os.path.join(tmp, "out.gz")]
        if shutil.which("taskset"):
            cmd = ["taskset", "-c", "0"] + cmd
        t0 = time.perf_counter()
        subprocess.run(cmd, env=dict(os.environ, LC_ALL="C"), check=True, stdout=subprocess.DEVNULL)
        dt = time.perf_counter() - t0
    return {"metric": "createFitHiCContacts-hic_old.sh (reference, one CPU core)", "lines": lines, "bytes": nbytes, "seconds": dt,
            "seconds_per_million_lines": dt / lines * 1e6}


def measure(lines):
    from fithic_amd import _capi, juicer
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "dump.txt")
        nbytes = make_input(src, lines)
        out = {"metric": "Juicer dump -> contact counts (fithic_amd.juicer)", "lines": lines, "bytes": nbytes}
        for mode, names, res in (("verbatim", ("1", "1"), 0), ("midpoint", ("chr1", "chr1"), RES)):
            jc = _capi.JcContext(0)
            try:
                runs = []
                for _ in range(2):                                   # the first run pays for the pinned buffers and the code objects
                    jc.reset()
                    t0 = time.perf_counter()
                    jc.convert_file(src, names[0], names[1], res)
                    runs.append(dict(jc.stage_seconds(), call=time.perf_counter() - t0))
                out_bytes = jc.counts()["bytes"]
                t0 = time.perf_counter()
                juicer._write(os.path.join(tmp, "out.gz"), jc.text(), True)
                t_gzip = time.perf_counter() - t0
            finally:
                jc.close()
            out[mode] = {"out_bytes": out_bytes, "seconds": runs[1], "first_call_seconds": runs[0], "host_gzip_seconds": t_gzip,
                         "jc_parse_bytes_per_second": nbytes / runs[1]["parse"], "jc_format_bytes_per_second": out_bytes / runs[1]["format"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="path of the reference's createFitHiCContacts-hic_old.sh: time it on one CPU core instead")
    ap.add_argument("--lines", type=int, default=None)
    args = ap.parse_args()
    out = reference_seconds(args.reference, args.lines or 1000000) if args.reference else measure(args.lines or 8000000)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
