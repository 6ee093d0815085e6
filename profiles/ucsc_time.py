#!/usr/bin/env python3
"""Stage times of the UCSC interact track (fithic_amd.ucsc, csrc/fhx_sigtrack.inc) on the synthetic significances text of
profiles/mergefilter_time.py: rows as `fithic` writes them (10 tab-separated columns, about 95 bytes), q in %e form.  One JSON
line on stdout.

    python profiles/ucsc_time.py [--lines 4000000]                  read + upload / newline scan / select / deferred round trip /
                                                                    format / copy out on GPU 0 (the second of two runs), at about
                                                                    1 % kept (threshold 0.05) and again at 100 % kept (threshold 5),
                                                                    with n_deferred; and ms_select's stages on the same text in
                                                                    the same run, as the yardstick beside it
    python profiles/ucsc_time.py --reference SCRIPT                 no GPU: the pipeline of the reference's visualize-UCSC.sh
                         [--lines 1000000]                          (zcat | awk | awk, its line 18, taken from SCRIPT as it stands)
                                                                    on a gzipped copy of the same text, one CPU core, at 0.05 and at 5

The six native stages are the host clocks fhx_ms_track_stage_seconds returns (taken around stream synchronisations).
"""
import argparse
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mergefilter_time import make_input                              # noqa: E402


def reference_seconds(script, lines):
    with open(script) as f:
        pipeline = [ln for ln in f if ln.startswith("zcat ") and ">> $OUTPUT" in ln]
    if len(pipeline) != 1:
        sys.exit("%s: the track pipeline (zcat $INPUT | awk ... >> $OUTPUT) was not found" % script)
    out = {"metric": "visualize-UCSC.sh track pipeline (reference, one CPU core)", "lines": lines}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "sig.txt")
        out["bytes"] = make_input(src, lines)
        with open(src, "rb") as f, gzip.open(src + ".gz", "wb", compresslevel=1) as g:
            shutil.copyfileobj(f, g)
        for name, qval in (("kept_1_percent", "0.05"), ("kept_100_percent", "5")):
            track = os.path.join(tmp, "track.txt")
            if os.path.exists(track):
                os.remove(track)
            env = dict(os.environ, LC_ALL="C", INPUT=src + ".gz", OUTPUT=track, QVALTHRESH=qval)
            cmd = ["bash", "-c", pipeline[0]]
            if shutil.which("taskset"):
                cmd = ["taskset", "-c", "0"] + cmd
            t0 = time.perf_counter()
            subprocess.run(cmd, env=env, check=True)
            dt = time.perf_counter() - t0
            with open(track, "rb") as f:
                kept = sum(chunk.count(b"\n") for chunk in iter(lambda: f.read(1 << 24), b""))
            out[name] = {"qval": qval, "kept": kept, "track_bytes": os.path.getsize(track), "seconds": dt, "seconds_per_million_lines": dt / lines * 1e6}
    return out


def measure(lines):
    from fithic_amd import mergefilter, ucsc
    out = {"metric": "significances -> UCSC interact track (fithic_amd.ucsc)", "lines": lines}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "sig.txt")
        out["bytes"] = make_input(src, lines)
        for name, qval in (("kept_1_percent", "0.05"), ("kept_100_percent", "5")):
            runs = []
            for _ in range(2):                                       # the first run pays for the pinned buffers and the code objects
                t0 = time.perf_counter()
                got = ucsc.track(src, qval)
                runs.append(dict(got.stage_seconds(), call=time.perf_counter() - t0))
            subset = mergefilter.select(src, qval, strict=True)      # the yardstick: ms_select and ms_gather on the same text
            out[name] = {"qval": qval, "kept": got.n_kept, "n_deferred": got.n_deferred, "track_bytes": len(got.text()), "seconds": runs[1],
                         "first_call_seconds": runs[0], "select_bytes_per_second": out["bytes"] / runs[1]["select"],
                         "format_bytes_per_second": len(got.text()) / max(runs[1]["format"], 1e-9),
                         "ms_select_seconds": subset.stage_seconds()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="path of the reference's visualize-UCSC.sh: time its pipeline on one CPU core instead")
    ap.add_argument("--lines", type=int, default=None)
    args = ap.parse_args()
    out = reference_seconds(args.reference, args.lines or 1000000) if args.reference else measure(args.lines or 4000000)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
