"""createFitHiCFragments-fixedsize.py restated: the fixed-size fragments file `fithic` reads, one line per bin (reference:
fithic/utils/createFitHiCFragments-fixedsize.py), same flags, same prints, same bytes.

    python -m fithic_amd.fragments --chrLens chrom.sizes --outFile fragments.gz --resolution 10000

One line per bin and no arithmetic worth a kernel: plain Python.  `bins()` gives the same table as (chr ids, mids, hits) for
Engine.load_fragments, so that together with fithic_amd.validpairs.read(...).load_into() a run needs no intermediate file.
"""
import argparse
import gzip
import os

import numpy as np


def chrom_bins(path, res):
    """[(name, [bin starts])] in file order.  createFitHiCFragments-fixedsize.py:59-72: split(), int(size); a length that is no
    multiple of res ends at int((size + res) / res) * res - the last, shorter bin is a whole one."""
    out = []
    with open(path, "r") as fp:
        for line in fp:
            if line == "":
                continue
            t = line.rstrip().split()
            name, size = t[0], int(t[1])
            end = size if size % res == 0 else int((size + res) / res) * res
            out.append((name, range(0, end, res)))
    return out


def fragment_text(path, res):
    """the decompressed bytes of the fragments file (:73-79): lines joined by newlines, none after the last"""
    return "\n".join("%s\t%s\t%s\t1\t1" % (name, start, int(start + res / 2)) for name, starts in chrom_bins(path, res) for start in starts)


def bins(path, res, chroms):
    """(chr ids, mids, hits) as tables.read_fragments returns them for the written file; `chroms` is the run's ChromIndex"""
    ids, mids = [], []
    for name, starts in chrom_bins(path, res):
        mid = np.asarray([int(start + res / 2) for start in starts], np.int64)
        if mid.size and mid[-1] > (1 << 31) - 1:
            raise ValueError("%s: a bin midpoint of %s does not fit int32" % (path, name))
        ids.append(np.full(mid.size, chroms.intern(name), np.int32))
        mids.append(mid.astype(np.int32))
    if not ids:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    c, m = np.concatenate(ids), np.concatenate(mids)
    return c, m, np.ones(m.size, np.int32)


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog="python -m fithic_amd.fragments", description="Check help flag")
    parser.add_argument("--chrLens", help="Chromosome lengths file. In format, 'chrNUM\tlength'", required=True)
    parser.add_argument("--outFile", help="Output file for storing fragment file", required=True)
    parser.add_argument("--resolution", help="Resolution of dataset being analyzed", type=int, required=True)
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    sizes, out = os.path.realpath(args.chrLens), os.path.realpath(args.outFile)
    print("ChrSizeFile: %s" % sizes)
    print("OutFile: %s" % out)
    print("BinSize: %s" % args.resolution)
    with gzip.open(out, "wt") as f:
        f.write(fragment_text(sizes, args.resolution))


if __name__ == "__main__":
    main()
