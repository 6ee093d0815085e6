"""HiCPro2FitHiC on the MI355X engine: HiC-Pro's `.matrix` / `_abs.bed` / `.biases` turned into the three tables `fithic` reads
(reference: fithic/utils/HiCPro2FitHiC.py), same flags, same file names, same progress lines.

    python -m fithic_amd.hicpro -i sample_10000.matrix -b sample_10000_abs.bed [-s sample_10000_iced.matrix.biases] [-o .] [-r 0]

writes fithic.interactionCounts.gz, fithic.fragmentMappability.gz and (with -s) fithic.biases.gz; their decompressed bytes are
the reference's.  The matrix - one line per non-zero cell, 1.5e8 lines genome-wide at 5 kb - is parsed, looked up and summed
per bin by kernels (csrc/fhx_hicpro.hip); the bed and bias files have one line per bin and are handled here with the
reference's own Python semantics.  `read()` keeps the contact columns in HBM and hands them to an Engine without the three
files ever existing.

Known deviations: the device path takes a RAW matrix only - counts written as digits or digits.000 (the reference prints both
as the integer).  A non-integral count (an ICE-normalised matrix), an exponent form (`1e2`), an underscore, a sign, an index of
more than 10 digits or a count beyond int32 is refused with a ValueError that names the line - the reference accepts those;
nothing is written then, while the reference leaves the files written up to the bad line.  A line with a fourth token is refused
too (the reference ignores the extra tokens).  There is no CPU implementation here: without the library or a GPU the entry
points raise.
"""
import argparse
import gzip
import math
import os

import numpy as np

from . import _capi, tables
from ._resident import Resident

MAX_INDEX_SPAN = 1 << 27
_INT32_MIN, _INT32_MAX = -(1 << 31), (1 << 31) - 1


class Bed:
    """The bed file as the reference's fragDic (:19-30): index -> [chr, start text, mid], a repeated index overwrites."""

    def __init__(self, frag, res, chroms):
        self.res, self.chroms = res, chroms
        self.indices = sorted(frag)                                  # the order the fragments file is written in (:49)
        self.frag = frag                                             # index -> (chr id, start text, mid)
        self.index_base = self.indices[0] if self.indices else 0
        self.n_slots = self.indices[-1] - self.index_base + 1 if self.indices else 0
        if self.n_slots > MAX_INDEX_SPAN:
            raise ValueError("bed indices span %d..%d: more than 2^27 slots, the dense bin table does not take that"
                             % (self.indices[0], self.indices[-1]))
        self.chr_id = np.full(self.n_slots, -1, np.int32)            # dense over [index_base, index_base + n_slots); -1: absent
        self.mid = np.zeros(self.n_slots, np.int32)
        for index, (c, _, mid) in frag.items():
            if not _INT32_MIN <= mid <= _INT32_MAX:
                raise ValueError("bed index %d: midpoint %d does not fit int32" % (index, mid))
            self.chr_id[index - self.index_base] = c
            self.mid[index - self.index_base] = mid

    def name(self, index):
        return self.chroms.names[self.frag[index][0]]


def read_bed(path, res=0, chroms=None):
    """HiCPro2FitHiC.py:21-30: split(), chr = t[0], start = t[1] kept as text, index = int(t[3]); res == 0 is replaced by
    end - start of the line it is met at (the first one, unless that bin is empty)."""
    chroms = tables.ChromIndex() if chroms is None else chroms
    frag = {}
    with open(path, "r") as f:
        for lines in f:
            line = lines.rstrip().split()
            name, start, en = line[0], line[1], line[2]
            if res == 0:
                res = int(en) - int(start)
            mid = int(start) + int(res / 2)
            frag[int(line[3])] = (chroms.intern(name), start, mid)
    return Bed(frag, res, chroms)


def fragments_lines(bed, totals):
    """HiCPro2FitHiC.py:48-53; totals[slot] = the bin's total contact count (exact integers)"""
    out = []
    for index in bed.indices:
        _, start, mid = bed.frag[index]
        tcc = int(totals[index - bed.index_base])
        out.append("%s\t%s\t%s\t%s\t%s\n" % (bed.name(index), start, mid, tcc, 1 if tcc > 0 else 0))
    return out


def convert_bias(path):
    """HiCPro2FitHiC.py:58-81: line k (1-based) -> the value of index k divided by the mean of the values that are not NaN, -1
    for NaN.  The sum runs left to right, as the reference's does (its rounding order)."""
    values = []
    total, n = 0, 0
    with open(path, "r") as f:
        for lines in f:
            value = float(lines.rstrip())
            values.append(value)
            if not math.isnan(value):
                total += value
                n += 1
    avg = total / n                                                  # ZeroDivisionError when every value is NaN, like the reference
    return [-1 if math.isnan(v) else v / avg for v in values]


def bias_lines(bed, values):
    """HiCPro2FitHiC.py:76-82; KeyError(index) for a bias line beyond the bed"""
    out = []
    for k, value in enumerate(values):
        index = k + 1
        if index not in bed.frag:
            raise KeyError(index)
        out.append("%s\t%s\t%s\n" % (bed.name(index), bed.frag[index][2], value))
    return out


def _line_of(path, number):
    """the `number`-th line of a file (1-based, lines end at \\n), as bytes"""
    left = number - 1
    with open(path, "rb") as f:
        tail = b""
        while True:
            chunk = f.read(1 << 24)
            if not chunk:
                return tail
            if left:
                k = chunk.count(b"\n")
                if k < left:
                    left -= k
                    continue
                pos = -1
                for _ in range(left):
                    pos = chunk.find(b"\n", pos + 1)
                chunk = chunk[pos + 1:]
                left = 0
            end = chunk.find(b"\n")
            if end >= 0:
                return tail + chunk[:end]
            tail += chunk


def _refusal(path, e):
    """the exception a refused matrix is reported with (module docstring, `Known deviations`)"""
    if e.why == _capi.HP_ABSENT:
        return KeyError(e.index)                                     # fragDic[i], as the reference raises it
    if e.why == _capi.HP_TOTAL:
        return ValueError("%s: a bin's total contact count reaches 2^53, where the reference's float sum rounds; this path "
                          "does not take such a matrix" % path)
    if e.why == _capi.HP_INTERNAL:
        return e
    where = "%s, line %d" % (path, e.line)
    text = _line_of(path, e.line).decode("latin-1")
    tokens = text.split()
    if e.why == _capi.HP_BYTES:
        return ValueError("%s: a NUL, a non-ASCII byte or a \\r that is not part of \\r\\n: %r" % (where, text[:80]))
    if e.why == _capi.HP_LONG_LINE:
        return ValueError("%s: a line of more than 4096 bytes" % where)
    if e.why == _capi.HP_TOKENS and len(tokens) < 3:
        return ValueError("%s: %d token(s) where `i j count` is expected: %r" % (where, len(tokens), text[:80]))
    try:                                                             # would the reference have read this line?
        int(tokens[0]), int(tokens[1]), float(tokens[2])
    except ValueError as err:
        return ValueError("%s: %s" % (where, err))
    what = {_capi.HP_TOKENS: "more than three tokens (the reference ignores the extra ones)",
            _capi.HP_INDEX: "an index of more than 10 digits or outside int32",
            _capi.HP_FRACTION: "a count that is not a whole number",
            _capi.HP_COUNT: "a count that is not written as digits[.digits] within int32 (a sign, an exponent, an underscore, "
                            "inf / nan or more than 15 digits)"}.get(e.why, "a line outside the device grammar")
    return ValueError("%s: %s: %r.  The reference accepts this line; fithic_amd.hicpro expects a raw (integer) HiC-Pro matrix "
                      "and does not take it." % (where, what, text[:80]))


class HicPro(Resident):
    """One converted HiC-Pro data set: the fragments and bias tables on the host, the contact columns resident in HBM.
    load_into: the three tables into a configured Engine; `chroms` is the run's ChromIndex: empty (it receives this data set's
    names) or one whose ids agree with them."""
    _FETCH = "fetch_rows"

    def __init__(self, bed, hp, n_rows, totals, bias_values):
        super().__init__(hp, n_rows, bed.chroms.names)
        self.bed, self.chroms, self.n_rows = bed, bed.chroms, n_rows
        self.totals = totals                                         # int64 per slot of the dense table
        self.bias_values = bias_values                               # per bias line: value / mean, -1 for NaN; None without -s

    @property
    def fragments(self):
        """(chr ids, mids, hits) as tables.read_fragments returns them for the written fragments file"""
        slots = np.asarray(self.bed.indices, np.int64) - self.bed.index_base
        hits = self.totals[slots]
        if hits.size and hits.max() > _INT32_MAX:
            raise ValueError("a bin's total contact count does not fit int32")
        return self.bed.chr_id[slots].copy(), self.bed.mid[slots].copy(), hits.astype(np.int32)

    @property
    def bias(self):
        """(chr ids, mids, values) as tables.read_bias returns them for the written bias file; None without a bias file"""
        if self.bias_values is None:
            return None
        for k in range(len(self.bias_values)):
            if k + 1 not in self.bed.frag:
                raise KeyError(k + 1)
        slots = np.arange(1, len(self.bias_values) + 1, dtype=np.int64) - self.bed.index_base
        return self.bed.chr_id[slots].copy(), self.bed.mid[slots].copy(), np.asarray(self.bias_values, np.float64)

    def _load_tables(self, engine, chroms):
        engine.load_fragments(*self.fragments, chroms.sort_rank())
        bias = self.bias
        if bias is not None:
            engine.load_bias(*bias)


def read(bed, matrix, bias=None, res=0, device=0):
    """The direct path: bed + matrix (+ bias) -> a HicPro whose contact columns stay on GPU `device`."""
    b = read_bed(bed, res)
    hp = _capi.HpContext(device)
    try:
        hp.load_bins(b.index_base, b.chr_id, b.mid)
        try:
            n = hp.parse_matrix(matrix)
        except _capi.HpRefused as e:
            raise _refusal(matrix, e) from None
        return HicPro(b, hp, n, hp.totals(), None if bias is None else convert_bias(bias))
    except BaseException:
        hp.close()
        raise


def outputfithicform(bedPath, matrixPath, intCPath, fragMapPath, biasVectorPath=None, biasVectorOutput=None, res=0, device=0):
    """HiCPro2FitHiC.py:17-83 with the reference's signature.  Everything is computed before anything is written: a refused
    matrix or a bad bias file leaves no output file."""
    print("Loading matrix file...")
    want_bias = biasVectorPath is not None and biasVectorOutput is not None
    with read(bedPath, matrixPath, None, res, device) as data:
        for k in range(1, data.n_rows // 1000000 + 1):
            print("%d million lines read" % k)
        frag_text = fragments_lines(data.bed, data.totals)
        bias_text = None
        if want_bias:
            print("Converting bias file...")
            bias_text = bias_lines(data.bed, convert_bias(biasVectorPath))
        _capi.host_write_contacts(intCPath, data.chroms.names, *data.contacts())
        with gzip.open(fragMapPath, "wt") as f:
            f.write("".join(frag_text))
        if want_bias:
            with gzip.open(biasVectorOutput, "wt") as f:
                f.write("".join(bias_text))
    print("Conversion from HiC-Pro to Fit-Hi-C format completed")


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog="python -m fithic_amd.hicpro")
    parser.add_argument("-i", "--matrix", help="Input matrix file with raw contact frequencies.", required=True)
    parser.add_argument("-b", "--bed", help="BED file with bins coordinates.", required=True)
    parser.add_argument("-s", "--bias", help="The bias file provided after IC normalization.", default=None)
    parser.add_argument("-o", "--output", help="Output path", default=".")
    parser.add_argument("-r", "--resolution", help="Resolution of the matrix", type=int, default=0)
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    icounts_output = os.path.join(args.output + "/fithic.interactionCounts.gz")
    fragmap_output = os.path.join(args.output + "/fithic.fragmentMappability.gz")
    bias_output = os.path.join(args.output + "/fithic.biases.gz") if args.bias is not None else None
    outputfithicform(args.bed, args.matrix, icounts_output, fragmap_output, args.bias, bias_output, args.resolution)


if __name__ == "__main__":
    main()
