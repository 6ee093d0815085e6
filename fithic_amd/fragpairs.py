"""HiC-Pro's allValidPairs binned to the restriction fragments of a digest: the contact counts that go with the fragments file of
`fithic_amd.digest` for `fithic -r 0`.  The reference ships no script for this step; the semantics below are this project's own.

    python -m fithic_amd.fragpairs VALIDPAIRS OUTFILE (--bed digest.bed | --fasta genome.fa --re HindIII [--also RE ...])
                                   [--drop NAME ...] [--device N]

writes OUTFILE as given (gzip) and prints the five counts.  The file - 1e8 to 1e9 lines - is parsed, looked up, sorted and counted
by kernels (csrc/fhx_fragpairs.hip); `read()` keeps the cells in HBM and hands them to an Engine without the file ever existing.

The fragment table comes from a `digest.Digest` made in this process, or from the bed file `digest --bed` writes (parsed on the
host; contigs are numbered in order of first appearance).  Per contig c (0-based) it is the ascending list E_c of fragment ends:
the contig's sites with duplicates kept, then its length - `Digest.fragment_ends()`.  g is the row of a fragment in the fragments
file.  The digest calls the contigs chr1, chr2, ... in file order and its column 3 is the fragment END; the contacts repeat
exactly those names and numbers.

A line is split at blanks and tabs; token 2 is name1, token 3 pos1, token 5 name2, token 6 pos2 (HiC-Pro's own fragment names in
tokens 9 and 10 are not read).  A line one of whose names is in `drop` is dropped and counted, and not read further.  Any other
name that is no contig of the table is a refusal.  A name may be in `drop` and a contig of the table: its fragments receive no
contacts.  Positions are 1-based and the bed is 0-based and half-open, so p lies in the fragment with start < p <= end:
k = bisect_left(E_c, p).  An empty fragment is never hit, of equal ends the first is taken.  The pair is ordered g1 < g2; a pair
with g1 == g2 is dropped and counted.  A cell's count is the number of lines that hit it.  Cells are written in ascending (g1, g2),
one line `chr<c1+1> \\t E[g1] \\t chr<c2+1> \\t E[g2] \\t count`, through the library's contacts writer (size-tagged gzip members).
The filters of the fixed-size script (names of at most 5 bytes, `chrM` anywhere in the line, a minimum distance) do not apply.

Known deviations: nothing is approximated.  Each of these is a ValueError that names file, 1-based line and reason - the smallest
such line of the file - and nothing is written: fewer than 6 tokens; a name that is neither a contig nor dropped; a position
that is not 1 to 10 digits (a sign, a point, an exponent), that is 0 or that lies above the contig's length; a NUL, a control
byte other than tab, DEL, a non-ASCII byte or a \\r that is not part of \\r\\n; a line of more than 4096 bytes; a cell hit by more
than 2^31 - 1 lines.  A bed file is refused with file and line for: fewer than 3 tokens, a start or an end that is not 1 to 10
digits or an end above 2^31 - 1, a name that comes back after another name, a contig whose first start is not 0, a start that is
not the previous end, an end below its start.  Limits, a ValueError before the validPairs file is opened: more than 4096 contigs,
a contig or drop name of more than 63 bytes, 2^31 or more fragments, more than 4096 drop names.
Not done: real marginal counts in the fragments file's column 4; a midpoint variant; fragment-size or pair-distance filters;
--gpus above 1.  There is no CPU implementation here: without the library or a GPU `read` raises.
"""
import argparse
import gzip
import os
import sys

import numpy as np

from . import _capi
from ._resident import Resident, _is_gzip
from .hicpro import _line_of

MAX_CONTIGS, MAX_NAME, MAX_DROP = _capi.FP_MAX_CONTIGS, _capi.FP_NAME_BYTES - 1, _capi.FP_MAX_CONTIGS
COUNT_NAMES = ("lines", "pairs", "dropped_name", "same_fragment", "cells")
_REASONS = {
    _capi.FP_TOKENS: "fewer than 6 tokens (read chr1 pos1 strand1 chr2 pos2 are expected)",
    _capi.FP_NAME: "a name that is neither a contig of the fragment table nor dropped (--drop)",
    _capi.FP_POSITION: "a position that is not written as 1 to 10 digits",
    _capi.FP_RANGE: "a position that is 0 or lies above the contig's length",
    _capi.FP_BYTES: "a NUL, a control byte other than tab, DEL, a non-ASCII byte or a \\r that is not part of \\r\\n",
    _capi.FP_LONG_LINE: "a line of more than 4096 bytes",
}


class Table:
    """The fragments of a digest: `names` (bytes, file order), `first` (int64, len(names) + 1 row offsets) and `ends` (int32): rows
    first[c] .. first[c + 1] - 1 of `ends` are E_c."""

    def __init__(self, names, first, ends):
        self.names, self.first, self.ends = list(names), np.asarray(first, np.int64), np.asarray(ends, np.int32)

    def __len__(self):
        return len(self.ends)


def check_limits(names, n_fragments, drop=()):
    """ValueError for a table or a drop list beyond the limits (module docstring); needs no GPU"""
    if len(names) > MAX_CONTIGS:
        raise ValueError("%d contigs: at most %d are taken" % (len(names), MAX_CONTIGS))
    for n in names:
        if len(n) > MAX_NAME:
            raise ValueError("contig name %r has %d bytes: at most %d are taken" % (n, len(n), MAX_NAME))
    if n_fragments >= 1 << 31:
        raise ValueError("%d fragments: fewer than 2^31 are taken" % n_fragments)
    if len(drop) > MAX_DROP:
        raise ValueError("%d names to drop: at most %d are taken" % (len(drop), MAX_DROP))
    for n in drop:
        if not 1 <= len(n) <= MAX_NAME:
            raise ValueError("name to drop %r: 1 to %d bytes are expected" % (n, MAX_NAME))


def table_of_digest(d):
    """the Table of a digest.Digest"""
    contig, end = d.fragment_ends()
    first = np.r_[0, np.cumsum(np.bincount(contig, minlength=len(d.names)))].astype(np.int64)
    return Table([n.encode("latin-1") for n in d.names], first, end)


def _numbers(buf, start, stop):
    """tokens buf[start[i]:stop[i]] as 1 to 10 digits -> (values int64, bad bool)"""
    length = stop - start
    bad = (length < 1) | (length > 10)
    value = np.zeros(len(start), np.int64)
    for k in range(10):
        rows = np.flatnonzero((length > k) & ~bad)
        if not len(rows):
            break
        digit = buf[start[rows] + k].astype(np.int64) - 48
        wrong = (digit < 0) | (digit > 9)
        bad[rows[wrong]] = True
        value[rows] = value[rows] * 10 + digit
    return value, bad


def table_of_bed(path):
    """the Table of the bed file `digest --bed` writes (plain or gzipped), parsed with numpy on the host.  ValueError with file and
    line for a file that is not such a bed (module docstring)."""
    path = os.fspath(path)
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)

    def refuse(row, what):
        raise ValueError("%s, line %d: %s" % (path, row + 1, what))

    buf = np.frombuffer(data, np.uint8)
    if not len(buf):
        raise ValueError("%s: no fragment in the file" % path)
    newline = np.flatnonzero(buf == 10)
    line_start = np.r_[0, newline + 1]
    if line_start[-1] == len(buf):                                   # the text ends in a newline: no line begins behind it
        line_start = line_start[:-1]
    line_stop = np.r_[line_start[1:], len(buf)]
    blank = (buf == 32) | (buf == 9) | (buf == 13) | (buf == 10)
    tok_start = np.flatnonzero(~blank & np.r_[True, blank[:-1]])
    tok_stop = np.flatnonzero(~blank & np.r_[blank[1:], True]) + 1
    t0 = np.searchsorted(tok_start, line_start)                      # every line's first token
    n_tok = np.searchsorted(tok_start, line_stop) - t0
    # every check is made on every line, and the smallest refused line is reported: what a refused line's own tokens give (its
    # numbers, the start of the line behind it) only raises lines that lie behind it
    problems = []

    def note(rows, what):
        if len(rows):
            problems.append((int(rows[0]), len(problems), what))                 # on one line the earlier check names the reason

    if not len(tok_start):
        refuse(0, "0 token(s) where name, start and end are expected")
    note(np.flatnonzero(n_tok < 3), "fewer than 3 tokens where name, start and end are expected")
    last = len(tok_start) - 1
    t1, t2 = np.minimum(t0 + 1, last), np.minimum(t0 + 2, last)
    t0 = np.minimum(t0, last)
    start, bad_start = _numbers(buf, tok_start[t1], tok_stop[t1])
    end, bad_end = _numbers(buf, tok_start[t2], tok_stop[t2])
    note(np.flatnonzero(bad_start | bad_end | (end > 0x7fffffff)),
         "a start or an end that is not written as 1 to 10 digits, or an end above 2^31 - 1")
    # where the name changes from one line to the next
    a, b = tok_start[t0], tok_stop[t0]
    length = b - a
    changed = np.r_[True, length[1:] != length[:-1]]
    for k in range(int(length.max())):
        rows = np.flatnonzero((length[1:] > k) & ~changed[1:]) + 1
        if not len(rows):
            break
        changed[rows[buf[a[rows] + k] != buf[a[rows - 1] + k]]] = True
    heads = np.flatnonzero(changed)
    names, seen = [], set()
    for row in heads:
        name = data[a[row]:b[row]]
        if name in seen:
            note([row], "the name %r comes back after another name" % name.decode("latin-1"))
            break
        seen.add(name)
        names.append(name)
    first_row = np.zeros(len(start), bool)
    first_row[heads] = True
    later = np.flatnonzero(~first_row)
    note(np.flatnonzero(first_row & (start != 0)), "a contig whose first start is not 0")
    note(later[start[later] != end[later - 1]], "a start that is not the previous end")
    note(np.flatnonzero(end < start), "an end below its start")
    if problems:
        row, _, what = min(problems)
        refuse(row, what)
    return Table(names, np.r_[heads, len(start)].astype(np.int64), end.astype(np.int32))


def table_of(table):
    """a Table, a digest.Digest or the path of a bed file -> a Table"""
    if isinstance(table, Table):
        return table
    if hasattr(table, "fragment_ends"):
        return table_of_digest(table)
    return table_of_bed(table)


def _refusal(path, e):
    """the exception a refused file is reported with (module docstring, `Known deviations`)"""
    if e.why == _capi.FP_COUNT:
        return ValueError("%s: a cell is hit by more than 2^31 - 1 pairs; the count column is int32" % path)
    if e.why == _capi.FP_PAIRS:
        return ValueError("%s: 2^32 or more pairs are kept; the sort does not take them" % path)
    if e.why not in _REASONS:
        return e
    text = ": %r" % _line_of(path, e.line).decode("latin-1")[:80] if not _is_gzip(path) and e.why != _capi.FP_LONG_LINE else ""
    return ValueError("%s, line %d: %s%s" % (path, e.line, _REASONS[e.why], text))


class FragPairs(Resident):
    """One validPairs file binned to fragments: the cells (chr1, end1, chr2, end2, count) resident in HBM, in ascending order of
    the two fragments' rows in the fragments file.  `names` holds chr1, chr2, ... - one per contig of the table, as
    Digest.fragments leaves them in a ChromIndex.  counts(): lines, pairs (kept), dropped_name, same_fragment, cells.
    load_into: the cells into a configured Engine whose fragments are loaded."""

    def __init__(self, fp, n_cells, names):
        super().__init__(fp, n_cells, names)
        self.n_cells = n_cells

    def write(self, path):
        _capi.host_write_contacts(path, self.names, *self.contacts())


def read(validpairs_path, table, drop=(), device=0):
    """The direct path: a validPairs file (plain or gzipped) and a fragment table (a digest.Digest or the path of its bed file) -> a
    FragPairs whose cells stay on GPU `device`.  ValueError for a table beyond the limits or a file outside the grammar.  Raises
    without the library or a GPU: there is no CPU path."""
    table = table_of(table)
    drop = sorted(set(d.encode("latin-1") if isinstance(d, str) else bytes(d) for d in drop))
    check_limits(table.names, len(table), drop)
    contig_of = {n: k for k, n in enumerate(table.names)}
    if len(contig_of) != len(table.names):
        raise ValueError("a contig name is given twice in the fragment table")
    dropped = set(drop)
    names = list(table.names) + [d for d in drop if d not in contig_of]
    name_contig = [-1 if n in dropped else contig_of[n] for n in names]
    path = os.fspath(validpairs_path)
    fp = _capi.FpContext(device)
    try:
        fp.load_table(names, name_contig, table.first, table.ends)
        try:
            n = fp.bin_file(path)
        except _capi.FpRefused as e:
            raise _refusal(path, e) from None
        return FragPairs(fp, n, ["chr%d" % (k + 1) for k in range(len(table.names))])
    except BaseException:
        fp.close()
        raise


def parse_args(argv):
    parser = argparse.ArgumentParser(prog="python -m fithic_amd.fragpairs",
                                     description="allValidPairs -> the contact counts between the fragments of a digest, for fithic -r 0")
    parser.add_argument("validpairs", metavar="VALIDPAIRS", help="HiC-Pro's allValidPairs (plain or gzipped)")
    parser.add_argument("outfile", metavar="OUTFILE", help="the contact counts (gzip), written as given")
    parser.add_argument("--bed", metavar="PATH", help="the fragment bed that `python -m fithic_amd.digest --bed` wrote")
    parser.add_argument("--fasta", metavar="PATH", help="the reference genome: it is digested first (needs --re)")
    parser.add_argument("--re", metavar="RE", help="with --fasta: the enzyme's name, or the cutting position using ^")
    parser.add_argument("--also", metavar="RE", action="append", default=[], help="with --fasta: a further enzyme; may be repeated")
    parser.add_argument("--drop", metavar="NAME", action="append", default=[], help="drop the pairs that name this contig (e.g. chrM); "
                        "may be repeated")
    parser.add_argument("--device", type=int, default=0)
    args = parser.parse_args(argv)
    if (args.bed is None) == (args.fasta is None):
        parser.error("one of --bed and --fasta is expected")
    if args.fasta is not None and args.re is None:
        parser.error("--fasta needs --re")
    if args.bed is not None and (args.re is not None or args.also):
        parser.error("--re and --also go with --fasta")
    return args


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    if args.bed is not None:
        table = table_of_bed(args.bed)
    else:
        from . import digest
        table = table_of_digest(digest.read(args.fasta, [args.re] + args.also, device=args.device))
    with read(args.validpairs, table, drop=args.drop, device=args.device) as data:
        data.write(args.outfile)
        counts = data.counts()
    for key in COUNT_NAMES:
        print("%s\t%d" % (key, counts[key]))


if __name__ == "__main__":
    main()
