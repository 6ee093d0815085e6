"""createFitHiCFragments-nonfixedsize.sh on the MI355X engine: a reference genome cut with a restriction enzyme into the fragments
file `fithic -r 0` reads (reference: fithic/utils/createFitHiCFragments-nonfixedsize.sh, which runs HiC-Pro's digest_genome.py and
then a loop over its bed file).  The cut sites are found on the GPU (csrc/fhx_digest.hip); the two files are formatted and
compressed by the library's host code.

    python -m fithic_amd.digest OUTFILE RE FASTA [--also RE ...] [--bed PATH]

takes the script's three arguments and prints its `Working on <name>` lines.  The result is OUTFILE.gz, whose decompressed bytes
are what the script leaves when OUTFILE did not exist before: one line `chr<k> \\t 0 \\t <end> \\t 1 \\t 1` per fragment.  Column 3 is the
fragment's END, not a midpoint, and the contig names do not survive: they are chr1, chr2, ... in file order.  That is what the
script writes.

Step 1, the digest.  RE is a name in any case (hindiii A^AGCTT, mboi ^GATC, dpnii ^GATC, bglii A^GATCT) or a site of the letters
ACGTN with exactly one `^`; the offset is the index of `^`, the motif is the site without it, every N is expanded into A C G T.
A FASTA line that begins with `>` starts a contig named `line.split()[0][1:]`; every other line adds `line.lower().strip()` to
the contig's sequence; lines before the first header add to nothing.  Every start s at which the sequence equals a motif gives
the site s + offset: overlapping matches all count, the genome's own `n` matches nothing.  Per contig the sites of all motifs are
sorted with duplicates kept; the fragments are the pairs of [0] + sites with sites + [length], empty ones included, and a contig
without sequence is the one fragment 0 0.  Bed line: `name \\t start \\t end \\t HIC_<name>_<k> \\t 0 \\t +`, k from 1 within the contig.

`read(fasta, sites)` returns a Digest: names, lengths, sites(), fragments() as the columns Engine.load_fragments takes (no
intermediate file), write(), write_bed(), stage_seconds().

Extensions: a FASTA that starts with the gzip magic is inflated first; `--bed PATH` also writes Step 1's bed file.

Known deviations: only the regular text is taken and nothing is approximated.  Each of these is a ValueError that names file,
line and reason, and nothing is written: a NUL, a non-ASCII byte, DEL or a control byte other than \\n and a \\r directly before \\n
(a tab is taken in a header line); a blank or a tab in a line that is no header (strip() would drop it at the ends and count it
inside); a line of more than 4096 bytes (an unwrapped FASTA: re-wrap it, e.g. `fold -w 60`); a contig of more than 2^31 - 1 bases
(reported at its header); an empty contig name (`>` alone, `> text`); a name that holds one of * ? [ \\ (the script's unquoted
`read` and array split would mangle it); a name seen twice (HiC-Pro's script exits there); a file without any header (the script
would end in a failing gzip).  The grammar of the bytes holds for the lines before the first header too.  Limits, a ValueError
before any file is opened: a motif of 1 to 16 bases, at most 3 N per site, at most 64 expanded motifs in all.
Not done: an unwrapped FASTA (lines over 4096 bytes); IUPAC codes other than N; minimum or maximum fragment size filters; a
midpoint variant of column 3.  Read pairs are binned to the fragments by fithic_amd.fragpairs.  There is no CPU implementation here:
without the library or a GPU `read` raises.
"""
import argparse
import itertools
import os
import sys
import time

import numpy as np

from . import _capi
from .hicpro import _line_of

ENZYMES = {"hindiii": "A^AGCTT", "mboi": "^GATC", "dpnii": "^GATC", "bglii": "A^GATCT"}
MAX_MOTIF, MAX_N, MAX_MOTIFS = _capi.DG_MAX_MOTIF, 3, _capi.DG_MAX_MOTIFS
_REASONS = {
    _capi.DG_BYTES: "a NUL, a control byte other than \\n and a \\r directly before \\n, DEL or a non-ASCII byte",
    _capi.DG_BLANK: "a blank or a tab in a sequence line",
    _capi.DG_LONG_LINE: "a line of more than 4096 bytes: an unwrapped FASTA is not taken, re-wrap it (e.g. fold -w 60)",
    _capi.DG_CONTIG_LENGTH: "a contig of more than 2^31 - 1 bases",
    _capi.DG_EMPTY_NAME: "a header without a contig name",
    _capi.DG_NAME_CHARS: "a contig name that holds one of * ? [ \\",
    _capi.DG_DUPLICATE: "a contig name that was seen before",
    _capi.DG_NO_HEADER: "no header line (`>name`) in the file",
}


def parse_sites(sites):
    """['hindiii', 'G^ANTC', ...] -> [(motif in lower case, offset), ...] with every N expanded, in the order given.  Needs no GPU.
    ValueError for anything outside the limits (module docstring)."""
    if isinstance(sites, str):
        sites = [sites]
    out = []
    for given in sites:
        if not isinstance(given, str):
            raise ValueError("cut site %r: a name or a site such as A^AGCTT is expected" % (given,))
        site = ENZYMES.get(given.lower(), given).upper()
        if site.count("^") != 1 or any(c not in "ACGTN^" for c in site):
            raise ValueError("cut site %r: one of %s, or the letters ACGTN with exactly one ^, is expected" % (given, ", ".join(sorted(ENZYMES))))
        offset = site.index("^")
        motif = site.replace("^", "")
        if not 1 <= len(motif) <= MAX_MOTIF:
            raise ValueError("cut site %r: a motif of 1 to %d bases is expected" % (given, MAX_MOTIF))
        if motif.count("N") > MAX_N:
            raise ValueError("cut site %r: at most %d N per site" % (given, MAX_N))
        for letters in itertools.product(*[("ACGT" if c == "N" else c) for c in motif]):
            out.append(("".join(letters).lower(), offset))
    if not out:
        raise ValueError("at least one cut site is expected")
    if len(out) > MAX_MOTIFS:
        raise ValueError("%d motifs once every N is expanded: at most %d are taken" % (len(out), MAX_MOTIFS))
    return out


def _refusal(path, e):
    """the exception a refused file is reported with (module docstring, `Known deviations`)"""
    if e.why == _capi.DG_INTERNAL or e.why not in _REASONS:
        return e
    with open(path, "rb") as f:
        gzipped = f.read(2) == b"\x1f\x8b"
    text = "" if gzipped or e.why == _capi.DG_NO_HEADER else ": %r" % _line_of(path, e.line).decode("latin-1")[:80]
    return ValueError("%s, line %d: %s%s" % (path, e.line, _REASONS[e.why], text))


class Digest:
    """One digested FASTA: `names` (str, file order), `lengths` (int64) and the cut sites, fetched once from the device."""

    def __init__(self, names, lengths, site_contig, site_position, seconds):
        self.names, self.lengths = names, lengths
        self._contig, self._position = site_contig, site_position
        self._seconds = seconds

    def sites(self):
        """(contig index, position), int32, ordered by contig and position, duplicates kept"""
        return self._contig, self._position

    def fragment_ends(self):
        """(contig index, end) of every fragment in file order: a contig's sites, then its length"""
        n = len(self.names)
        per = np.bincount(self._contig, minlength=n).astype(np.int64)
        contig = np.repeat(np.arange(n, dtype=np.int32), per + 1)
        end = np.empty(len(contig), np.int32)
        last = np.cumsum(per + 1) - 1                                # the row of every contig's last fragment
        keep = np.ones(len(contig), bool)
        keep[last] = False
        end[keep] = self._position
        end[last] = self.lengths
        return contig, end

    def fragments(self, chroms):
        """(chr ids, mids, hits) as tables.read_fragments returns them for the written file - the mid column holds the fragment
        ENDS, as the file's column 3 does - with chr1, chr2, ... interned into `chroms`, the run's ChromIndex"""
        contig, end = self.fragment_ends()
        ids = np.array([chroms.intern("chr%d" % (k + 1)) for k in range(len(self.names))], np.int32)
        return ids[contig], end, np.ones(len(end), np.int32)

    def write(self, path, threads=0):
        """the fragments file, gzip: `path` is written as given (the command line adds .gz as the script's gzip does)"""
        t0 = time.perf_counter()
        _capi.dg_write_fragments(path, self.lengths, self._contig, self._position, threads=threads)
        self._seconds["write"] = self._seconds.get("write", 0.0) + time.perf_counter() - t0

    def write_bed(self, path, threads=0):
        """HiC-Pro's fragment bed, plain text"""
        t0 = time.perf_counter()
        _capi.dg_write_bed(path, [n.encode("latin-1") for n in self.names], self.lengths, self._contig, self._position, threads=threads)
        self._seconds["write"] = self._seconds.get("write", 0.0) + time.perf_counter() - t0

    def stage_seconds(self):
        """host clocks: read_upload, newline_scan, class_pass, sites, sort, fetch, write (the write calls made so far)"""
        out = dict(self._seconds)
        out.setdefault("write", 0.0)
        return out


def read(fasta, sites, device=0):
    """The digest of one FASTA with one or more cut sites (names or A^AGCTT style, as parse_sites takes them) -> a Digest.
    ValueError for a file outside the grammar.  Raises without the library or a GPU: there is no CPU path."""
    motifs = parse_sites(sites)
    fasta = os.fspath(fasta)
    dg = _capi.DgContext(device)
    try:
        try:
            dg.digest_file(fasta, motifs)
        except _capi.DgRefused as e:
            raise _refusal(fasta, e) from None
        names = [n.decode("latin-1") for n in dg.names()]
        lengths = dg.lengths()
        contig, position = dg.fetch_sites()
        return Digest(names, lengths, contig, position, dg.stage_seconds())
    finally:
        dg.close()


def parse_args(argv):
    parser = argparse.ArgumentParser(prog="python -m fithic_amd.digest",
                                     description="createFitHiCFragments-nonfixedsize.sh: OUTFILE.gz for fithic -r 0")
    parser.add_argument("outfile", metavar="OUTFILE", help="A desired output file path (.gz is appended, as the script's gzip does)")
    parser.add_argument("re", metavar="RE", help="Either the name of the restriction enzyme used, or the cutting position using ^. "
                        "For example, A^AGCTT for HindIII.")
    parser.add_argument("fasta", metavar="FASTA", help="A reference genome in fasta format (plain or gzipped)")
    parser.add_argument("--also", metavar="RE", action="append", default=[], help="a further enzyme; may be repeated")
    parser.add_argument("--bed", metavar="PATH", help="also write HiC-Pro's fragment bed file here")
    parser.add_argument("--device", type=int, default=0)
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    d = read(args.fasta, [args.re] + args.also, device=args.device)
    if args.bed:
        d.write_bed(args.bed)
    d.write(args.outfile + ".gz")
    for name in d.names:
        print("Working on %s" % name)


if __name__ == "__main__":
    main()
