"""createFitHiCContacts-hic on the MI355X engine: the text `juicer_tools dump` / `straw` prints for one chromosome pair of a Juicer
.hic file (`binX binY count` per record) turned into the contact counts `fithic` reads (reference:
fithic/utils/createFitHiCContacts-hic_old.sh and fithic/utils/createFitHiCContacts-hic.py).  Two command lines, one set of kernels
(csrc/fhx_juicer.hip); every input line gives exactly one output line.

    python -m fithic_amd.juicer DUMP CHR1 CHR2 OUT

is the old script, VERBATIM mode: OUT is gzip and its decompressed bytes are the script's under LC_ALL=C with mawk 1.3.4,
`CHR1 \\t $1 \\t CHR2 \\t $2 \\t $3 \\n` with awk's fields copied as text (`12.50` stays `12.50`): fields split at runs of blank and tab, a
missing field is empty, tokens after the third are ignored, a last line without a newline gets one.

    python -m fithic_amd.juicer --dump DUMP --CHR1 1 --CHR2 X --resolution R --outFile OUT [--datatype observed] [--Norm NONE]

takes the flags of the .py with --dump in place of --HiCFile, MIDPOINT mode: OUT holds what the .py prints per record,
`chr<CHR1> \\t binX+int(R/2) \\t chr<CHR2> \\t binY+int(R/2) \\t count \\n`, the count as Python's str() of the record's float (`17`, `17.0`
and `017` give `17.0`).  OUT is plain text as the reference's is.  Extension: when OUT ends in `.gz` the same bytes are written
gzipped, because `fithic` reads only gzip.  --datatype and --Norm are echoed as the reference echoes them; its three `list of ...`
lines need an open .hic file and are not printed.

`read([(dump, chr1, chr2), ...], resolution)` keeps the rows of all dumps in HBM and hands them to an Engine without any
intermediate file (with fragments.bins: a genome-wide run from a directory of dump files).  Reading the binary .hic container is
out of scope: the unit of input is the dump text, plain or gzipped.

Known deviations: nothing is parsed approximately, so a file outside the device grammar is refused with a ValueError that names
file, line and reason, and nothing is written.  Refused in both modes: a NUL, a control byte other than tab (so \\r\\n files), DEL,
a non-ASCII byte, a line of more than 4096 bytes.  `awk -v` expands backslash escapes and the script leaves $CHR1 unquoted, so a
chromosome name is taken only as 1 to 63 bytes of [A-Za-z0-9_.-]; anything else is a ValueError before the file is opened.
Midpoint mode, refused although the .py has no such rule: a line that is not exactly three tokens; a bin that is not 1 to 10 digits
without a sign, is no multiple of R (a .hic file holds no other record at that resolution) or whose midpoint is above 2^31 - 1;
a count that is not `digits` or `digits.` and one or more `0`, has more than 15 digits or is above 2^24 (hicstraw's records are
binary32: beyond 2^24 the reference itself would print another number); R outside 1 .. 2^31 - 1.  A normalised dump (fractions,
exponents, signs, NaN) is refused: a raw (`NONE`) dump is expected.  There is no CPU implementation here: without the library or a
GPU the entry points raise.
"""
import argparse
import gzip
import os
import re
import sys

from . import _capi
from ._resident import Resident
from .hicpro import _line_of

_NAME = re.compile(r"[A-Za-z0-9_.-]{1,63}\Z")
_REASONS = {
    _capi.JC_BYTES: "a NUL, a control byte other than tab (\\r is one), DEL or a non-ASCII byte",
    _capi.JC_LONG_LINE: "a line of more than 4096 bytes",
    _capi.JC_TOKENS: "exactly three tokens are expected (binX binY count)",
    _capi.JC_BIN: "binX and binY are expected as 1 to 10 digits without a sign",
    _capi.JC_GRID: "binX and binY must be multiples of the resolution",
    _capi.JC_RANGE: "a bin whose midpoint is above 2^31 - 1",
    _capi.JC_COUNT: "the count is not a whole number of at most 15 digits and at most 2^24 (16777216)",
    _capi.JC_FRACTION: "a count with a fraction, an exponent, a sign, nan or inf: a raw (`NONE`) dump is expected",
}


def check_name(name):
    """a chromosome name as both command lines take it, or ValueError"""
    if not isinstance(name, str) or not _NAME.match(name):
        raise ValueError("chromosome name %r: 1 to 63 bytes of [A-Za-z0-9_.-] are expected" % (name,))
    return name


def check_resolution(resolution):
    if isinstance(resolution, bool) or not isinstance(resolution, int) or not 1 <= resolution <= (1 << 31) - 1:
        raise ValueError("resolution %r: an integer from 1 to 2^31 - 1 is expected" % (resolution,))
    return resolution


def _refusal(path, e):
    """the exception a refused file is reported with (module docstring, `Known deviations`)"""
    if e.why == _capi.JC_INTERNAL or e.why not in _REASONS:
        return e
    with open(path, "rb") as f:
        gzipped = f.read(2) == b"\x1f\x8b"
    text = "" if gzipped else ": %r" % _line_of(path, e.line).decode("latin-1")[:80]
    return ValueError("%s, line %d: %s%s" % (path, e.line, _REASONS[e.why], text))


def _write(path, text, gzipped):
    if gzipped:                                                      # the settings of mergefilter.Selection.write_subset
        with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=6, mtime=0, filename="") as f:
            f.write(text)
    else:
        with open(path, "wb") as f:
            f.write(text)


class JuicerContacts(Resident):
    """The records of one or more dumps: the rows (chr1, mid1, chr2, mid2, count) resident in HBM in the order given, and their text.
    load_into: the rows into a configured Engine whose fragments are loaded."""
    _FETCH = "fetch_rows"

    def __init__(self, jc, resolution, names):
        super().__init__(jc, jc.counts()["rows"], names)
        self.resolution, self.n_rows = resolution, self._n

    def text(self):
        """the lines createFitHiCContacts-hic.py writes for the dumps, one after the other"""
        return self._handle.text()

    def write(self, path):
        """the text, gzipped: a contacts file `fithic` reads"""
        _write(path, self.text(), True)


def read(dumps, resolution, device=0, keep_text=True):
    """The direct path, midpoint mode: dumps = [(path, chr1, chr2), ...] with the names as --CHR1 / --CHR2 take them (no `chr`
    prefix) -> a JuicerContacts whose rows stay on GPU `device` in the order given.  Names get their ids in the order an
    ordinary read of the written file would give them: by first appearance, chr1 before chr2, a dump without lines naming none.
    keep_text=False skips the format kernel and the copy to the host: text() is then empty and only the rows are made."""
    check_resolution(resolution)
    dumps = [(os.fspath(p), "chr" + check_name(a), "chr" + check_name(b)) for p, a, b in dumps]
    jc = _capi.JcContext(device)
    try:
        names = []
        for path, a, b in dumps:
            if os.path.getsize(path) == 0:
                continue
            ids = []
            for name in (a, b):
                if name not in names:
                    names.append(name)
                ids.append(names.index(name))
            try:
                jc.convert_file(path, a, b, resolution, ids, keep_text=keep_text, keep_rows=True)
            except _capi.JcRefused as e:
                raise _refusal(path, e) from None
        return JuicerContacts(jc, resolution, names)
    except BaseException:
        jc.close()
        raise


def convert(path, chr1, chr2, out, resolution=None, device=0):
    """What the two command lines do: one dump -> `out`.  resolution=None is verbatim mode (gzip, the names as given); otherwise
    midpoint mode (`chr` + name; plain text, gzip when `out` ends in .gz).  Returns the number of lines.  A refused dump leaves
    nothing written."""
    check_name(chr1)
    check_name(chr2)
    if resolution is not None:
        check_resolution(resolution)
        chr1, chr2 = "chr" + chr1, "chr" + chr2
    jc = _capi.JcContext(device)
    try:
        try:
            n = jc.convert_file(path, chr1, chr2, resolution or 0)
        except _capi.JcRefused as e:
            raise _refusal(path, e) from None
        _write(out, jc.text(), resolution is None or os.fspath(out).endswith(".gz"))
        return n
    finally:
        jc.close()


def parse_args(argv):
    parser = argparse.ArgumentParser(description="Check help flag")
    parser.add_argument("--dump", help="Text printed by `juicer_tools dump` / `straw` for the pair. Mandatory parameter.", required=True)
    parser.add_argument("--CHR1", help="Chromosome 1. Mandatory parameter.", required=True)
    parser.add_argument("--CHR2", help="Chromosome 2. Mandatory parameter.", required=True)
    parser.add_argument("--resolution", help="Resolution of the dumped contact matrix (in bp). Mandatory parameter.", type=int, required=True)
    parser.add_argument("--datatype", help="Type of contact that was dumped (echoed).", default="observed")
    parser.add_argument("--Norm", help="Type of normalization that was dumped (echoed); only a raw (NONE) dump is taken.", default="KR")
    parser.add_argument("--outFile", help="Output file for storing contact counts", required=True)
    return parser.parse_args(argv)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) == 4 and not any(a.startswith("--") for a in argv):         # createFitHiCContacts-hic_old.sh DUMP CHR1 CHR2 OUT
        convert(argv[0], argv[1], argv[2], argv[3])
        return
    if not any(a.startswith("--") for a in argv):
        sys.exit("usage: python -m fithic_amd.juicer DUMP CHR1 CHR2 OUT\n"
                 "       python -m fithic_amd.juicer --dump DUMP --CHR1 A --CHR2 B --resolution R --outFile OUT")
    args = parse_args(argv)
    dump, out = os.path.realpath(args.dump), os.path.realpath(args.outFile)
    print("dump: %s" % dump)                                         # createFitHiCContacts-hic.py:44-75
    print("CHR1: %s" % args.CHR1)
    print("CHR2: %s" % args.CHR2)
    print("resolution: %s" % args.resolution)
    print("OutFile: %s" % out)
    print("datatype: %s" % args.datatype)
    print("Norm: %s" % args.Norm)
    convert(dump, args.CHR1, args.CHR2, out, args.resolution)


if __name__ == "__main__":
    main()
