"""validPairs2FitHiC-fixedSize.sh on the MI355X engine: HiC-Pro's allValidPairs (one line per read pair) binned into the
contact counts `fithic` reads (reference: fithic/utils/validPairs2FitHiC-fixedSize.sh), same positional arguments, same
progress lines, same file name.

    python -m fithic_amd.validpairs 10000 sample sample.allValidPairs outdir

writes outdir/sample_fithic.contactCounts.gz; its decompressed bytes are the script's under LC_ALL=C with mawk 1.3.4 (the
script's `sort` follows the locale and its awk prints large numbers its own way: both are pinned here).  The file - 1e8 to 1e9
lines - is filtered, binned, sorted and counted by kernels (csrc/fhx_validpairs.hip); `read()` keeps the cells in HBM and hands
them to an Engine without the file ever existing.

Known deviations: nothing is approximated, so a file outside the device grammar is refused with a ValueError that names the
first such line, and nothing is written.  Refused although the script takes them: an odd resolution or one below 2 (the script
prints fractions there), a position with a sign, a point or an exponent or one whose bin midpoint reaches 2^31 (mawk prints
2.14748e+09), a chromosome name that awk compares as a number or might (one that starts with a digit, a sign or a point and
is not a plain digit string without a leading zero; one that starts with inf or nan), a line of fewer than 6 tokens (an empty
one included), of more than 4096 bytes or with a control or non-ASCII byte, more than 1024 distinct names.  Names and positions
are only looked at on lines that pass the script's first two filters (both names of at most 5 bytes, no `chrM` anywhere in the
line): the script never reads them on the others.  There is no CPU implementation here: without the library or a GPU the
entry points raise.
"""
import os
import sys

from . import _capi
from ._resident import Resident, _is_gzip
from .hicpro import _line_of


def _refusal(path, res, e):
    """the exception a refused file is reported with (module docstring, `Known deviations`)"""
    accepts = ".  The reference accepts this; fithic_amd.validpairs does not take it."
    if e.why == _capi.VP_RES:
        return ValueError("resolution %r: an even number of at least 2 is expected (the script prints half a resolution as a "
                          "fraction)" % (res,) + accepts)
    if e.why == _capi.VP_NAMES:
        return ValueError("%s: more chromosome names (at most 1024) or larger bin indices than the 64-bit sort key holds: %s"
                          % (path, e) + accepts)
    if e.why == _capi.VP_COUNT:
        return ValueError("%s: a cell is hit by more than 2^31 - 1 pairs; the count column is int32" % path + accepts)
    if e.why == _capi.VP_PAIRS:
        return ValueError("%s: 2^32 or more pairs pass the filters; the sort does not take them" % path + accepts)
    if e.why == _capi.VP_INTERNAL:
        return e
    where = "%s, line %d" % (path, e.line)
    text = _line_of(path, e.line).decode("latin-1") if not _is_gzip(path) else ""
    if e.why == _capi.VP_BYTES:
        return ValueError("%s: a NUL, a control byte other than tab, a non-ASCII byte or a \\r that is not part of \\r\\n: %r"
                          % (where, text[:80]))
    if e.why == _capi.VP_LONG_LINE:
        return ValueError("%s: a line of more than 4096 bytes" % where)
    if e.why == _capi.VP_TOKENS:
        return ValueError("%s: %d token(s) where at least 6 are expected (read chr1 pos1 strand1 chr2 pos2): %r"
                          % (where, len(text.split()), text[:80]))
    what = {_capi.VP_NAME: "a chromosome name that awk compares as a number, or might (it starts with a digit, a sign, a point, "
                           "inf or nan and is not a plain digit string without a leading zero)",
            _capi.VP_POSITION: "a position that is not written as 1 to 10 digits",
            _capi.VP_RANGE: "a position whose bin midpoint reaches 2^31 (awk prints it in %.6g form)"}.get(
                e.why, "a line outside the device grammar")
    return ValueError("%s: %s: %r" % (where, what, text[:80]) + accepts)


class ValidPairs(Resident):
    """One binned validPairs file: the cells (chr1, mid1, chr2, mid2, count) resident in HBM, in the script's output order.
    load_into: the cells into a configured Engine whose fragments are loaded."""

    def __init__(self, vp, res, n_cells, names):
        super().__init__(vp, n_cells, names)
        self.res, self.n_cells = res, n_cells

    def write(self, path):
        _capi.vp_write_contacts(path, self.names, *self.contacts())


def read(path, res, device=0):
    """The direct path: a validPairs file (plain or gzipped) -> a ValidPairs whose cells stay on GPU `device`."""
    vp = _capi.VpContext(device)
    try:
        try:
            n = vp.bin_file(path, res)
        except _capi.VpRefused as e:
            raise _refusal(path, res, e) from None
        return ValidPairs(vp, int(res), n, vp.names())
    except BaseException:
        vp.close()
        raise


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 4:
        sys.exit("usage: python -m fithic_amd.validpairs RESOLUTION LIBNAME VALIDPAIRS OUTDIR")
    res, lib_name, path, outdir = int(argv[0]), argv[1], argv[2], argv[3]
    print("The resolution given is %d" % res)                      # validPairs2FitHiC-fixedSize.sh:16-20
    print("Library name is %s" % lib_name)
    print("The lower distance threshold is %d" % (res * 2))
    with read(path, res) as data:
        data.write(os.path.join(outdir, lib_name + "_fithic.contactCounts.gz"))


if __name__ == "__main__":
    main()
