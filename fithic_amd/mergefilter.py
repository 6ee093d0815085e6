"""merge-filter.sh on the MI355X engine: the rows of a significances file with `q <= fdr`, then the merging of neighbours
(reference: fithic/utils/merge-filter.sh), same positional arguments, same two files.

    python -m fithic_amd.mergefilter INPUT RESOLUTION OUTPUT FDR [UTILITYFOLDER]

makes dirname(OUTPUT), writes dirname(OUTPUT)/fithic_subset.gz and writes OUTPUT through fithic_amd.combine with the script's
settings (-H 0, connectivity 8, percent 100, neighbourhood 2, order 0).  The fifth argument is accepted and ignored: the script
never reads it either (it sets `utilityfolder` and uses `$UTILITYFOLDER`).  Both files, decompressed, are the script's bytes
under LC_ALL=C with mawk 1.3.4.  INPUT may be gzipped or plain (the script's zcat takes only the first).

The selection runs in kernels (csrc/fhx_sigselect.hip) and is made on the TEXT of field 7, as awk makes it:
  * line 1 is dropped whatever it holds; kept lines are copied verbatim, a last line without its newline gets one;
  * a field mawk's strtod flags ERANGE for - every subnormal (2.225074e-308 is a number, 2.225073e-308 is not) and every
    exponent above the double range - is compared as a STRING with the text of fdr: with fdr = 0.05 a row whose q is
    1.000000e-320 is dropped ('1' > '0'), with fdr = 5 it is kept;
  * everything else is compared as a number, through one integer key per field and a bound found here by bisection with float().
`select(..., strict=True, skip_first_line=False)` is the selection visualize-UCSC.sh makes (`$7 < q`, no header drop); the
interact track itself is written by fithic_amd.ucsc.

The script hands the subset to Combine with -H 0, and Combine then lists the chromosomes with `cut -f1 | sort -k1,1 | uniq`:
cut splits at TABS only, so a kept line without a tab is listed whole, its first token is taken as one more chromosome to
process, and that chromosome's merged rows are written once more.  A file fithic wrote is tab-separated and has none of this;
on a file with blanks as separators OUTPUT repeats rows exactly as the script's does (`Selection.chromosome_passes`).

No row passes: the script's Combine writes OUTPUT holding only its header line (no newline after it), and so does this
module; fithic_subset.gz is then an empty gzip file.

Known deviations: nothing is approximated, so a file outside the device grammar is refused with a ValueError that names the
first such line, and nothing is written.  Refused although the script takes them: a field 7 that is not in the shape C's %e
writes for a non-negative finite double, D.DDDDDDe[+-]XX or e[+-]XXX (a sign, nan, inf, a first digit 0 before non-zero
digits, other widths), or whose exponent is exactly 308 (mawk compares numbers up to 1.797693e+308 and strings above: the
selection does not rest on where strtod overflows); a line of fewer than 7 tokens (an empty one included; awk compares "" and
keeps it), of more than 4096 bytes, or with a NUL, a non-ASCII byte or a control byte other than tab and newline (\\r is one,
so \\r\\n files are refused); an fdr that is not written digits[.digits][e[+-]digits] or .digits[e[+-]digits], whose value is
non-zero and not a normal double, or that is longer than 32 bytes.  The header line only has to satisfy the byte and length
rules.  There is no CPU implementation here: without the library or a GPU the entry points raise.
"""
import gzip
import math
import os
import re
import sys

from . import _capi
from .hicpro import _line_of

_FDR = re.compile(rb"(?:[0-9]+(?:\.[0-9]+)?|\.[0-9]+)(?:e[+-]?[0-9]+)?\Z")
_ACCEPTS = ".  The reference accepts this; fithic_amd.mergefilter does not take it."
# the numeric class: keys (exponent, seven digits) from 2.225074e-308 to 9.999999e+307, in order
_MANTISSAS = 9000000
_LOWEST = 2225074 - 1000000                                          # index of (-308, 2225074)
_HIGHEST = (307 + 308) * _MANTISSAS + _MANTISSAS - 1                 # index of (307, 9999999)
FLOAT_MIN = 2.2250738585072014e-308


def fdr_text(fdr):
    """the threshold as the bytes the shell passes; ValueError for one outside the grammar"""
    text = fdr.encode("ascii", "replace") if isinstance(fdr, str) else bytes(fdr)
    if len(text) > _capi.MS_FDR_BYTES:
        raise ValueError("fdr %r: longer than %d bytes" % (fdr, _capi.MS_FDR_BYTES) + _ACCEPTS)
    if not _FDR.match(text):
        raise ValueError("fdr %r: digits[.digits][e[+-]digits] or .digits[e[+-]digits] is expected" % (fdr,) + _ACCEPTS)
    value = float(text)
    if value != 0 and (math.isinf(value) or value < FLOAT_MIN):
        raise ValueError("fdr %r: its value is not zero and not a normal double (awk would compare strings)" % (fdr,) + _ACCEPTS)
    return text


def _field(index):
    """the %e text of the index-th numeric key"""
    e, m = divmod(index, _MANTISSAS)
    e -= 308
    m += 1000000
    return "%d.%06de%s%02d" % (m // 1000000, m % 1000000, "-" if e < 0 else "+", abs(e))


def key_of(index):
    e, m = divmod(index, _MANTISSAS)
    return e * 10000000 + m + 1000000                                # (exponent + 308) * 10^7 + the seven digits


def key_bound(fdr, strict=False):
    """The largest key whose field satisfies float(field) <= float(fdr) (< when strict), 0 when none does: float() is monotone in
    the key, so the fields that pass are a prefix of the key order and bisection finds its end."""
    q = float(fdr_text(fdr))
    passes = (lambda i: float(_field(i)) < q) if strict else (lambda i: float(_field(i)) <= q)
    if not passes(_LOWEST):
        return 0
    if passes(_HIGHEST):
        return key_of(_HIGHEST)
    lo, hi = _LOWEST, _HIGHEST                                       # passes(lo), not passes(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if passes(mid):
            lo = mid
        else:
            hi = mid
    return key_of(lo)


def _refusal(path, e):
    """the exception a refused file is reported with (module docstring, `Known deviations`)"""
    if e.why in (_capi.MS_INTERNAL, _capi.MS_FDR):
        return e
    with open(path, "rb") as f:
        gzipped = f.read(2) == b"\x1f\x8b"
    text = _line_of(path, e.line).decode("latin-1") if not gzipped else ""
    return _refusal_at("%s, line %d" % (path, e.line), e.why, text)


def _refusal_at(where, why, text):
    """the ValueError for reason `why` at `where` ("<file>, line <n>"), `text` being the line when it is at hand ("" for a gzipped
    file and for a line that was never written: Engine.significant)"""
    if why == _capi.MS_BYTES:
        return ValueError("%s: a NUL, a non-ASCII byte or a control byte other than tab and newline (\\r is one): %r" % (where, text[:80]))
    if why == _capi.MS_LONG_LINE:
        return ValueError("%s: a line of more than 4096 bytes" % where + _ACCEPTS)
    if why == _capi.MS_TOKENS:
        return ValueError("%s: %d token(s) where at least 7 are expected (chr1 mid1 chr2 mid2 count p q): %r"
                          % (where, len(text.split()), text[:80]) + _ACCEPTS)
    return ValueError("%s: field 7 is not written as %%e writes a non-negative finite double (D.DDDDDDe[+-]XX), or its exponent "
                      "is 308: %r" % (where, text[:80]) + _ACCEPTS)


class Selection:
    """The FDR subset of one significances file: the kept lines, verbatim and in file order."""

    def __init__(self, text, n_lines, n_kept, seconds, device):
        self._text, self.n_lines, self.n_kept, self._seconds, self.device = text, n_lines, n_kept, seconds, device

    def subset_text(self):
        return self._text

    def stage_seconds(self):
        return dict(self._seconds)

    def write_subset(self, path):
        with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=6, mtime=0, filename="") as f:
            f.write(self._text)

    def chromosome_passes(self):
        """The chromosomes in the order, and as often as, the reference's Combine processes them under -H 0: the first tokens of
        `cut -f1 | sort -k1,1 | uniq` over the subset (C locale: bytewise on field 1, leading blanks included, then on the line)."""
        def field1(line):
            i = 0
            while i < len(line) and line[i] == 0x20:
                i += 1
            while i < len(line) and line[i] != 0x20:
                i += 1
            return line[:i]
        firsts = {line.split(b"\t", 1)[0] for line in self._text.split(b"\n")[:-1]}
        passes = []
        for line in sorted(firsts, key=lambda v: (field1(v), v)):
            tokens = line.split()
            if not tokens:
                raise ValueError("a kept line starts with blanks and a tab: the reference's Combine stops with an IndexError there")
            passes.append(tokens[0].decode("latin-1"))
        return passes

    def merged(self, resolution):
        """-> (names, records) of the merged file as the script writes it: combine()'s records, chromosome by chromosome in the
        order of chromosome_passes()"""
        import numpy as np
        names, rec, _ = self.combine(resolution)
        passes = self.chromosome_passes()
        if not len(rec):
            return names, rec
        return names, np.concatenate([rec[rec["chr"] == names.index(c)] for c in passes])

    def combine(self, resolution, conn=8, pct=100, neigh=2, order=0):
        """-> (names, records, info) as combine.combine_records gives them for the subset read with -H 0"""
        from . import combine
        if not self.n_kept:                                          # the reference goes on with no chromosome and no node
            import numpy as np
            return [], np.zeros(0, _capi.CNI_RECORD), _capi.CniInfo()
        return combine.combine_records(combine.frame_of_text(self._text), int(resolution), conn, pct, neigh, order, device=self.device)


def select(path, fdr, strict=False, skip_first_line=True, device=0):
    """The rows of `path` (plain or gzipped) with field 7 <= fdr (< when strict) as mawk decides it, chosen on GPU `device`;
    `fdr` is text, the way the shell passes it."""
    text = fdr_text(fdr)
    bound = key_bound(text, strict)
    zero_kept = 0 < float(text) if strict else 0 <= float(text)
    ms = _capi.MsContext(device)
    try:
        try:
            ms.select_file(path, text, bound, zero_kept, strict, skip_first_line)
        except _capi.MsRefused as e:
            raise _refusal(path, e) from None
        counts = ms.counts()
        return Selection(ms.subset(), counts["lines"], counts["kept"], ms.stage_seconds(), device)
    finally:
        ms.close()


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) not in (4, 5):
        sys.exit("usage: python -m fithic_amd.mergefilter INPUT RESOLUTION OUTPUT FDR [UTILITYFOLDER]")
    path, resolution, out_path, fdr = argv[0], int(argv[1]), argv[2], argv[3]
    from . import combine
    chosen = select(path, fdr)                                       # a refused file leaves nothing behind
    outdir = os.path.dirname(out_path) or "."
    os.makedirs(outdir, exist_ok=True)
    chosen.write_subset(os.path.join(outdir, "fithic_subset.gz"))
    names, rec = chosen.merged(resolution)
    combine.write_merged(out_path, names, rec, resolution)


if __name__ == "__main__":
    main()
