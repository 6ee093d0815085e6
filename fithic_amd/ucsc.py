"""visualize-UCSC.sh on the MI355X engine: the UCSC `interact` track of the rows of a significances file with `q < QVALTHRESH`
(reference: fithic/utils/visualize-UCSC.sh), same positional arguments, same file.

    python -m fithic_amd.ucsc INPUT OUTPUT QVALTHRESH

OUTPUT is plain text and, byte for byte, what the script writes under LC_ALL=C with mawk 1.3.4: its two fixed lines, then for
every kept row
    $1 ($2-1) ($4+1) NR int(-log($7)/log(10)) -log($7)/log(10) EXP 0 $1 ($2-1) ($2+1) SOURCE_NAME . $3 ($4-1) ($4+1) TARGET_NAME +
joined by single blanks, NR counting the kept rows from 1.  INPUT may be gzipped or plain (the script's zcat takes only the first).

Selection, grammar and formatting run in kernels (csrc/fhx_sigtrack.inc behind the selection of csrc/fhx_sigselect.hip):
  * the selection is mergefilter's made strict (`$7 < q`) with no line skipped: a data row on line 1 is kept when it passes.  A
    real fithic header has `q-value` as field 7, a string to awk, and a letter sorts above every threshold of the accepted
    grammar: on line 1, and only there, a field 7 that starts with an ASCII letter drops the line;
  * the score is what awk computes with the host's libm, `-log(strtod($7))/log(10)`, printed once through int() and once through
    awk's number printing (%d when integral, else %.6g), and its text depends on libm to the last bit: 1.000000e-03 gives `2 3`.
    The kernel writes the two fields only where an error bound certifies them (csrc/fhx_score.hpp).  Every other kept row - every
    power of ten, every subnormal or overflowing field the string comparison kept - is deferred: its field 7 goes to the host,
    which makes awk's own calls, and the line is completed on the device.  `n_deferred` counts these rows;
  * a q of zero gives `inf inf`, a q of 1 gives `0 0`, q above 1 a negative value behind an int() that truncates toward zero.

Known deviations: nothing is approximated, so a file outside the device grammar is refused with a ValueError that names the
first such line, and nothing is written.  Refused although the script takes them: everything fithic_amd.mergefilter refuses (the
shape of field 7, exponent 308, fewer than 7 tokens, lines of more than 4096 bytes, bytes outside printable ASCII and tab, the
grammar of the threshold); a token 2 or 4 that is not 1 to 9 ASCII digits without a sign (leading zeros are taken: 007 is 7;
awk prints $4+1 as 2.14748e+09 from 2^31 - 1 on, and takes signs, fractions and text); a token 1 or 3 of more than 63 bytes;
more than 2^31 - 1 kept rows (awk prints NR through %.6g from there).  These rules hold for every parsed line, kept or not; a
line 1 dropped by the header rule only has to satisfy the byte, length and token-count rules.  There is no CPU implementation
here: without the library or a GPU the entry points raise.

`fithic --significant FDR --significant-track` and Engine.track make the same track straight from a pass's resident q-values
(csrc/fhx_sigresident_track.inc), without the significances file being written or read back.
"""
import sys

from . import _capi, mergefilter

_ACCEPTS = mergefilter._ACCEPTS.replace("fithic_amd.mergefilter", "fithic_amd.ucsc")


def _refusal_kept(path):
    return ValueError("%s: more than 2^31 - 1 rows pass the threshold" % path + _ACCEPTS)


def _refusal(path, e):
    """the exception a refused file is reported with (module docstring, `Known deviations`)"""
    if e.why == _capi.MS_KEPT:
        return _refusal_kept(path)
    if e.why not in (_capi.MS_MIDPOINT, _capi.MS_NAME):
        inherited = mergefilter._refusal(path, e)
        if isinstance(inherited, ValueError):
            return ValueError(str(inherited).replace("fithic_amd.mergefilter", "fithic_amd.ucsc"))
        return inherited
    with open(path, "rb") as f:
        gzipped = f.read(2) == b"\x1f\x8b"
    text = mergefilter._line_of(path, e.line).decode("latin-1") if not gzipped else ""
    return _refusal_at("%s, line %d" % (path, e.line), e.why, text)


def _refusal_at(where, why, text):
    """the ValueError for reason `why` at `where` ("<file>, line <n>"), `text` being the line when it is at hand ("" for a gzipped
    file and for a line that was never written: Engine.track)"""
    if why not in (_capi.MS_MIDPOINT, _capi.MS_NAME):
        return ValueError(str(mergefilter._refusal_at(where, why, text)).replace("fithic_amd.mergefilter", "fithic_amd.ucsc"))
    if why == _capi.MS_MIDPOINT:
        return ValueError("%s: fragmentMid1 and fragmentMid2 (tokens 2 and 4) are expected as 1 to 9 digits without a sign: %r"
                          % (where, text[:80]) + _ACCEPTS)
    return ValueError("%s: a chromosome name (token 1 or 3) of more than 63 bytes: %r" % (where, text[:80]) + _ACCEPTS)


class Track:
    """The interact track of one significances file."""

    def __init__(self, text, counts, seconds, device):
        self._text, self._seconds, self.device = text, seconds, device
        self.n_lines, self.n_kept, self.n_deferred = counts["lines"], counts["kept"], counts["deferred"]

    def text(self):
        """the whole file, the two fixed lines included"""
        return self._text

    def stage_seconds(self):
        return dict(self._seconds)

    def write(self, path):
        with open(path, "wb") as f:
            f.write(self._text)


def track(path, qval, device=0):
    """The interact track of the rows of `path` (plain or gzipped) with field 7 < qval as mawk decides it, made on GPU `device`;
    `qval` is text, the way the shell passes it."""
    text = mergefilter.fdr_text(qval)
    bound = mergefilter.key_bound(text, strict=True)
    ms = _capi.MsContext(device)
    try:
        try:
            ms.track_file(path, text, bound, 0 < float(text))
        except _capi.MsRefused as e:
            raise _refusal(path, e) from None
        return Track(ms.track(), ms.track_counts(), ms.track_stage_seconds(), device)
    finally:
        ms.close()


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 3:
        sys.exit("usage: python -m fithic_amd.ucsc INPUT OUTPUT QVALTHRESH")
    track(argv[0], argv[2]).write(argv[1])                            # a refused input leaves nothing written


if __name__ == "__main__":
    main()
