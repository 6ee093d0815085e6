"""visualize-UCSC.sh restated in plain Python (reference: fithic/utils/visualize-UCSC.sh:16-18 run with mawk 1.3.4 under LC_ALL=C):
what fithic_amd.ucsc and csrc/fhx_sigtrack.inc must give, byte for byte.  Pinned to the real script by tests/golden/ucsc and to
the installed awk by tests/test_ucsc_host.py.

The selection is mergefilter_model's, strict and with no line skipped, plus the header rule: on line 1 only, a field 7 that
starts with an ASCII letter is a string above every accepted threshold and the line is dropped.  The score of a kept row is
v = -log(float(field)) / log(10) with the host's libm, printed as int(v) (truncation toward zero) and as v, each the way awk
prints a number: %d when it is integral and below 2^31 in magnitude, %.6g otherwise.  Beyond mergefilter_model's grammar, on
every parsed line: tokens 2 and 4 are 1 to 9 digits, tokens 1 and 3 at most 63 bytes.
"""
import math
import re

import mergefilter_model as mm
from mergefilter_model import BYTES, FDR, FIELD, LONG_LINE, TOKENS, Refused          # noqa: F401

MIDPOINT, NAME = 7, 8
HEAD = (b'track type=interact name="Your_Fit-Hi-C_Interactions" description="Fit-Hi-C_Interactions" interactDirectional=true '
        b'useScore=on maxHeightPixels=50:100:200 visibility=full\n'
        b'#chrom  chromStart  chromEnd  name  score  value  exp  color  sourceChrom  sourceStart  sourceEnd  sourceName  sourceStrand  '
        b'targetChrom  targetStart  targetEnd  targetName  targetStrand\n')
_MID = re.compile(rb"[0-9]{1,9}\Z")


def awk_number(v):
    """a number as mawk's print writes it"""
    if math.isinf(v):
        return "inf" if v > 0 else "-inf"
    if v == int(v) and abs(v) < 2 ** 31:
        return "%d" % int(v)
    return "%.6g" % v


def score_fields(field):
    """the two score fields of a kept row, as text"""
    q = float(field)
    v = math.inf if q == 0 else -math.log(q) / math.log(10)
    return awk_number(float(math.trunc(v)) if math.isfinite(v) else v), awk_number(v)


def track(data, qval):
    """-> (the whole file, the number of kept rows)"""
    qval = mm.check_fdr(qval)
    out, nr = [HEAD], 0
    for number, line in enumerate(mm.lines_of(data), 1):
        bad = mm._BAD_BYTE.search(line)
        if bad and bad.start() < mm.MAX_LINE:
            raise Refused(BYTES, number)
        if len(line) > mm.MAX_LINE:
            raise Refused(LONG_LINE, number)
        tokens = line.replace(b"\t", b" ").split()
        if len(tokens) < 7:
            raise Refused(TOKENS, number)
        if number == 1 and tokens[6][:1].isalpha():
            continue
        if mm.classify(tokens[6]) is None:
            raise Refused(FIELD, number)
        if not _MID.match(tokens[1]) or not _MID.match(tokens[3]):
            raise Refused(MIDPOINT, number)
        if len(tokens[0]) > 63 or len(tokens[2]) > 63:
            raise Refused(NAME, number)
        if not mm.keeps(tokens[6], qval, strict=True):
            continue
        nr += 1
        c1, c2, m1, m2 = tokens[0].decode("latin-1"), tokens[2].decode("latin-1"), int(tokens[1]), int(tokens[3])
        out.append(" ".join([c1, str(m1 - 1), str(m2 + 1), str(nr), *score_fields(tokens[6]), "EXP", "0", c1, str(m1 - 1), str(m1 + 1),
                             "SOURCE_NAME", ".", c2, str(m2 - 1), str(m2 + 1), "TARGET_NAME", "+"]).encode("latin-1") + b"\n")
    return b"".join(out), nr


# ---- fields whose score lies next to a boundary: shared by the CPU and the GPU tests -----------------------------------------
_NEAR = {}


def near_boundary_fields(exponents=(-1, -5, -17, -120), each=200):
    """For every exponent x, the `each` fields D.DDDDDDe<x> whose score lies closest to an integer or to a rounding boundary of
    %.6g, found by a scan over all 9 * 10^6 mantissas; made once."""
    import numpy as np
    key = (tuple(exponents), each)
    if key not in _NEAR:
        m = np.arange(1000000, 10000000, dtype=np.float64)
        fields = []
        for x in exponents:
            t = np.abs((6 - x) - np.log10(m))
            near_integer = np.abs(t - np.rint(t))
            with np.errstate(divide="ignore"):
                scale = 10.0 ** (5 - np.floor(np.log10(t)))
            s = t * scale
            near_cell = np.abs(s - np.floor(s) - 0.5) / scale
            d = np.minimum(near_integer, near_cell)
            d[~np.isfinite(d)] = 0                                    # the power of ten itself
            nearest = np.argpartition(d, each)[:each]
            for i in nearest[np.argsort(d[nearest], kind="stable")]:
                mant = int(m[i])
                fields.append(("%d.%06de%s%02d" % (mant // 1000000, mant % 1000000, "-" if x < 0 else "+", abs(x))).encode())
        _NEAR[key] = fields
    return list(_NEAR[key])


def rows_of(fields, seps=(b"\t", b" ", b"  ", b" \t")):
    """one significances row per field 7"""
    return b"".join(seps[k % len(seps)].join([b"chr%d" % (1 + k % 3), b"%d" % (5000 * (k % 900) + 2500), b"chr%d" % (1 + k % 5),
                                             b"%d" % (5000 * (k % 900 + k % 7 + 3) + 2500), b"%d" % (5 + k % 90), b"1.000000e-09", f, b"1.000000", b"x"])
                    + b"\n" for k, f in enumerate(fields))
