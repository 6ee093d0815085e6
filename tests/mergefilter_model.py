"""The selection of merge-filter.sh restated in plain Python (reference: fithic/utils/merge-filter.sh:22 run with mawk 1.3.4 under
LC_ALL=C): what fithic_amd.mergefilter and csrc/fhx_sigselect.hip must give, byte for byte.  Pinned to the real script by
tests/golden/mergefilter and to the installed awk by tests/test_mergefilter_host.py.

A field 7 in the shape C's %e writes falls in one of three classes:
  zero     every digit 0: the number 0;
  numeric  first digit 1-9, value in [2.225074e-308, 9.999999e+307]: awk compares numbers - here float(field) against float(fdr);
  string   a non-zero value below 2.225074e-308 or an exponent of 309 and more: mawk's strtod flags ERANGE, the field is no
           number to awk and is compared bytewise with the text of fdr.
An exponent of exactly 308 is refused (mawk: numbers up to 1.797693e+308, strings above).  Everything the grammar leaves out
is refused with the smallest offending 1-based line number.
"""
import re

TOKENS, FIELD, BYTES, LONG_LINE, FDR = 1, 2, 3, 4, 5
MAX_LINE = 4096
FDR_BYTES = 32
_SHAPE = re.compile(rb"([0-9])\.([0-9]{6})e([+-])([0-9]{2,3})\Z")
_FDR = re.compile(rb"(?:[0-9]+(?:\.[0-9]+)?|\.[0-9]+)(?:e[+-]?[0-9]+)?\Z")
_BAD_BYTE = re.compile(rb"[^\t\x20-\x7e]")


class Refused(ValueError):
    def __init__(self, why, line):
        super().__init__("reason %d at line %d" % (why, line))
        self.why, self.line = why, line


def check_fdr(fdr):
    """the bytes of the threshold; Refused(FDR, 0) outside the grammar"""
    text = fdr.encode("ascii", "replace") if isinstance(fdr, str) else bytes(fdr)
    if len(text) > FDR_BYTES or not _FDR.match(text):
        raise Refused(FDR, 0)
    value = float(text)
    if value != 0 and not 2.2250738585072014e-308 <= value < float("inf"):
        raise Refused(FDR, 0)
    return text


def classify(field):
    """-> "zero", "numeric", "string", or None for a field that is refused"""
    m = _SHAPE.match(field)
    if not m:
        return None
    digits = int(m.group(1) + m.group(2))
    if digits == 0:
        return "zero"
    if m.group(1) == b"0":
        return None
    exponent = int(m.group(4)) * (-1 if m.group(3) == b"-" else 1)
    if exponent == 308:
        return None
    if exponent > 308 or (exponent, digits) < (-308, 2225074):
        return "string"
    return "numeric"


def keeps(field, fdr, strict=False):
    """awk's `$7 <= q` (`$7 < q`) for a field of one of the three classes"""
    cls = classify(field)
    if cls == "string":                                              # bytes objects compare as memcmp does, then by length
        return field < fdr if strict else field <= fdr
    value = 0.0 if cls == "zero" else float(field)
    return value < float(fdr) if strict else value <= float(fdr)


def lines_of(data):
    """the lines without their newlines; a newline that ends the text starts no line"""
    if not data:
        return []
    return (data[:-1] if data.endswith(b"\n") else data).split(b"\n")


def select(data, fdr, strict=False, skip_first_line=True):
    """the subset: the kept lines verbatim, in order, each ending in a newline"""
    fdr = check_fdr(fdr)
    out = []
    for number, line in enumerate(lines_of(data), 1):
        bad = _BAD_BYTE.search(line)
        if bad and bad.start() < MAX_LINE:
            raise Refused(BYTES, number)
        if len(line) > MAX_LINE:
            raise Refused(LONG_LINE, number)
        if skip_first_line and number == 1:
            continue
        tokens = line.replace(b"\t", b" ").split()
        if len(tokens) < 7:
            raise Refused(TOKENS, number)
        if classify(tokens[6]) is None:
            raise Refused(FIELD, number)
        if keeps(tokens[6], fdr, strict):
            out.append(line + b"\n")
    return b"".join(out)
