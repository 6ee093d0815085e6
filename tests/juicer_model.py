"""Plain-Python model of the Juicer dump path (fithic_amd.juicer, csrc/fhx_juicer.hip): what createFitHiCContacts-hic_old.sh
(verbatim mode) and createFitHiCContacts-hic.py:93 (midpoint mode) write for the text `juicer_tools dump` prints, and the grammar
with the order of its checks.  No numpy, no library: the tests hold the device and the fixtures of tests/golden/juicer to it."""
import re

(OK, BYTES, LONG_LINE, TOKENS, BIN, GRID, RANGE, COUNT, FRACTION, INTERNAL) = range(10)
MAX_LINE = 4096
INT32_MAX = (1 << 31) - 1
COUNT_MAX = 1 << 24
NAME = re.compile(rb"[A-Za-z0-9_.-]{1,63}\Z")
_TOKEN = re.compile(rb"[^ \t]+")                                     # mawk splits at runs of blank and tab; \r, \f and \v are no separators
_BIN = re.compile(rb"[0-9]{1,10}\Z")
_WHOLE = re.compile(rb"([0-9]+)(\.0+)?\Z")
_NUMBER_BYTES = re.compile(rb"[0-9.+\-eE]+\Z")
_WORDS = re.compile(rb"[+-]?(nan|inf|infinity)\Z", re.IGNORECASE)


class Refused(Exception):
    def __init__(self, why, line):
        super().__init__("reason %d on line %d" % (why, line))
        self.why, self.line = why, line


def check_name(name):
    if not NAME.match(name):
        raise ValueError("chromosome name %r" % (name,))
    return name


def lines_of(data):
    """the lines of a text: they end at \\n, a last line without one counts, an empty text has none"""
    if not data:
        return []
    lines = data.split(b"\n")
    if data.endswith(b"\n"):
        lines.pop()
    return lines


def _refused_byte(c):
    return (c < 0x20 and c != 9) or c >= 0x7f


def reason(line, resolution=None):
    """(why, record) of one line; the checks run in the order of the reason codes.  record: the three fields as text in verbatim
    mode, (mid1, mid2, count) in midpoint mode."""
    if any(_refused_byte(c) for c in line[:MAX_LINE]):               # the walk stops at byte 4096: what lies behind is not looked at
        return BYTES, None
    if len(line) > MAX_LINE:
        return LONG_LINE, None
    tokens = _TOKEN.findall(line)
    if resolution is None:
        return OK, tuple((tokens + [b"", b"", b""])[:3])
    if len(tokens) != 3:
        return TOKENS, None
    x, y, c = tokens
    if not _BIN.match(x) or not _BIN.match(y):
        return BIN, None
    x, y = int(x), int(y)
    if x % resolution or y % resolution:
        return GRID, None
    half = int(resolution / 2)                                       # createFitHiCContacts-hic.py:93
    if x + half > INT32_MAX or y + half > INT32_MAX:
        return RANGE, None
    m = _WHOLE.match(c)
    if m:
        if len(m.group(1)) > 15 or int(m.group(1)) > COUNT_MAX:
            return COUNT, None
        return OK, (x + half, y + half, int(m.group(1)))
    if _WORDS.match(c) or _NUMBER_BYTES.match(c):
        return FRACTION, None
    return COUNT, None


def records(data, resolution=None):
    """the record of every line, or Refused with the smallest offending line"""
    out = []
    for k, line in enumerate(lines_of(data)):
        why, rec = reason(line, resolution)
        if why:
            raise Refused(why, k + 1)
        out.append(rec)
    return out


def convert(data, chr1, chr2, resolution=None):
    """the bytes the script (resolution None) or the .py writes for the dump text `data`"""
    check_name(chr1)
    check_name(chr2)
    if resolution is None:
        return b"".join(b"%s\t%s\t%s\t%s\t%s\n" % (chr1, a, chr2, b, c) for a, b, c in records(data))
    if not 1 <= resolution <= INT32_MAX:
        raise ValueError("resolution %r" % (resolution,))
    return b"".join(b"chr%s\t%d\tchr%s\t%d\t%s\n" % (chr1, m1, chr2, m2, str(float(n)).encode())
                    for m1, m2, n in records(data, resolution))


def columns(dumps, resolution):
    """read()'s table for dumps = [(data, chr1, chr2), ...]: (names, chr1, mid1, chr2, mid2, count) as lists"""
    names, cols = [], [[], [], [], [], []]
    for data, a, b in dumps:
        rows = records(data, resolution)
        if not data:
            continue
        ids = []
        for name in ("chr" + check_name(a).decode(), "chr" + check_name(b).decode()):
            if name not in names:
                names.append(name)
            ids.append(names.index(name))
        for m1, m2, n in rows:
            for col, v in zip(cols, (ids[0], m1, ids[1], m2, n)):
                col.append(v)
    return (names, *cols)
