"""validPairs2FitHiC-fixedSize.sh restated in plain Python: what fithic_amd.validpairs must compute, byte for byte.

The script's pipeline (fithic/utils/validPairs2FitHiC-fixedSize.sh:33-40) under LC_ALL=C, with the grammar and the refusals of
include/fithic_mi355x.h (FHX_VP_*).  test_validpairs_host.py pins this model to fixtures made by the real script; the GPU tests
compare the device path with this model."""
import gzip

(OK, TOKENS, NAME, POSITION, RANGE, BYTES, LONG_LINE, NAMES, COUNT, RES, INTERNAL, PAIRS) = range(12)
MAX_LINE = 4096
MAX_NAMES = 1024


class Refused(Exception):
    def __init__(self, why, line=0):
        super().__init__("reason %d at line %d" % (why, line))
        self.why, self.line = why, line


def _name_ok(name):
    """the names the grammar takes: awk compares every other one as a number, or might"""
    if name[:1].isdigit():
        return name.isdigit() and (len(name) == 1 or name[0] != ord("0"))
    if not (name[:1].isalpha() or name[:1] == b"_"):
        return False
    return name[:3].lower() not in (b"inf", b"nan")


def _awk_less(a, b):
    """awk's a < b on two fields of the grammar (:37): numeric when both look like numbers, bytewise otherwise"""
    if a.isdigit() and b.isdigit():
        return int(a) < int(b)
    return a < b


def _walk(content, ended):
    """one line without its \\n (ended: a \\n follows it): (reason or 0, tokens).  The bytes are looked at from the left, as the
    kernel's lane does."""
    for i, c in enumerate(content):
        if i >= MAX_LINE:
            return LONG_LINE, None
        if c == 13 and ended and i + 1 == len(content):
            content = content[:i]                                     # \\r\\n
            break
        if (c < 0x20 and c != 9) or c >= 0x7f:                        # a \\r that is not part of \\r\\n among them
            return BYTES, None
    return 0, content.replace(b"\t", b" ").split(b" ")


def lines_of(data):
    if not data:
        return []
    lines = data.split(b"\n")
    if data.endswith(b"\n"):
        lines.pop()
        ended = [True] * len(lines)
    else:
        ended = [True] * (len(lines) - 1) + [False]
    return list(zip(lines, ended))


def pairs(data, res):
    """the kept pairs after filters, binning and end order: [(name1, bin1, name2, bin2)] in file order"""
    if res < 2 or res % 2:
        raise Refused(RES)
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)                                  # zcat -f (:33)
    out = []
    for number, (content, ended) in enumerate(lines_of(data), 1):
        why, tokens = _walk(content, ended)
        if why:
            raise Refused(why, number)
        tokens = [t for t in tokens if t]
        if len(tokens) < 6:
            raise Refused(TOKENS, number)
        n1, p1, n2, p2 = tokens[1], tokens[2], tokens[4], tokens[5]
        if len(n1) > 5 or len(n2) > 5 or b"chrM" in content:           # :34
            continue
        if not _name_ok(n1) or not _name_ok(n2):
            raise Refused(NAME, number)
        if not (p1.isdigit() and p2.isdigit() and len(p1) <= 10 and len(p2) <= 10):
            raise Refused(POSITION, number)
        p1, p2 = int(p1), int(p2)
        b1, b2 = p1 // res * res, p2 // res * res                     # :36
        if b1 + res // 2 >= 1 << 31 or b2 + res // 2 >= 1 << 31:
            raise Refused(RANGE, number)
        if n1 == n2 and not (p1 - p2) ** 2 > 2 * res:                 # :35: sqrt(($3-$6)^2>t) - the comparison is inside
            continue
        if (b1 <= b2) if n1 == n2 else _awk_less(n1, n2):             # :37
            out.append((n1, b1, n2, b2))
        else:
            out.append((n2, b2, n1, b1))
    names = set(p[0] for p in out) | set(p[2] for p in out)
    if len(names) > MAX_NAMES:
        raise Refused(NAMES)
    return out


def cells(data, res):
    """[(name1, mid1, name2, mid2, count)] in the order of `sort | uniq -c` under LC_ALL=C (:38)"""
    counted = {}
    for n1, b1, n2, b2 in pairs(data, res):
        line = b"%s\t%d\t%s\t%d" % (n1, b1, n2, b2)
        counted[line] = counted.get(line, 0) + 1
    out = []
    for line in sorted(counted):
        n1, b1, n2, b2 = line.split(b"\t")
        out.append((n1, int(b1) + res // 2, n2, int(b2) + res // 2, counted[line]))
    return out


def text(data, res):
    """the decompressed bytes of LIBNAME_fithic.contactCounts.gz (:39): uniq -c's count field keeps its leading blanks"""
    return b"".join(b"%s\t%d\t%s\t%d\t%7d\n" % c for c in cells(data, res))


def columns(data, res):
    """names in bytewise order and the five columns, as fithic_amd.validpairs returns them"""
    cs = cells(data, res)
    names = sorted(set(c[0] for c in cs) | set(c[2] for c in cs))
    rank = {n: k for k, n in enumerate(names)}
    return ([n.decode() for n in names], [rank[c[0]] for c in cs], [c[1] for c in cs], [rank[c[2]] for c in cs], [c[3] for c in cs],
            [c[4] for c in cs])
