"""fithic_amd.fragpairs restated in plain Python - bisect, a dict, sorted: what the device path must compute, byte for byte.  The
reference has no script for this step; the semantics are those of the module's docstring and of include/fithic_mi355x.h
(FHX_FP_*).  The table comes from tests/digest_model.py's contigs() or from a bed file.  Not a test."""
import bisect
import gzip

import digest_model as dm

(OK, TOKENS, NAME, POSITION, RANGE, BYTES, LONG_LINE, COUNT, INTERNAL, PAIRS) = range(10)
MAX_LINE = 4096
MAX_CONTIGS, MAX_NAME = 4096, 63


class Refused(Exception):
    def __init__(self, why, line=0):
        super().__init__("reason %d at line %d" % (why, line))
        self.why, self.line = why, line


def table_of_contigs(contigs):
    """digest_model.contigs() -> [(name as bytes, E_c)]: a contig's sites with duplicates kept, then its length"""
    return [(name.encode("latin-1"), list(cuts) + [length]) for name, length, cuts in contigs]


def table_of_fasta(data, sites):
    return table_of_contigs(dm.contigs(data, sites))


def table_of_bed(bed):
    """the bytes of a bed file -> [(name, E_c)], contigs in order of first appearance; ValueError("line N: ...") for a file that is
    no digest's bed"""
    out, seen = [], set()
    for number, line in enumerate(dm.lines_of(bed), 1):
        tokens = line.split()
        if len(tokens) < 3:
            raise ValueError("line %d: tokens" % number)
        name, start, end = tokens[0].encode("latin-1"), tokens[1], tokens[2]
        for t in (start, end):
            if not (t.isdigit() and t.isascii() and len(t) <= 10):
                raise ValueError("line %d: number" % number)
        start, end = int(start), int(end)
        if end > 0x7fffffff:
            raise ValueError("line %d: number" % number)
        if not out or out[-1][0] != name:
            if name in seen:
                raise ValueError("line %d: name comes back" % number)
            seen.add(name)
            out.append((name, []))
            if start != 0:
                raise ValueError("line %d: first start" % number)
        elif start != out[-1][1][-1]:
            raise ValueError("line %d: start is not the previous end" % number)
        if end < start:
            raise ValueError("line %d: end below start" % number)
        out[-1][1].append(end)
    return out


def check_limits(table):
    if len(table) > MAX_CONTIGS:
        raise ValueError("contigs")
    if any(len(name) > MAX_NAME for name, _ in table):
        raise ValueError("name")
    if sum(len(ends) for _, ends in table) >= 1 << 31:
        raise ValueError("fragments")


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
    return 0, [t for t in content.replace(b"\t", b" ").split(b" ") if t]


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


def pairs(data, table, drop=()):
    """([(g1, g2)] of the kept pairs in file order, counts); Refused for the first line outside the grammar"""
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    drop = set(drop)
    contig = {name: c for c, (name, _) in enumerate(table)}
    first = [0]
    for _, ends in table:
        first.append(first[-1] + len(ends))
    out, counts = [], dict(lines=0, pairs=0, dropped_name=0, same_fragment=0, cells=0)
    for number, (content, ended) in enumerate(lines_of(data), 1):
        why, tokens = _walk(content, ended)
        if why:
            raise Refused(why, number)
        if len(tokens) < 6:
            raise Refused(TOKENS, number)
        counts["lines"] += 1
        n1, p1, n2, p2 = tokens[1], tokens[2], tokens[4], tokens[5]
        if n1 in drop or n2 in drop:                                  # the line is not read further
            counts["dropped_name"] += 1
            continue
        if n1 not in contig or n2 not in contig:
            raise Refused(NAME, number)
        if not (p1.isdigit() and p2.isdigit() and len(p1) <= 10 and len(p2) <= 10):
            raise Refused(POSITION, number)
        g = []
        for name, p in ((n1, int(p1)), (n2, int(p2))):
            ends = table[contig[name]][1]
            if p < 1 or p > ends[-1]:
                raise Refused(RANGE, number)
            g.append(first[contig[name]] + bisect.bisect_left(ends, p))     # start < p <= end
        if g[0] == g[1]:
            counts["same_fragment"] += 1
            continue
        counts["pairs"] += 1
        out.append((min(g), max(g)))
    return out, counts


def cells(data, table, drop=()):
    """([(c1, E[g1], c2, E[g2], count)] in ascending (g1, g2), counts)"""
    kept, counts = pairs(data, table, drop)
    counted = {}
    for key in kept:
        counted[key] = counted.get(key, 0) + 1
    row = [(c, e) for c, (_, ends) in enumerate(table) for e in ends]
    out = [row[g1] + row[g2] + (counted[(g1, g2)],) for g1, g2 in sorted(counted)]
    if any(c[4] > 0x7fffffff for c in out):
        raise Refused(COUNT)
    counts["cells"] = len(out)
    return out, counts


def text(data, table, drop=()):
    """the decompressed bytes of the written file"""
    return b"".join(b"chr%d\t%d\tchr%d\t%d\t%d\n" % (c1 + 1, e1, c2 + 1, e2, n) for c1, e1, c2, e2, n in cells(data, table, drop)[0])


def columns(data, table, drop=()):
    """the five columns as fithic_amd.fragpairs returns them"""
    cs = cells(data, table, drop)[0]
    return [[c[k] for c in cs] for k in range(5)]
