"""fithic_amd.coarsen restated in plain Python / numpy - a loop for the plan, a dict for the lookup, a sort and np.add.reduceat for
the sums: what `coarsen.plan` and the device path must compute, column for column and byte for byte.  The reference has no script
for this step; the semantics are those of the module's docstring and of include/fithic_mi355x.h (FHX_CZ_*).
test_coarsen_model.py pins this model to hand-written expectations.  Not a test."""
import numpy as np

(OK, LOCUS, COUNT, SUM, INTERNAL) = range(5)
INT32_MAX = (1 << 31) - 1


class Refused(Exception):
    def __init__(self, why, row=0):
        super().__init__("reason %d at row %d" % (why, row))
        self.why, self.row = why, row


def plan(frag_chr, frag_mid, frag_hits, factor, resolution):
    """-> (coarse [(chr, mid, hits)], group_of [fine row -> coarse row]); ValueError as coarsen.plan raises it"""
    if factor < 1 or resolution < 0 or factor * resolution > INT32_MAX:
        raise ValueError("factor or resolution")
    chrom_order, rows_of = [], {}
    for row, (c, m) in enumerate(zip(frag_chr, frag_mid)):
        if int(c) not in rows_of:
            chrom_order.append(int(c))
            rows_of[int(c)] = []
        rows_of[int(c)].append((int(m), row))
    for c in chrom_order:
        loci = sorted(rows_of[c])
        for (m1, r1), (m2, r2) in zip(loci, loci[1:]):
            if m1 == m2:
                raise ValueError("twice: rows %d and %d" % (r1, r2))
    for row, m in enumerate(frag_mid):
        if resolution > 0 and (int(m) - resolution // 2) % resolution != 0:
            raise ValueError("not on the grid: row %d" % row)
    coarse, group_of = [], [None] * len(frag_mid)
    for c in chrom_order:
        last_key = None
        for k, (m, row) in enumerate(sorted(rows_of[c])):
            if resolution > 0:
                big = factor * resolution
                key = (m - resolution // 2) // big * big + big // 2
            else:
                key = k // factor
            if key != last_key:
                coarse.append([c, key, 0])
                last_key = key
            if resolution == 0:
                coarse[-1][1] = m                                     # the group's last member names it
            coarse[-1][2] += int(frag_hits[row])
            group_of[row] = len(coarse) - 1
    if any(h > INT32_MAX for _, _, h in coarse) or any(m > INT32_MAX for _, m, _ in coarse):
        raise ValueError("above 2^31 - 1")
    return [tuple(t) for t in coarse], group_of


def cells(frag_chr, frag_mid, coarse, group_of, rows, diagonal=True):
    """rows: five columns -> ([(chr1, mid1, chr2, mid2, sum)] in ascending (g1, g2), counts); Refused for the first bad row"""
    row_of = {(int(c), int(m)): k for k, (c, m) in enumerate(zip(frag_chr, frag_mid))}
    keys, values, dropped = [], [], 0
    for r, (c1, m1, c2, m2, n) in enumerate(zip(*[np.asarray(v).tolist() for v in rows])):
        if (c1, m1) not in row_of or (c2, m2) not in row_of:
            raise Refused(LOCUS, r)
        if n < 0:
            raise Refused(COUNT, r)
        g1, g2 = group_of[row_of[(c1, m1)]], group_of[row_of[(c2, m2)]]
        if g1 > g2:
            g1, g2 = g2, g1
        if g1 == g2 and not diagonal:
            dropped += 1
            continue
        keys.append((g1 << 32) | g2)
        values.append(n)
    counts = dict(rows=len(rows[0]), diagonal=dropped, cells=0)
    if not keys:
        return [], counts
    keys, values = np.array(keys, np.uint64), np.array(values, np.int64)
    order = np.argsort(keys, kind="stable")
    keys, values = keys[order], values[order]
    heads = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    sums = np.add.reduceat(values, heads)
    out = []
    for key, total in zip(keys[heads].tolist(), sums.tolist()):
        g1, g2 = key >> 32, key & 0xffffffff
        if total > INT32_MAX:
            raise Refused(SUM, key)
        out.append((coarse[g1][0], coarse[g1][1], coarse[g2][0], coarse[g2][1], total))
    counts["cells"] = len(out)
    return out, counts


def coarsen(fragments, rows, factor, resolution, diagonal=True):
    """the fine table (chr, mid, hits) and five columns -> (coarse table, cells, counts)"""
    coarse, group_of = plan(*fragments, factor, resolution)
    got, counts = cells(fragments[0], fragments[1], coarse, group_of, rows, diagonal)
    return coarse, got, counts


def contacts_text(names, cells_):
    """the decompressed bytes of the written contacts file"""
    return "".join("%s\t%d\t%s\t%d\t%d\n" % (names[c1], m1, names[c2], m2, n) for c1, m1, c2, m2, n in cells_).encode()


def fragments_text(names, coarse, coarse_resolution):
    """the decompressed bytes of the written fragments file; coarse_resolution = N * R, 0 for meta-fragments"""
    return "".join("%s\t%d\t%d\t%d\t%d\n" % (names[c], m - coarse_resolution // 2 if coarse_resolution else 0, m, h, 1 if h > 0 else 0)
                   for c, m, h in coarse).encode()
