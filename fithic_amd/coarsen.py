"""Contact counts summed onto N-fold coarser loci: a fixed-size map at R taken to N*R, or the single restriction fragments of a
digest taken to meta-fragments of N consecutive ones (the reference's own `combineFrags10` test data are such), without another
pass over the read pairs.  The reference ships no script for this step; the semantics below are this project's own.

    python -m fithic_amd.coarsen -i CONTACTS.gz -f FRAGMENTS.gz -r R -n N -o OUTDIR [-l LIB] [--no-diagonal] [--device D]

writes OUTDIR/LIB_x<N>.contactCounts.gz and OUTDIR/LIB_x<N>.fragments.gz and prints the new resolution, or `meta-fragments of N`
with -r 0.  `read()` takes the rows of a contacts file, five host columns or - HBM to HBM - of a resident producer
(`validpairs.read`, `fragpairs.read`, `juicer.read`, `hicpro.read`) and keeps the cells in HBM for an Engine.

The plan (`plan()`, host, numpy, O(loci)).  The fine table is (chr id, mid, hits) as `tables.read_fragments` returns it.
Chromosomes keep their order of first appearance, inside a chromosome the loci are taken in ascending mid; the same (chr, mid)
twice is a ValueError that names both rows.
  R > 0, grid mode: every mid must satisfy (mid - R//2) % R == 0 - an off-grid locus is a ValueError that names it; such loci are
    grouped with R = 0.  With s = mid - R//2 and R' = N*R the coarse locus is (chr, (s // R') * R' + R'//2).  Only coarse bins that
    hold a fine locus exist.  R' must stay <= 2^31 - 1.
  R = 0, meta-fragment mode: ranks k = 0, 1, ... run inside the chromosome, the group is k // N, the last group of a chromosome may
    be shorter.  The coarse locus carries the column-3 value of the group's last member: with a digest's table, whose column 3 is
    the fragment's end, the meta-fragment's end - every coarse locus is again a line of a fragments file.
hits' is the sum of the members' hits; above 2^31 - 1 is a ValueError.  A coarse row is the position in the coarse table.

The rows (device, csrc/fhx_coarsen.hip).  Each end is looked up in the fine table; the two coarse rows are ordered g1 <= g2; a
row with g1 == g2 is a diagonal cell, kept by default and dropped with diagonal=False (as `fragpairs` drops same-fragment pairs).
The counts of the rows with equal (g1, g2) are summed; a cell exists when any row maps to it, a sum of zero included.  The cells
come out ascending in (g1, g2).  Refused with a ValueError that names the smallest such 0-based row and its five values, and
nothing stays loaded: an end that is no locus of the table, a negative count.  A cell whose sum is above 2^31 - 1 is refused and
named too.

`write()` writes `chr1 \\t mid1 \\t chr2 \\t mid2 \\t count` with the count plain, through the library's contacts writer
(`fragpairs` writes with it; the `%7d` padding of `validpairs.write` is the fixed-size script's `uniq -c` and belongs to that
script's bytes alone).  `write_fragments()` writes `chr \\t col2 \\t mid \\t hits' \\t mappable`: col2 is mid - R'//2 in grid mode and
0 in meta-fragment mode, as the reference's combineFrags lists have it; mappable is 1 if hits' > 0 else 0 (HiCPro2FitHiC.py:50-53).

Not done: no bias is made - biases are per locus and do not sum; `fithic --kr` and `hickry` work on the new rows.  There is no
`fithic` flag for this step and no sharded (--gpus N) form.  There is no CPU implementation here: without the library or a GPU
`read` raises.
"""
import argparse
import gzip
import os
import sys

import numpy as np

from . import _capi, tables
from ._resident import Resident

_INT32_MAX = (1 << 31) - 1
_REASONS = {_capi.CZ_LOCUS: "an end that is no locus of the fragments table", _capi.CZ_COUNT: "a negative count"}


class Plan:
    """The coarse table `chr`, `mid`, `hits` (int32), `group_of` (int32: fine row, in the order given -> coarse row) and
    `resolution` (N*R, or 0 in meta-fragment mode)."""

    def __init__(self, chr_, mid, hits, group_of, resolution, fine_chr, fine_mid):
        self.chr, self.mid, self.hits, self.group_of, self.resolution = chr_, mid, hits, group_of, resolution
        self._fine_chr, self._fine_mid = fine_chr, fine_mid

    def __len__(self):
        return len(self.mid)

    def device_tables(self):
        """(first, fine mids, group_of) laid out by chromosome id, the mids ascending within one: what fhx_cz_load_plan takes"""
        order = np.lexsort((self._fine_mid, self._fine_chr))
        n_chr = int(self._fine_chr.max()) + 1
        first = np.searchsorted(self._fine_chr[order], np.arange(n_chr + 1)).astype(np.int64)
        return first, self._fine_mid[order].astype(np.int32), self.group_of[order]


def plan(frag_chr, frag_mid, frag_hits, factor, resolution):
    """(chr ids, mids, hits) of the fine table, N, R -> the Plan (module docstring).  Pure host code."""
    factor, resolution = int(factor), int(resolution)
    if factor < 1:
        raise ValueError("factor %d: at least 1 is expected" % factor)
    if resolution < 0:
        raise ValueError("resolution %d: 0 (meta-fragments) or a bin size is expected" % resolution)
    coarse_res = factor * resolution
    if coarse_res > _INT32_MAX:
        raise ValueError("factor %d x resolution %d is above 2^31 - 1" % (factor, resolution))
    c, m, h = (np.asarray(v, np.int64).ravel() for v in (frag_chr, frag_mid, frag_hits))
    if not (len(c) == len(m) == len(h)):
        raise ValueError("the three columns of the fragments table differ in length")
    if len(c) and c.min() < 0:
        raise ValueError("a negative chromosome id in the fragments table")
    uniq, first_row, inverse = np.unique(c, return_index=True, return_inverse=True)
    rank = np.empty(len(uniq), np.int64)
    rank[np.argsort(first_row, kind="stable")] = np.arange(len(uniq))            # order of first appearance
    order = np.lexsort((m, rank[inverse]))
    cs, ms, hs = c[order], m[order], h[order]
    new_chr = np.r_[True, cs[1:] != cs[:-1]] if len(cs) else np.zeros(0, bool)
    twice = np.flatnonzero(~new_chr & (ms == np.r_[ms[:1], ms[:-1]]))
    if len(twice):
        k = int(twice[0])
        raise ValueError("the locus (chromosome id %d, mid %d) is given twice: rows %d and %d of the fragments table"
                         % (cs[k], ms[k], *sorted((int(order[k - 1]), int(order[k])))))
    if resolution > 0:
        start = ms - resolution // 2
        off = np.flatnonzero(start % resolution != 0)
        if len(off):
            k = int(order[off].min())
            raise ValueError("the locus (chromosome id %d, mid %d), row %d of the fragments table, is not on the grid of resolution %d: "
                             "off-grid loci are grouped with resolution 0" % (c[k], m[k], k, resolution))
        coarse_mid = start // coarse_res * coarse_res + coarse_res // 2
        if len(coarse_mid) and coarse_mid.max() > _INT32_MAX:
            raise ValueError("a coarse midpoint is above 2^31 - 1")
        head = new_chr | (coarse_mid != np.r_[coarse_mid[:1], coarse_mid[:-1]])
    else:
        chr_start = np.flatnonzero(new_chr)
        k_in_chr = np.arange(len(cs)) - np.repeat(chr_start, np.diff(np.r_[chr_start, len(cs)]))
        head = k_in_chr % factor == 0
    heads = np.flatnonzero(head)
    group_sorted = np.cumsum(head) - 1
    if resolution > 0:
        out_mid = coarse_mid[heads]
    else:
        out_mid = ms[np.r_[heads[1:], len(ms)] - 1] if len(heads) else ms[:0]     # the group's last member
    hits = np.add.reduceat(hs, heads) if len(heads) else hs[:0]
    if len(hits) and hits.max() > _INT32_MAX:
        g = int(np.argmax(hits > _INT32_MAX))
        raise ValueError("the hits of the coarse locus (chromosome id %d, mid %d) sum to %d: above 2^31 - 1" % (cs[heads[g]], out_mid[g], hits[g]))
    group_of = np.empty(len(c), np.int32)
    group_of[order] = group_sorted
    return Plan(cs[heads].astype(np.int32), out_mid.astype(np.int32), hits.astype(np.int32), group_of, coarse_res, c, m)


def _handle_of(source):
    """the native handle that holds a resident producer's rows: the object itself, or the context it keeps (as their own load_into
    reach it)"""
    if hasattr(source, "device_ptrs") and hasattr(source, "stream"):
        return source
    if isinstance(source, Resident) and not isinstance(source, Coarsened) and source._handle is not None:
        return source._handle
    raise TypeError("%r: a contacts file, five columns or a resident producer (validpairs, fragpairs, juicer, hicpro) is expected" % (source,))


def _names_of(source):
    return list(source.names if hasattr(source, "names") else source.chroms.names)


def _locus(names, chr_id, mid):
    return "%s:%d" % (names[chr_id] if 0 <= chr_id < len(names) else "chromosome id %d" % chr_id, mid)


class Coarsened(Resident):
    """The coarse cells (chr1, mid1, chr2, mid2, count) resident in HBM in ascending (coarse row 1, coarse row 2), and the coarse
    fragments table on the host.  The chr columns index `names`; `resolution` is N*R, or 0 for meta-fragments.  counts(): rows
    (given), diagonal (dropped), cells.  load_into: the coarse fragments and the cells into a configured Engine."""

    def __init__(self, cz, n_cells, names, plan_):
        super().__init__(cz, n_cells, names)
        self.n_cells, self.plan, self.resolution = n_cells, plan_, plan_.resolution

    def fragments(self):
        """(chr ids, mids, hits) of the coarse table, as tables.read_fragments returns them for the written file"""
        return self.plan.chr.copy(), self.plan.mid.copy(), self.plan.hits.copy()

    def write(self, path):
        _capi.host_write_contacts(path, self.names, *self.contacts())

    def fragments_text(self):
        half = self.resolution // 2
        return "".join("%s\t%d\t%d\t%d\t%d\n" % (self.names[c], m - half if self.resolution else 0, m, h, 1 if h > 0 else 0)
                       for c, m, h in zip(self.plan.chr.tolist(), self.plan.mid.tolist(), self.plan.hits.tolist()))

    def write_fragments(self, path):
        with gzip.open(path, "wt") as f:
            f.write(self.fragments_text())

    def _load_tables(self, engine, chroms):
        engine.load_fragments(*self.fragments(), chroms.sort_rank())


def _refusal(e, names, plan_, row_of):
    """the exception refused rows are reported with (module docstring); row_of(r) -> the five values of row r"""
    if e.why == _capi.CZ_SUM:
        g1, g2 = e.row >> 32, e.row & 0xffffffff
        return ValueError("the counts of the cell %s x %s sum to more than 2^31 - 1; the count column is int32"
                          % (_locus(names, int(plan_.chr[g1]), int(plan_.mid[g1])), _locus(names, int(plan_.chr[g2]), int(plan_.mid[g2]))))
    if e.why not in _REASONS:
        return e
    c1, m1, c2, m2, n = row_of(e.row)
    return ValueError("row %d (%s %s count %d): %s" % (e.row, _locus(names, c1, m1), _locus(names, c2, m2), n, _REASONS[e.why]))


def read(source, fragments, factor, resolution, chroms=None, diagonal=True, device=0):
    """source: the path of a contacts file, five host columns (chr1, mid1, chr2, mid2, count) or a resident producer; fragments:
    the path of the fine fragments file or its (chr ids, mids, hits) -> a Coarsened whose cells stay on GPU `device`.  `chroms` is
    the run's ChromIndex: the names of files are interned into it, the ids of columns and triples index it (a producer's names
    must agree with it).  ValueError for a table `plan` refuses or rows the device refuses.  Raises without the library or a GPU:
    there is no CPU path."""
    chroms = tables.ChromIndex() if chroms is None else chroms
    cols = None
    if isinstance(source, (str, bytes, os.PathLike)):
        t = tables.read_contacts(os.fspath(source), chroms)
        cols = [t.chr1, t.mid1, t.chr2, t.mid2, t.count]
    elif isinstance(source, (tuple, list)):
        if len(source) != 5:
            raise ValueError("%d columns where chr1, mid1, chr2, mid2, count are expected" % len(source))
        cols = [np.asarray(v) for v in source]
    else:
        handle = _handle_of(source)
        for k, name in enumerate(_names_of(source)):
            if chroms.intern(name) != k:
                raise ValueError("chromosome %r has id %d in the given ChromIndex and %d in the producer" % (name, chroms.intern(name), k))
    if isinstance(fragments, (str, bytes, os.PathLike)):
        fragments = tables.read_fragments(os.fspath(fragments), chroms)
    p = plan(*fragments, factor, resolution)
    if not len(p):
        raise ValueError("no locus in the fragments table")
    names = list(chroms.names)
    if int(p.chr.max()) >= len(names):
        raise ValueError("chromosome id %d of the fragments table has no name in the ChromIndex (%d names)" % (p.chr.max(), len(names)))
    cz =_capi.CzContext(device)
    try:
        cz.load_plan(*p.device_tables(), p.chr, p.mid)
        try:
            if cols is not None:
                n = cz.coarsen_host(*cols, diagonal=diagonal)
            else:
                n = cz.coarsen_device(handle.device_ptrs() if len(source) else [0] * 5, len(source), handle.stream(), diagonal=diagonal)
        except _capi.CzRefused as e:
            def row_of(r):
                five = cols if cols is not None else source.contacts()
                return [int(v[r]) for v in five]
            raise _refusal(e, names, p, row_of) from None
        return Coarsened(cz, n, names, p)
    except BaseException:
        cz.close()
        raise


def parse_args(argv):
    parser = argparse.ArgumentParser(prog="python -m fithic_amd.coarsen",
                                     description="contact counts and fragments summed onto N-fold coarser loci")
    parser.add_argument("-i", "--contacts", metavar="CONTACTS.gz", required=True, help="the contact counts at the fine loci")
    parser.add_argument("-f", "--fragments", metavar="FRAGMENTS.gz", required=True, help="the fragments file of the fine loci")
    parser.add_argument("-r", "--resolution", type=int, required=True, help="the fine bin size; 0 groups consecutive fragments")
    parser.add_argument("-n", "--factor", type=int, required=True, help="how many fine loci make a coarse one")
    parser.add_argument("-o", "--outdir", metavar="OUTDIR", required=True)
    parser.add_argument("-l", "--lib", metavar="LIB", default="fithic", help="the prefix of the two file names (default fithic)")
    parser.add_argument("--no-diagonal", action="store_true", help="drop the cells whose two ends fall into one coarse locus")
    parser.add_argument("--device", type=int, default=0)
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else argv)
    stem = os.path.join(args.outdir, "%s_x%d" % (args.lib, args.factor))
    with read(args.contacts, args.fragments, args.factor, args.resolution, diagonal=not args.no_diagonal, device=args.device) as data:
        cols = data.contacts()                                       # everything is computed before anything is written
        text = data.fragments_text()
        _capi.host_write_contacts(stem + ".contactCounts.gz", data.names, *cols)
        with gzip.open(stem + ".fragments.gz", "wt") as f:
            f.write(text)
        counts = data.counts()
    print("The new resolution is %d" % data.resolution if data.resolution else "meta-fragments of %d" % args.factor)
    print("%d rows, %d dropped as diagonal, %d cells" % (counts["rows"], counts["diagonal"], counts["cells"]))


if __name__ == "__main__":
    main()
