"""TEST INFRASTRUCTURE - built inputs for the nearby-contact merging (fithic_amd.combine / csrc/fhx_cni.hip), no GPU needed.

Every shape is a list of rows (chromosome name, mid1, mid2, cc, p, q) aimed at one seam of the 21 kernels that random tables do
not reach: one long dependent pick chain, roots that merge only through the last cells in key order, all-tied rankings, rows
written (hi, lo), diagonal cells, equal coordinates under two names, the percentile's edges, q = 0.0, duplicates of a cell that
straddle the scan and sort tiles, -p above 100.  A Case carries the flags of one run and the closed-form result where there is
one; tests/test_cni_shapes_inputs.py holds oracle.combine_oracle to those closed forms (so the GPU test cannot pass vacuously)
and tests/test_gpu_combine_shapes.py holds the engine to the oracle's lines and to model() for the fields the text does not show.

Cells are named by k: mid = k * RES + RES / 2, which the reference turns into the float bin k + 1 (CombineNearbyInteraction.py:
301-309) and the engine into the numerator n = (k + 1) * RES on the lattice offset 0.
"""
import functools

RES = 1000
HEAD = "chr1\tfragmentMid1\tchr2\tfragmentMid2\tcontactCount\tp-value\tq-value\tbias1\tbias2\tExpCC\n"


def mid(k):
    return k * RES + RES // 2


def row(name, k1, k2, cc, q, p=None):
    return (name, mid(k1), mid(k2), int(cc), float(q / 8 if p is None else p), float(q))


def text_of(rows, header=True):
    """the significances file of these rows: ten columns like Fit-Hi-C's, repr() of the floats so that they read back exactly"""
    body = "".join("%s\t%d\t%s\t%d\t%d\t%r\t%r\t1.0\t1.0\t1.0\n" % (r[0], r[1], r[0], r[2], r[3], r[4], r[5]) for r in rows)
    return (HEAD if header else "") + body


class Case:
    """one run: rows, the flags as keywords of combine_lines / combine_records, and what is known in closed form
    (lines, picked = {(name, k_lo, k_hi)}, nodes, components, largest, min_pick_rounds, box_is_full, same_lines_as)"""

    def __init__(self, id, rows, kw, **expect):
        self.id, self.rows, self.kw, self.expect = id, rows, kw, expect

    def __repr__(self):
        return self.id


# ---- a plain model of everything but the pick: cells, components, their statistics ------------------------------------------
def model(rows, conn, res=RES):
    """-> ({(name, k_lo, k_hi): dict(first_row, cc, p, q, component_size, box, box_cells, sum_cc)}, summary dict).  box =
    (min k_lo, max k_lo, min k_hi, max k_hi); box_cells counts the cells of the same name inside the box (:392-398)."""
    cells = {}
    for i, (name, m1, m2, cc, p, q) in enumerate(rows):
        k1, k2 = (m1 - res // 2) // res, (m2 - res // 2) // res
        assert mid(k1) == m1 and mid(k2) == m2 and res == RES
        cells.setdefault((name, min(k1, k2), max(k1, k2)), dict(first_row=i, cc=cc, p=p, q=q))
    steps = [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a or b) and (conn == 8 or a == 0 or b == 0)]
    seen, sizes = set(), []
    for start in cells:
        if start in seen:
            continue
        comp, todo = [], [start]
        seen.add(start)
        while todo:
            c = todo.pop()
            comp.append(c)
            for a, b in steps:
                o = (c[0], c[1] + a, c[2] + b)
                if o in cells and o not in seen:
                    seen.add(o)
                    todo.append(o)
        box = (min(c[1] for c in comp), max(c[1] for c in comp), min(c[2] for c in comp), max(c[2] for c in comp))
        if (box[1] - box[0] + 1) * (box[3] - box[2] + 1) < len(cells):      # walk the smaller of the box and the table
            inside = sum(1 for a in range(box[0], box[1] + 1) for b in range(box[2], box[3] + 1) if (start[0], a, b) in cells)
        else:
            inside = sum(1 for c in cells if c[0] == start[0] and box[0] <= c[1] <= box[1] and box[2] <= c[2] <= box[3])
        total = sum(cells[c]["cc"] for c in comp)
        for c in comp:
            cells[c].update(component_size=len(comp), box=box, box_cells=inside, sum_cc=total)
        sizes.append(len(comp))
    return cells, dict(nodes=len(cells), components=len(sizes), largest=max(sizes) if sizes else 0)


def parse_line(line, res=RES):
    """one output line -> (cell, dict of the fields the text shows)"""
    w = line.split("\t")
    assert len(w) == 13 and w[0] == w[2]
    k1, k2 = (float(w[1]) - res / 2) / res, (float(w[3]) - res / 2) / res
    assert k1 == int(k1) and k2 == int(k2)
    box = (int(w[7]) // res, int(w[8]) // res - 1, int(w[9]) // res, int(w[10]) // res - 1)
    return (w[0], int(k1), int(k2)), dict(cc=int(w[4]), p=float(w[5]), q=float(w[6]), box=box, sum_cc=int(w[11]), strong=float(w[12]))


# ---- the shapes --------------------------------------------------------------------------------------------------------------
def chain_rows(n, name="chrA"):
    """cells (i, i+10): each touches the next only diagonally; q rises along the chain, so with -n 1 every pick waits for the one before"""
    return [row(name, i, i + 10, 5 + (i * 37) % 11, 1e-9 * (1 + i)) for i in range(n)]


def swap_odd(rows):
    return [(r[0], r[2], r[1]) + r[3:] if i % 2 else r for i, r in enumerate(rows)]


def comb_rows():
    rows = []
    for t in range(64):
        rows += [("chrA", 2 * t, 1000 + j) for j in range(64)]
    rows += [("chrA", lo, 1064) for lo in range(128)]                  # the spine: last in key order within every lo
    n = len(rows)
    assert n == 64 * 64 + 128
    return [row(name, a, b, 3 + j % 13, 1e-9 * (1 + (j * 1009) % n)) for j, (name, a, b) in enumerate(rows)]


def square_rows(side=64, name="chrA"):
    return [row(name, 100 + a, 300 + b, 9, 1e-6) for a in range(side) for b in range(side)]


DIAGONAL_CELLS = [(5, 5), (5, 6), (6, 6), (6, 5), (7, 7), (4, 6), (8, 7)]       # as written: (6, 5) repeats (5, 6), (8, 7) is (7, 8)


def diagonal_rows(name="chrA"):
    return [row(name, a, b, 20 + j, 1e-7 * (1 + j)) for j, (a, b) in enumerate(DIAGONAL_CELLS)]


NAMES_A = [(10, 20), (11, 20), (11, 21), (30, 40)]
NAMES_B = [(10, 20), (11, 20), (11, 21), (10, 21), (31, 40)]                    # (31, 40) touches A's (30, 40) across the names only


def two_name_rows(a="chrA", b="chrB"):
    rows = []
    for j in range(5):
        if j < len(NAMES_A):
            rows.append(row(a, NAMES_A[j][0], NAMES_A[j][1], 30 + j, 1e-7 * (2 + j)))
        rows.append(row(b, NAMES_B[j][0], NAMES_B[j][1], 40 + j, 1e-7 * (3 + j)))
    return rows


PCT_LENGTHS = (1, 2, 3, 10, 100, 101, 199, 200)
PCT_VALUES = (1, 49, 50, 99, 100)


def line_q(L, tied):
    """q along a straight line of L cells: a scramble of 1..L (37 is coprime to every L used); tied: runs of three equal values,
    so the percentile's bound is shared and the strict `q > bound` shows"""
    return [1e-6 * (1 + ((i * 37) % L) // (3 if tied else 1)) for i in range(L)]


def line_rows(qs, hi=500, name="chrA", cc0=10):
    return [row(name, 50 + i, hi, cc0 + i, q, p=q) for i, q in enumerate(qs)]


def percent_selected(qs, pct, order):
    """closed form for one component with -n 0 and q > 0: custom_percent (:36-52) picks sorted(q)[L*pct/100], or the maximum when
    that index is <= 1; ascending order keeps q <= bound; descending order compares -q with the positive bound and stops at once"""
    if pct == 100:
        return len(qs)
    if order == 1:
        return 0
    index = len(qs) * pct // 100
    bound = max(qs) if index <= 1 else sorted(qs)[index]
    return sum(1 for q in qs if q <= bound)


ZERO_ALL = [0.0] * 6
ZERO_MIXED = [0.0, 0.0, 0.0, 1e-5, 2e-5, 3e-5]
# cells 50+i with cc = 10+i and -n 2, worked by hand: ranking (q or -q, -cc); a pick drops what lies within two bins
ZERO_RUNS = [("s1", dict(order=1), {5, 2}, {5, 2}),
             ("s1_p50", dict(order=1, pct=50), {5, 2}, set()),      # mixed: bound 0.0, first key -3e-5 < 0.0 stops at once
             ("p50", dict(pct=50), {5, 2}, {2})]                    # mixed: bound 1e-5; picks 2, drops 1, 0 and 3; 4 is past it

DUP_CELLS = 5000


def dup_rows():
    """cell c at rows c, c + 5000, c + 10000 with other values each time; cells isolated, and scattered against the row order"""
    rows = []
    for m in range(3):
        for c in range(DUP_CELLS):
            pc = (c * 1237) % DUP_CELLS
            rows.append(row("chrA", 2 * (pc % 71), 200 + 2 * (pc // 71), 1 + c % 97 + 100 * m, 1e-8 * (1 + c) / (1 + m)))
    return rows


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    chain = chain_rows(4096)
    out.append(Case("chain_c8", chain, dict(conn=8, neigh=1), lines=2048, picked={("chrA", i, i + 10) for i in range(0, 4096, 2)},
                    nodes=4096, components=1, largest=4096, min_pick_rounds=65, box_is_full=True))
    out.append(Case("chain_c4", chain, dict(conn=4, neigh=1), lines=4096, picked={("chrA", i, i + 10) for i in range(4096)},
                    nodes=4096, components=4096, largest=1))
    comb = comb_rows()
    for conn in (8, 4):
        out.append(Case("comb_c%d" % conn, comb, dict(conn=conn), nodes=len(comb), components=1, largest=len(comb), box_is_full=True,
                        box=(0, 127, 1000, 1064)))
    square = square_rows()
    for neigh, want in ((0, 4096), (1, 1024), (2, 484), (3, 256), (63, 1), (64, 1)):
        step = neigh + 1
        picked = {("chrA", 100 + a, 300 + b) for a in range(0, 64, step) for b in range(0, 64, step)}
        assert len(picked) == want
        for order in (0, 1):
            out.append(Case("square_n%d_s%d" % (neigh, order), square, dict(neigh=neigh, order=order), lines=want, picked=picked,
                            nodes=4096, components=1, largest=4096, box_is_full=True))
    plain = chain_rows(200)
    even = {("chrA", i, i + 10) for i in range(0, 200, 2)}
    out.append(Case("orient_plain", plain, dict(neigh=1), lines=100, picked=even, nodes=200, components=1, largest=200))
    out.append(Case("orient_swapped", swap_odd(plain), dict(neigh=1), lines=100, picked=even, nodes=200, components=1, largest=200,
                    same_lines_as="orient_plain"))
    diag = diagonal_rows()
    out.append(Case("diagonal_c8", diag, dict(conn=8, neigh=1), lines=2, picked={("chrA", 5, 5), ("chrA", 7, 7)}, nodes=6, components=1,
                    largest=6))
    out.append(Case("diagonal_c4", diag, dict(conn=4, neigh=1), lines=2, picked={("chrA", 5, 5), ("chrA", 7, 7)}, nodes=6, components=2,
                    largest=4))
    out.append(Case("two_names", two_name_rows(), dict(neigh=0), lines=9, nodes=9, components=4, largest=4,
                    picked={("chrA",) + c for c in NAMES_A} | {("chrB",) + c for c in NAMES_B}))
    for L in PCT_LENGTHS:
        for tied in (False, True):
            qs = line_q(L, tied)
            assert tied or len(set(qs)) == L
            rows = line_rows(qs)
            for pct in PCT_VALUES:
                for order in (0, 1):
                    out.append(Case("pct_L%d_%s_p%d_s%d" % (L, "tied" if tied else "distinct", pct, order), rows,
                                    dict(pct=pct, order=order, neigh=0), lines=percent_selected(qs, pct, order), nodes=L, components=1,
                                    largest=L))
    for tag, qs, col in (("all", ZERO_ALL, 2), ("mixed", ZERO_MIXED, 3)):
        for run in ZERO_RUNS:
            picked = {("chrA", 50 + i, 500) for i in run[col]}
            out.append(Case("zero_%s_%s" % (tag, run[0]), line_rows(qs), run[1], lines=len(picked), picked=picked, nodes=6, components=1,
                            largest=6))
    dup = dup_rows()
    out.append(Case("duplicates", dup, dict(neigh=0), lines=DUP_CELLS, nodes=DUP_CELLS, components=DUP_CELLS, largest=1,
                    first_copy=True))
    for pct in (101, 1000):
        out.append(Case("above100_p%d" % pct, chain_rows(300), dict(pct=pct, neigh=1), lines=0, nodes=300, components=1, largest=300))
    assert len({c.id for c in out}) == len(out)
    return tuple(out)


def case(id):
    return next(c for c in cases() if c.id == id)


# ---- the lattice's edges, for CniContext.load directly (numerators n = bin * RES, offset 0) ----------------------------------
TOP = (1 << 24) - 1
EDGE_CHR = 65535
EDGE_CELLS = [(0, 0), (0, TOP), (TOP - 1, TOP), (TOP, TOP)]
# by hand: (0,0) and (0,TOP) stand alone; (TOP-1,TOP) and (TOP,TOP) touch.  box = (min lo, max lo, min hi, max hi) in bins
EDGE_EXPECT = {(0, 0): dict(component_size=1, box=(0, 0, 0, 0), box_cells=1, sum_cc=11, first_row=0),
               (0, TOP): dict(component_size=1, box=(0, 0, TOP, TOP), box_cells=1, sum_cc=12, first_row=1),
               (TOP - 1, TOP): dict(component_size=2, box=(TOP - 1, TOP, TOP, TOP), box_cells=2, sum_cc=13 + 14, first_row=2),
               (TOP, TOP): dict(component_size=2, box=(TOP - 1, TOP, TOP, TOP), box_cells=2, sum_cc=13 + 14, first_row=3)}


def make_key_is_all_ones():
    """cnd::make_key of the last edge cell: chr << 48 | lo << 24 | hi is the u64 with every bit set, the sort's dead-lane filler"""
    return (EDGE_CHR << 48 | TOP << 24 | TOP) == (1 << 64) - 1


def edge_columns():
    """(chr ids, n1, n2, cc, p, q) of EDGE_CELLS on chromosome id 65535: the last cell's key is all ones"""
    n1 = [a * RES for a, _ in EDGE_CELLS]
    n2 = [b * RES for _, b in EDGE_CELLS]
    q = [1e-5 * (1 + j) for j in range(len(EDGE_CELLS))]
    return [EDGE_CHR] * len(EDGE_CELLS), n1, n2, [11, 12, 13, 14], [v / 2 for v in q], q


# ---- the built golden input (tests/golden/make_golden.py f10 writes it and runs the real script on it) ----------------------
def golden_built_rows():
    """about 500 rows on three chromosomes: a 300-cell chain with every second row from 100 on written (hi, lo), a 12 x 12 square
    of ties, the diagonal set, the two-name set, six cells with q = 0.0 and six with zeros and positive q mixed"""
    chain = chain_rows(300, "chr2")
    rows = chain[:100] + swap_odd(chain[100:])
    rows += square_rows(12, "chr10") + diagonal_rows("chr10")
    rows += two_name_rows("chr10", "chrX")
    rows += line_rows(ZERO_ALL, 500, "chrX") + line_rows(ZERO_MIXED, 700, "chrX", cc0=40)
    return rows
