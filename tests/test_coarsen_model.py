"""tests/coarsen_model.py and fithic_amd.coarsen.plan (host code, no GPU) held to expectations written out by hand: the groups of
chromosomes of 1, 9, 10, 11 and 21 loci, N = 1 and an N above every chromosome, the grid with gaps and a short last bin, odd and even
R', the refusals by name, a table given out of order, hits' at the int32 edge, and fragments.bins at R against fragments.bins at N*R;
then the model's cells on twelve rows written by hand."""
import numpy as np
import pytest

import coarsen_model as cm
from fithic_amd import coarsen, fragments, tables

INT32_MAX = (1 << 31) - 1


def both(c, m, h, factor, resolution):
    """the plan of the model and of coarsen.plan, after checking that they agree -> (coarse [(chr, mid, hits)], group_of)"""
    coarse, group_of = cm.plan(c, m, h, factor, resolution)
    p = coarsen.plan(c, m, h, factor, resolution)
    assert p.resolution == factor * resolution and len(p) == len(coarse)
    assert all(v.dtype == np.int32 for v in (p.chr, p.mid, p.hits, p.group_of))
    assert list(zip(p.chr.tolist(), p.mid.tolist(), p.hits.tolist())) == coarse and p.group_of.tolist() == group_of
    return coarse, group_of


def refused_by_both(c, m, h, factor, resolution, match):
    with pytest.raises(ValueError):
        cm.plan(c, m, h, factor, resolution)
    with pytest.raises(ValueError, match=match):
        coarsen.plan(c, m, h, factor, resolution)


def fragment_table(sizes):
    """chromosome c has sizes[c] loci at mid 100 * (k + 1) + 7 * c with hits k + 1, k = 0, 1, ..."""
    c = [ch for ch, n in enumerate(sizes) for _ in range(n)]
    m = [100 * (k + 1) + 7 * ch for ch, n in enumerate(sizes) for k in range(n)]
    h = [k + 1 for n in sizes for k in range(n)]
    return c, m, h


# ---- the plan: meta-fragments ---------------------------------------------------------------------------------------------
def test_chromosomes_of_1_9_and_10_loci_in_tens():
    coarse, group_of = both(*fragment_table([1, 9, 10]), 10, 0)
    assert coarse == [(0, 100, 1), (1, 907, 45), (2, 1014, 55)]
    assert group_of == [0] + [1] * 9 + [2] * 10


def test_chromosomes_of_11_21_and_1_loci_in_tens_end_in_a_short_group():
    coarse, group_of = both(*fragment_table([11, 21, 1]), 10, 0)
    assert coarse == [(0, 1000, 55), (0, 1100, 11), (1, 1007, 55), (1, 2007, 155), (1, 2107, 21), (2, 114, 1)]
    assert group_of == [0] * 10 + [1] + [2] * 10 + [3] * 10 + [4] + [5]


def test_factor_1_gives_the_fine_table_back():
    c, m, h = fragment_table([3, 1, 2])
    for resolution, mids in ((0, m), (10, [10 * v + 5 for v in m])):
        coarse, group_of = both(c, mids, h, 1, resolution)
        assert coarse == list(zip(c, mids, h)) and group_of == list(range(6))


def test_a_factor_above_every_chromosome_gives_one_locus_each():
    coarse, group_of = both(*fragment_table([3, 1, 2]), 64, 0)
    assert coarse == [(0, 300, 6), (1, 107, 1), (2, 214, 3)] and group_of == [0, 0, 0, 1, 2, 2]


# ---- the plan: the grid -----------------------------------------------------------------------------------------------------
def test_ten_bins_in_fours_and_a_chromosome_with_a_gap():
    c = [0] * 10 + [1] * 3 + [2]
    m = [10 * k + 5 for k in range(10)] + [5, 15, 125] + [45]
    h = list(range(1, 11)) + [7, 0, 2] + [0]
    coarse, group_of = both(c, m, h, 4, 10)                          # R' = 40, even: mids 20, 60, 100, ...
    assert coarse == [(0, 20, 10), (0, 60, 26), (0, 100, 19), (1, 20, 7), (1, 140, 2), (2, 60, 0)]
    assert group_of == [0] * 4 + [1] * 4 + [2] * 2 + [3, 3, 4] + [5]


def test_an_odd_coarse_resolution():
    coarse, group_of = both([4] * 5, [2, 7, 12, 17, 22], [1] * 5, 3, 5)      # R' = 15: bins [0, 15) and [15, 30), mids 7 and 22
    assert coarse == [(4, 7, 3), (4, 22, 2)] and group_of == [0, 0, 0, 1, 1]


def test_an_off_grid_mid_is_refused_by_name():
    c, m, h = [0, 0, 1, 1], [5, 15, 16, 25], [1, 1, 1, 1]
    refused_by_both(c, m, h, 2, 10, r"chromosome id 1, mid 16\), row 2 .*resolution 0")
    both(c, m, h, 2, 0)                                              # the same table is taken as meta-fragments
    refused_by_both([0], [10], [1], 2, 10, "mid 10")                 # a bin start is no midpoint


def test_a_locus_given_twice_is_refused_with_both_rows():
    refused_by_both([0, 1, 0, 1, 0], [5, 15, 15, 15, 25], [1] * 5, 2, 10, r"chromosome id 1, mid 15\) is given twice: rows 1 and 3")
    refused_by_both([0, 0], [7, 7], [1, 1], 3, 0, "rows 0 and 1")
    both([0, 1], [15, 15], [1, 1], 2, 10)                            # the same mid on two chromosomes is two loci


def test_a_table_given_out_of_order():
    c = [2, 0, 2, 1, 0, 2, 0]
    m = [25, 35, 5, 15, 5, 15, 15]
    h = [1, 2, 3, 4, 5, 6, 7]
    coarse, group_of = both(c, m, h, 2, 10)                          # chromosomes 2, 0, 1 as they first appear; mids ascending
    assert coarse == [(2, 10, 9), (2, 30, 1), (0, 10, 12), (0, 30, 2), (1, 10, 4)]
    assert group_of == [1, 3, 0, 4, 2, 0, 2]
    coarse, group_of = both(c, m, h, 2, 0)                           # ranks run over the ascending mids: (5, 15), (25) / (5, 15), (35)
    assert coarse == [(2, 15, 9), (2, 25, 1), (0, 15, 12), (0, 35, 2), (1, 15, 4)]
    assert group_of == [1, 3, 0, 4, 2, 0, 2]


def test_hits_up_to_int32_and_not_beyond():
    coarse, _ = both([0, 0, 0], [5, 15, 25], [INT32_MAX - 5, 5, 1], 2, 10)
    assert coarse == [(0, 10, INT32_MAX), (0, 30, 1)]
    refused_by_both([0, 0, 0], [5, 15, 25], [INT32_MAX - 5, 6, 1], 2, 10, r"sum to 2147483648")
    refused_by_both([0, 0], [5, 15], [1, 1], 0, 10, "factor")
    refused_by_both([0, 0], [5, 15], [1, 1], 3, 1 << 30, r"above 2\^31 - 1")


@pytest.mark.parametrize("resolution,factor", [(10, 4), (5, 3), (2, 7)])
def test_bins_at_r_planned_to_n_r_are_the_bins_at_n_r(resolution, factor, tmp_path):
    big = resolution * factor
    sizes = str(tmp_path / "sizes")
    with open(sizes, "w") as f:                                       # a multiple of R', of R only, of neither, and shorter than one bin
        f.write("chrA\t%d\nchrB\t%d\nchrC\t%d\nchrD\t%d\n" % (3 * big, 3 * big + resolution, 2 * big + resolution + 1, 1))
    p = coarsen.plan(*fragments.bins(sizes, resolution, tables.ChromIndex()), factor, resolution)
    want_chr, want_mid, _ = fragments.bins(sizes, big, tables.ChromIndex())
    assert np.array_equal(p.chr, want_chr) and np.array_equal(p.mid, want_mid) and len(p) == 3 + 4 + 3 + 1
    assert p.hits.sum() == len(p.group_of) and p.hits.max() == factor


# ---- the rows: twelve of them, on loci 0 = (0, 10), 1 = (0, 30), 2 = (1, 10) ---------------------------------------------------------
FINE = ([0, 0, 0, 0, 1, 1], [5, 15, 25, 35, 5, 15], [1] * 6)
ROWS = [(0, 5, 0, 25, 3),      # 0 x 1
        (0, 35, 0, 15, 4),     # 1 x 0: the other orientation of the same cell
        (0, 5, 1, 5, 2),       # 0 x 2, trans
        (1, 15, 0, 15, 5),     # 2 x 0
        (0, 5, 0, 15, 6),      # 0 x 0: two fine loci of one coarse locus
        (0, 15, 0, 15, 1),     # 0 x 0: a fine diagonal
        (0, 25, 1, 5, 0),      # 1 x 2 with a count of zero ...
        (1, 15, 0, 35, 0),     # ... twice: a cell whose sum is zero
        (1, 5, 1, 15, 9),      # 2 x 2
        (0, 25, 0, 35, 0),     # 1 x 1, a zero-count row in a cell that has more
        (0, 35, 0, 25, 8),     # 1 x 1
        (0, 15, 0, 35, 1)]     # 0 x 1
COLUMNS = [list(v) for v in zip(*ROWS)]


def test_twelve_rows_with_the_diagonal_kept():
    coarse, got, counts = cm.coarsen(FINE, COLUMNS, 2, 10)
    assert coarse == [(0, 10, 2), (0, 30, 2), (1, 10, 2)]
    assert got == [(0, 10, 0, 10, 7), (0, 10, 0, 30, 8), (0, 10, 1, 10, 7), (0, 30, 0, 30, 8), (0, 30, 1, 10, 0), (1, 10, 1, 10, 9)]
    assert counts == dict(rows=12, diagonal=0, cells=6)
    names = ["chrX", "chr2"]
    assert cm.contacts_text(names, got[1:3]) == b"chrX\t10\tchrX\t30\t8\nchrX\t10\tchr2\t10\t7\n"
    assert cm.fragments_text(names, coarse, 20) == b"chrX\t0\t10\t2\t1\nchrX\t20\t30\t2\t1\nchr2\t0\t10\t2\t1\n"
    assert cm.fragments_text(names, [(1, 777, 0)], 0) == b"chr2\t0\t777\t0\t0\n"


def test_twelve_rows_with_the_diagonal_dropped():
    _, got, counts = cm.coarsen(FINE, COLUMNS, 2, 10, diagonal=False)
    assert got == [(0, 10, 0, 30, 8), (0, 10, 1, 10, 7), (0, 30, 1, 10, 0)]
    assert counts == dict(rows=12, diagonal=5, cells=3)
    _, got, counts = cm.coarsen(FINE, COLUMNS, 64, 0, diagonal=False)          # one locus per chromosome: only the trans cell is left
    assert got == [(0, 35, 1, 15, 7)] and counts == dict(rows=12, diagonal=8, cells=1)


def test_the_model_refuses_the_first_bad_row():
    def why_row(rows, **kw):
        with pytest.raises(cm.Refused) as e:
            cm.coarsen(FINE, [list(v) for v in zip(*rows)], 2, 10, **kw)
        return e.value.why, e.value.row
    assert why_row(ROWS[:7] + [(0, 5, 0, 45, 1)] + ROWS[7:]) == (cm.LOCUS, 7)
    assert why_row(ROWS[:3] + [(2, 5, 0, 5, 1)]) == (cm.LOCUS, 3)             # a chromosome the table does not have
    assert why_row(ROWS + [(0, 5, 0, 5, -1), (0, 6, 0, 5, 1)]) == (cm.COUNT, 12)
    assert why_row(ROWS + [(0, 6, 0, 5, -1)]) == (cm.LOCUS, 12)               # on one row the locus is looked at first
    assert why_row([(0, 5, 0, 5, -1)], diagonal=False) == (cm.COUNT, 0)       # ... and the count before the diagonal
    big = [(0, 5, 0, 25, INT32_MAX - 1), (0, 35, 0, 15, 1)]
    assert cm.coarsen(FINE, [list(v) for v in zip(*big)], 2, 10)[1] == [(0, 10, 0, 30, INT32_MAX)]
    assert why_row(big + [(0, 15, 0, 25, 1)]) == (cm.SUM, 1)                  # the cell 0 x 1, as g1 << 32 | g2
