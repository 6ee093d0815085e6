"""The pass's class kernels with their tabulated reciprocals and lean divisions (fhx_bdtrc.hpp: contfrac_lazy_impl<.., LEAN>,
pseries<.., LEAN>) against Context.bdtrc_array - one lane per row through bdtrc_count, whose statements keep hipcc's `/` and the
per-lane reciprocals - BIT FOR BIT, on rows chosen for the new paths, through the pass's own launches (debug_k2_rows):

  * counts whose j = count + 2 i leaves the continued fractions' table in mid-loop (J - 40 .. J + 4), in both converging classes;
  * tiles whose waves mix counts inside and beyond the table (every count from 31 up shares the sort's last bucket);
  * counts 2, 3 and 31 / 32, the last bucket's edge;
  * cf_bd rows of both orientations at one count in one tile (the two binomials: total 100 swaps from count 51 on, total
    645 040 870 never does), and a tile of one orientation only;
  * power-series rows that reach n == b (the swapped orientation at total 100: b = count), rows that end before the first term,
    rows whose a + n leaves the 1 / j table, priors on both sides of the lean window's edge (1e-150) and at 1e-300;
  * the count == 1 strip at priors 1e-300, 1e-12 and 0.00999;
  * both binomials, and both kernel sets: a total of 100 makes the pass launch the SMALL_N kernels, two large totals the others.

A valid power-series row cannot run more terms than the 1 / j table holds (b x <= 1 and x <= 0.95 with b >= 2 give x <= 0.5 and
at most ~55 terms; the table has 512 entries): the term index leaves the table only through a + n, which is covered.
The class counts must be those of debug_classify and of the numpy restatement."""
import numpy as np
import pytest

import k2_rows as kr

pytestmark = pytest.mark.gpu

BIG = 645040870.0
SMALL = 100.0


@pytest.fixture(scope="module")
def ctx():
    from fithic_amd import _capi
    c = _capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def table_len(ctx):
    """J of the continued fractions' table and of the power series' table, from the hook"""
    return ctx.debug_table_div(0, np.empty(0)).shape[0] + 1, ctx.debug_table_div(1, np.empty(0)).shape[0] + 1


def per_lane_p(c, r):
    out = np.empty(len(r), np.float64)
    for side, total in ((0, r.n_intra), (1, r.n_inter)):
        sel = r.is_inter == side
        if sel.any():
            out[sel] = c.bdtrc_array(total, r.count[sel], r.prior[sel])
    return out


def check(c, r, what):
    p, by_class, _, hist = c.debug_k2_rows(r.n_intra, r.n_inter, r.count, r.prior, r.is_inter)
    lane = per_lane_p(c, r)
    diff = np.flatnonzero(~((p.view(np.int64) == lane.view(np.int64)) | (np.isnan(p) & np.isnan(lane))))
    assert len(diff) == 0, (what, len(diff), [(int(r.count[i]), float(r.prior[i]), int(r.is_inter[i]), float(p[i]), float(lane[i])) for i in diff[:5]])
    assert by_class == kr.class_rows(r.outcomes()), what
    arith = np.empty(len(r), np.int32)
    for side, total in ((0, r.n_intra), (1, r.n_inter)):
        sel = r.is_inter == side
        if sel.any():
            arith[sel] = c.debug_classify(total, r.count[sel], r.prior[sel])[1]
    for key, cls in (("pseries", kr.PSERIES), ("cf_bcf", kr.CF_BCF), ("cf_bd", kr.CF_BD), ("cf_swapped", kr.CF_SWAPPED)):
        assert by_class[key] == int((arith == cls).sum()), (what, key)
    # the fused key histogram: the class kernels count every p in its own bin; only k2h_heavy moves counts to lower bins
    true = kr.top_bins(p)
    assert int(hist.sum()) == int(true.sum()) and (np.cumsum(hist) >= np.cumsum(true)).all(), what
    if by_class["cf_swapped"] == 0:
        assert np.array_equal(hist, true), what
    return p


def converging_rows(total, counts, per, rng):
    """(count, prior) in the direct orientation of a large total: cf_bcf below (count - 1) / (total - 1), cf_bd from there to count / (total + 1)"""
    c = np.repeat(np.asarray(counts, np.int32), 2 * per)
    edge, top = (c - 1.0) / (total - 1.0), c / (total + 1.0)
    u = rng.random(len(c))
    bcf = edge * (0.2 + 0.799 * u)
    bd = edge + (top - edge) * u
    prior = np.where(np.arange(len(c)) % 2 == 0, bcf, bd)
    return c, prior


def small_total_grid(rng, counts=range(2, 100), per=24):
    """(count, prior) over (0, 1) for the total of 100: every class, cf_bd in both orientations"""
    c = np.repeat(np.asarray(list(counts), np.int32), per)
    around = np.clip(c / SMALL + rng.normal(0.0, 0.02, len(c)), 1e-6, 1.0 - 1e-6)
    prior = np.where(rng.random(len(c)) < 0.5, around, rng.uniform(0.001, 0.999, len(c)))
    return c, prior


def swapped_bd_small(rng, counts, per):
    """(count, prior) of cf_bd in the swapped orientation at the total of 100: count / 101 < prior <= (count - 1) / 99, count >= 51"""
    c = np.repeat(np.asarray(list(counts), np.int32), per)
    lo, hi = c / (SMALL + 1.0), (c - 1.0) / (SMALL - 1.0)
    return c, lo + (hi - lo) * rng.uniform(0.02, 0.98, len(c))


def flag1(r):
    """the orientation of a row: incbet's xx > aa / (aa + bb)"""
    aa = r.count.astype(np.float64)
    bb = r.totals() - (aa - 1.0)
    return r.prior > aa / (aa + bb)


@pytest.mark.parametrize("n_inter", [BIG, SMALL], ids=["large_totals", "small_n_kernels"])
def test_counts_across_the_table_edge(ctx, table_len, n_inter):
    """a + 2 i crosses J in mid-loop; waves of the last bucket mix counts inside and beyond the table; the buckets' edges"""
    J = table_len[0]
    rng = np.random.default_rng(11)
    counts = list(range(J - 40, J + 5)) + [2, 3, 30, 31, 32, 33, 40, 200, 600, 1500, 5000]
    big = converging_rows(BIG, counts, 12, rng)
    other = converging_rows(BIG, counts, 12, rng) if n_inter == BIG else small_total_grid(rng)
    r = kr.two_sided(BIG, big, n_inter, other).shuffled(rng)
    out = r.outcomes()
    for cls, least in ((kr.CF_BCF, 3), (kr.CF_BD, 2)):             # count 2 below its cf_bd range is a power-series row
        sel = (out == cls) & (r.is_inter == 0)
        assert sel.sum() >= 600 and {least, 3, 31, 32, J - 40, J - 1, J, J + 4} <= set(r.count[sel].tolist()), cls
    check(ctx, r, ("edge", n_inter))


def test_bd_orientations_share_a_tile(ctx):
    """cf_bd at counts 52 .. 99: total 100 takes the swapped orientation (a = total - count + 1), the large total the direct one -
    same counts, same tile, both binomials; then the direct rows alone"""
    rng = np.random.default_rng(12)
    counts = range(52, 100)
    small = [np.concatenate(v) for v in zip(swapped_bd_small(rng, counts, 8), small_total_grid(rng, counts, 8))]
    r = kr.two_sided(SMALL, small, BIG, converging_rows(BIG, list(counts), 8, rng)).shuffled(rng)
    bd = r.outcomes() == kr.CF_BD
    f = flag1(r)
    assert (bd & f).sum() >= 100 and (bd & ~f).sum() >= 100
    both = set(r.count[bd & f].tolist()) & set(r.count[bd & ~f].tolist())
    assert len(both) >= 20                                     # the same count in both orientations
    assert bd.sum() <= 1024                                    # one tile of k2_queue_by_count
    check(ctx, r, "bd_mixed")
    one = r.take(np.flatnonzero(bd & ~f))
    check(ctx, kr.Rows(BIG, BIG, one.count, one.prior, np.zeros(len(one), np.uint8)), "bd_direct_only")


@pytest.mark.parametrize("n_inter", [1.0e6, SMALL], ids=["large_totals", "small_n_kernels"])
def test_power_series_rows(ctx, table_len, n_inter):
    J = table_len[1]
    rng = np.random.default_rng(13)
    # direct orientation at the large total: b x <= 1 needs prior <= 1 / total; a = count on both sides of the 1 / j table's end
    counts = [2, 3, 4, 7, 31, 200, J - 30, J - 12, J - 3, J - 2, J - 1, J, J + 1, 1000]
    pri = [1e-300, 1e-200, 1e-160, 9.9e-151, 1.0e-150, 1.1e-150, 1e-140, 1e-30, 1e-18, 1e-12, 1e-10, 5e-10, 1.2e-9, 1.5e-9]
    c_dir = np.repeat(np.array(counts, np.int32), len(pri))
    p_dir = np.tile(np.array(pri), len(counts))
    if n_inter == SMALL:
        # swapped orientation at total 100: a = 101 - count, b = count, x = 1 - prior <= 1 / count; the term n == b is reached
        c_sw = np.repeat(np.arange(2, 40, dtype=np.int32), 16)
        p_sw = 1.0 - rng.uniform(0.02, 1.0, len(c_sw)) / c_sw
        c_dr = np.repeat(np.arange(2, 100, dtype=np.int32), 6)           # direct at total 100: prior <= 1 / (101 - count)
        p_dr = rng.uniform(0.05, 1.0, len(c_dr)) / (101.0 - c_dr)
        other = (np.concatenate([c_sw, c_dr]), np.concatenate([p_sw, p_dr]))
    else:
        other = (c_dir, np.minimum(p_dir * 600.0, 9.9e-7))                # the second binomial: total 1e6
    r = kr.two_sided(BIG, (c_dir, p_dir), n_inter, other).shuffled(rng)
    ps = r.outcomes() == kr.PSERIES
    assert ps.sum() >= 300
    if n_inter == SMALL:
        assert (ps & flag1(r)).sum() >= 100 and (ps & ~flag1(r) & (r.is_inter == 1)).sum() >= 100
    check(ctx, r, ("pseries", n_inter))


def test_closed_form_strip(ctx):
    """count == 1 at priors 1e-300, 1e-12 and 0.00999 (Cephes' log1p / expm1), both binomials, among rows of the other classes"""
    rng = np.random.default_rng(14)
    pri = np.array([1e-300, 1e-12, 0.00999, 0.01, 0.5])
    ones = (np.ones(len(pri) * 40, np.int32), np.tile(pri, 40))
    r = kr.Rows.concat([kr.two_sided(BIG, ones, 1.0e6, ones), kr.mixed_rows(1500, 15, n_intra=BIG, n_inter=1.0e6)]).shuffled(rng)
    assert (r.outcomes() == kr.CLOSED_LOCAL).sum() >= 240
    check(ctx, r, "closed")
