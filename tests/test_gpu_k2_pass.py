"""K2 as a pass runs it - k2_classify with its LDS table, the wave-local closed form, k2_closed, the class kernels, the count-sorted
300-iteration class with its hand-back - on chosen (count, prior, total) rows, through the fhx_debug_k2_rows hook (the launches of
fhx_pvalues on caller-supplied rows; tests/k2_rows.py builds the rows, tests/test_k2_pass_inputs.py checks that they reach every path).

Bars: NaN pattern identical and |p - reference| <= 1e-10 against scipy's values (f3_bdtrc.npz) and the oracle; counts stay <= 1e4,
so the last bit of libm's log times the count stays below 1e-11 (see test_gpu_fuzz.py).  Beside it the relative bar of
tests/p_relative.py against the oracle, row by row: 2 S + 4 ulp, S = what a libm one ulp off moves the oracle's own value.  And p must equal Context.bdtrc_array - one
lane per row through bdtrc_count -> incbet - BIT FOR BIT: the class kernels claim the same operations in the same order.

The last test is an Engine run: the third exit of the no-bias table path (k2_memo_overflow scanning for its -1.0 marks)."""
import os

import numpy as np
import pytest

import k2_rows as kr
from conftest import bits_equal, max_abs_diff
from p_relative import assert_p_faithful

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def ctx():
    from fithic_amd import _capi
    c = _capi.Context(0)          # raises if there is no GPU or the library is missing: no fallback
    yield c
    c.close()


@pytest.fixture(scope="module")
def wide():
    """totals kept as they are (FHX_TOTALS_WIDE): 7150761687 stays that number instead of scipy's narrowed, negative one"""
    from fithic_amd import _capi
    c = _capi.Context(0)
    c.set_params(10000, totals=_capi.TOTALS_WIDE)
    yield c
    c.close()


def oracle_p(r, totals="reference"):
    from oracle import fithic_oracle as fo
    return fo.bdtrc(r.count.astype(np.float64) - 1, r.totals(), r.prior, totals=totals)


def per_lane_p(c, r):
    """Context.bdtrc_array (k_bdtrc_array: bdtrc_count -> incbet, one lane per row) for the rows of both binomials"""
    out = np.empty(len(r), np.float64)
    for side, total in ((0, r.n_intra), (1, r.n_inter)):
        sel = r.is_inter == side
        if sel.any():
            out[sel] = c.bdtrc_array(total, r.count[sel], r.prior[sel])
    return out


def run_and_check(c, r, nonfixed=False, ref=None, totals="reference", what=""):
    """the hook on r: p bit-equal to the per-lane entry, within TOL of the oracle (and of `ref`), class counts as predicted"""
    p, by_class, n_redo, hist = c.debug_k2_rows(r.n_intra, r.n_inter, r.count, r.prior, r.is_inter, nonfixed=nonfixed)
    lane = per_lane_p(c, r)
    diff = np.flatnonzero(~((p.view(np.int64) == lane.view(np.int64)) | (np.isnan(p) & np.isnan(lane))))
    assert len(diff) == 0, (what, len(diff), [(int(r.count[i]), float(r.prior[i]), int(r.is_inter[i]), float(p[i]), float(lane[i])) for i in diff[:5]])
    assert max_abs_diff(p, oracle_p(r, totals)) <= TOL, what
    assert_p_faithful(p, r.count, r.totals(), r.prior, totals=totals, what=what)          # ... and within the relative bar, row by row
    if ref is not None:
        assert max_abs_diff(p, ref) <= TOL, what
    assert by_class == kr.class_rows(r.outcomes()), what
    return p, by_class, n_redo, hist


@pytest.mark.parametrize("nonfixed", [False, True])
def test_scipy_fixture_through_the_pass(ctx, nonfixed):
    """a. Every total of f3_bdtrc.npz once as the intra binomial and once as the inter one, the other binomial holding the next
    total's rows: a swap of P.intra / P.inter or of the two halves of tb_lds would show.  Both classification kernels."""
    fx = kr.fixture_rows()
    totals = sorted(fx)
    assert len(totals) >= 19 and sum(len(v[0]) for v in fx.values()) > 12900
    for j, nt in enumerate(totals):
        other = totals[(j + 1) % len(totals)]
        r = kr.two_sided(nt, fx[nt][:2], other, fx[other][:2])
        run_and_check(ctx, r, nonfixed, ref=np.concatenate([fx[nt][2], fx[other][2]]), what=(nt, other))


@pytest.mark.parametrize("n_intra,n_inter", kr.BOUNDARY_PAIRS)
def test_class_boundaries(wide, n_intra, n_inter):
    """b. Each of the five thresholds of each count (as the device computes them: debug_classify) with three doubles on both sides,
    the domain edges, 0.95 / 0.05, the closed-form switch at 0.01, NaN; counts on both sides of K2_TB_COUNTS and K2H_KCAP and
    around the total.  Classes must be the numpy restatement's, p must meet both bars."""
    thr = []
    for total in (n_intra, n_inter):
        counts = kr.boundary_counts(total)
        t = wide.debug_classify(total, counts, np.full(len(counts), 0.5), thresholds=True)[2]
        live = (counts >= 2) & (counts <= total)                       # elsewhere no prior reaches a threshold
        assert bits_equal(t[live], kr.thresholds(total, counts)[live]), total
        thr.append(t)
    r = kr.boundary_case(n_intra, n_inter, thr[0], thr[1])
    assert len(np.unique(r.outcomes())) >= (7 if max(n_intra, n_inter) > 1000 else 4)
    for nonfixed in (False, True):
        run_and_check(wide, r, nonfixed, totals="wide", what=(n_intra, n_inter, nonfixed))


def test_class_boundaries_narrowed_total(ctx):
    """b. in reference mode 7150761687 is narrowed to a negative C int as scipy does: every row of that binomial is NaN"""
    r = kr.boundary_case(1.0e6, 7150761687.0)
    p, _, _, _ = ctx.debug_k2_rows(r.n_intra, r.n_inter, r.count, r.prior, r.is_inter)
    assert bits_equal(np.isnan(p), np.isnan(oracle_p(r))) and max_abs_diff(p, oracle_p(r)) <= TOL
    assert np.isnan(p[(r.is_inter == 1) & (r.count >= 1)]).all()


def test_small_totals(ctx):
    """c. Totals 0..172 (the pow branch of Cephes below 171; 0: nothing but trivial rows) as the intra binomial beside a large
    inter one, the other way round, and on both sides: the SMALL_N kernels with T.small_n set for one table only."""
    seen = set()
    for j, (name, r) in enumerate(kr.small_total_cases()):
        _, by_class, _, _ = run_and_check(ctx, r, nonfixed=(j % 7 == 3), what=name)
        seen.add(kr.plan_small_n(r.n_intra, r.n_inter))
        if max(r.n_intra, r.n_inter) == 0:
            assert sum(by_class.values()) == 0
    assert seen == {False, True}
    zero = kr.two_sided(0.0, kr.small_total_rows(0, np.random.default_rng(1)), 0.0, kr.small_total_rows(0, np.random.default_rng(2)))
    _, by_class, _, _ = run_and_check(ctx, zero, what="both totals 0")
    assert sum(by_class.values()) == 0


def test_handback_and_generic_bucket(ctx, monkeypatch):
    """d. Rows of the swapped class that cf_swapped_regular rejects (count > (n + 1) / 2 under a high prior) come back through the
    redo list and k2h_generic; counts >= K2H_KCAP go through the generic bucket.  The number handed back is the predicted one, and
    p equals the per-lane kernel's (FHX_K2_LEGACY) bit for bit."""
    total_back = 0
    for name, r, want_back in kr.handback_cases():
        monkeypatch.delenv("FHX_K2_LEGACY", raising=False)
        p, by_class, n_redo, _ = run_and_check(ctx, r, what=name)
        print("%s: %d rows, %d in the swapped class, %d handed back (predicted %d)" % (name, len(r), by_class["cf_swapped"], n_redo, want_back))
        assert n_redo == want_back, name
        monkeypatch.setenv("FHX_K2_LEGACY", "1")
        legacy, _, legacy_redo, _ = ctx.debug_k2_rows(r.n_intra, r.n_inter, r.count, r.prior, r.is_inter)
        assert bits_equal(p, legacy) and legacy_redo == 0, name
        total_back += n_redo
    assert total_back > 200


def heavy_variants(ctx, monkeypatch, r, what):
    """the hook under the default heavy kernel (two rows per lane), FHX_K2H_ROWS=4 and FHX_K2_LEGACY=1: all checked, all bit-equal"""
    out = []
    for env in ({}, {"FHX_K2H_ROWS": "4"}, {"FHX_K2_LEGACY": "1"}):
        monkeypatch.delenv("FHX_K2H_ROWS", raising=False)
        monkeypatch.delenv("FHX_K2_LEGACY", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out.append(run_and_check(ctx, r, what=(what, env)))
    monkeypatch.delenv("FHX_K2_LEGACY", raising=False)
    assert bits_equal(out[0][0], out[1][0]) and bits_equal(out[0][0], out[2][0]), what
    return out


def check_hist(r, p, hist, exact):
    """f. the fused key histogram against the bins of the p the call returned"""
    true = kr.top_bins(p)
    assert int(hist.sum()) == int((~np.isnan(p)).sum()) == int(true.sum())
    assert (np.cumsum(hist) >= np.cumsum(true)).all()                  # add_wave_min moves counts to lower bins only
    if exact:
        assert np.array_equal(hist, true)


@pytest.mark.parametrize("m", kr.ROW_COUNTS)
def test_row_counts(ctx, monkeypatch, m):
    """e. + f. Shuffled rows of every class at row counts around the group of four, the wave, the tile and the shard"""
    r = kr.mixed_rows(m, 80 + m)
    for (p, by_class, n_redo, hist), legacy in zip(heavy_variants(ctx, monkeypatch, r, m), (False, False, True)):
        check_hist(r, p, hist, exact=legacy or by_class["cf_swapped"] == 0)
    p, _, _, hist = run_and_check(ctx, r, nonfixed=True, what=(m, "nonfixed"))
    check_hist(r, p, hist, exact=False)


@pytest.mark.parametrize("inter", [False, True])
@pytest.mark.parametrize("m", [127, 128, 129, 255, 256, 257])
def test_heavy_bucket_sizes(ctx, monkeypatch, m, inter):
    """e. + f. One (binomial, count) bucket of 64 R - 1, 64 R, 64 R + 1 rows for R = 2 and R = 4 - a task of k2h_heavy is 64 R
    entries and every bucket starts at a multiple of that - inside a mix of all classes"""
    r = kr.heavy_bucket_case(m, 40 + m, inter=inter)
    for (p, by_class, n_redo, hist), legacy in zip(heavy_variants(ctx, monkeypatch, r, (m, inter)), (False, False, True)):
        assert by_class["cf_swapped"] >= m
        check_hist(r, p, hist, exact=legacy)


@pytest.mark.parametrize("which", [kr.CF_BCF, kr.CF_BD])
@pytest.mark.parametrize("m", [1023, 1024, 1025])
def test_count_sorted_class_sizes(ctx, which, m):
    """e. a k2_queue_by_count class (tiles of at most 1024 entries) of exactly 1023, 1024 and 1025 entries"""
    r = kr.sorted_class_case(which, m, 60 + m)
    p, by_class, _, hist = run_and_check(ctx, r, what=(which, m))
    assert by_class[kr.CLASS_KEYS[which - 1]] == m
    check_hist(r, p, hist, exact=False)


def test_histogram_is_exact_without_the_heavy_kernel(ctx):
    """f. no row of the swapped class: every kernel counts each p in its own bin (p == 1.0 through the per-thread counter)"""
    r = kr.rows_of_outcome(kr.CF_SWAPPED, 3000, 7, without=True)
    p, by_class, _, hist = run_and_check(ctx, r, what="no swapped rows")
    assert by_class["cf_swapped"] == 0 and int((p == 1.0).sum()) > 20 and len(np.unique(r.outcomes())) == 6
    check_hist(r, p, hist, exact=True)


def test_hook_refuses_what_it_cannot_represent_and_leaves_no_stale_rows(ctx):
    from fithic_amd import _capi
    one = (np.array([2], np.int32), np.array([0.5]), np.array([0], np.uint8))
    for n_intra, n_inter, cnt, pri in ((100.0, 100.0, [2], [-0.5]), (100.0, 100.0, [-1], [0.5]), (100.0, 100.0, [2 ** 20 + 1], [0.5]),
                                       (-1.0, 100.0, [2], [0.5]), (100.0, float("inf"), [2], [0.5]), (float("nan"), 100.0, [2], [0.5])):
        with pytest.raises(_capi.FhxError):
            ctx.debug_k2_rows(n_intra, n_inter, np.array(cnt, np.int32), np.array(pri), one[2])
    p, _, _, _ = ctx.debug_k2_rows(100.0, 100.0, *one)
    assert p[0] == ctx.bdtrc_array(100.0, one[0], one[1])[0]
    p0, by_class, n_redo, hist = ctx.debug_k2_rows(100.0, 100.0, one[0][:0], one[1][:0], one[2][:0])
    assert len(p0) == 0 and sum(by_class.values()) == 0 and n_redo == 0 and hist.sum() == 0
    with pytest.raises(_capi.FhxError):          # the hook's rows are gone: a pass needs a fresh load
        ctx.pass_stats()


def _overflow_case(d, mode):
    """~20 000 fixed-size rows, no bias: two chromosomes of 400 loci, every pair up to 50 bins apart, counts decaying with the
    distance (hundreds to thousands at the short ones), and inter-chromosomal rows of which many hold counts of 5 000 to 9 000 -
    in interOnly mode the table has one column and reaches counts in the thousands"""
    import gzip
    rng = np.random.default_rng(31 if mode == "All" else 32)
    res, n_loci = 10000, 400
    mids = np.arange(n_loci) * res + res // 2
    frags, rows = [], []
    for ch in ("chr1", "chr2"):
        frags += ["%s\t0\t%d\t2\t1\n" % (ch, m) for m in mids]
    for i in range(n_loci):
        for dist in range(1, 51):
            if i + dist < n_loci and dist % 2 == i % 2:
                c = min(9000, 1 + int(rng.poisson(2000.0 / (1.0 + dist) ** 1.1 * rng.lognormal(0, 0.4))))
                rows.append("chr1\t%d\tchr1\t%d\t%d\n" % (mids[i], mids[i + dist], c))
    n_intra = len(rows)
    for _ in range(20000 - n_intra if mode == "All" else 1500):
        c = int(rng.integers(5000, 9000)) if mode == "interOnly" or rng.random() < 0.3 else 1 + int(rng.poisson(3.0))
        rows.append("chr1\t%d\tchr2\t%d\t%d\n" % (rng.choice(mids), rng.choice(mids), c))
    if mode == "All":
        rows = [rows[i] for i in rng.permutation(len(rows))]
    paths = dict(contacts=os.path.join(d, "c.gz"), frags=os.path.join(d, "f.gz"))
    for key, lines in (("contacts", rows), ("frags", frags)):
        with gzip.open(paths[key], "wt") as f:
            f.write("".join(lines))
    return paths, dict(resolution=res, n_bins=20, mode=mode, L=1 * res, U=48 * res)


@pytest.mark.parametrize("mode", ["All", "interOnly"])
def test_table_path_overflow_beyond_its_list(mode, tmp_path, monkeypatch):
    """g. No bias file, fixed-size loci: K2 evaluates a (distance, count) table and the rows gather from it; rows whose count is
    above the table's cap are listed and evaluated in place - and when they are more than the list holds (max(rows / 16, 1024)),
    k2_memo_overflow scans the whole column for the -1.0 marks instead.  That third exit: p and q bit-equal to the run without the
    table (FHX_NO_MEMO=1), p within 1e-10 of the oracle."""
    from fithic_amd import tables
    from fithic_amd.engine import Engine
    from oracle import fithic_oracle as fo
    paths, kw = _overflow_case(str(tmp_path), mode)
    ref = fo.run(paths["contacts"], paths["frags"], None, kw["resolution"], kw["n_bins"], 1, kw["mode"], kw["L"], kw["U"], 1, 0.5, 2.0)[0]
    chroms = tables.ChromIndex()
    con = tables.read_contacts(paths["contacts"], chroms)
    frags = tables.read_fragments(paths["frags"], chroms)
    got = {}
    for memo in (True, False):
        monkeypatch.delenv("FHX_NO_MEMO", raising=False)
        if not memo:
            monkeypatch.setenv("FHX_NO_MEMO", "1")
        eng = Engine(0)
        try:
            eng.configure(kw["resolution"], kw["L"], kw["U"], kw["n_bins"], 1, kw["mode"], 0.5, 2.0)
            eng.load_fragments(*frags, chroms.sort_rank())
            eng.load_contacts(con.chr1, con.mid1, con.chr2, con.mid2, con.count)
            out = eng.run_pass()
            got[memo] = eng.fetch(p=True, q=True)
            max_count = int(out.stats["max_count"])
        finally:
            eng.close()
    # plan_k2's formula: the table holds counts 0..cap for each of memo_nd distances (+ one column for the inter binomial)
    n_rows = len(con)
    memo_nd = 0 if mode == "interOnly" else 48 - 1 + 1
    per_count = memo_nd + 1
    cap = min(max_count, min(1 << 24, n_rows // 4) // per_count - 1)
    assert cap >= 8
    dist = np.abs(con.mid1.astype(np.int64) - con.mid2) // kw["resolution"]
    inter = con.chr1 != con.chr2
    live = np.ones(n_rows, bool) if mode == "interOnly" else (inter | ((dist >= 1) & (dist <= 48)))
    n_over = int((live & (con.count > cap)).sum())
    print("%s: %d rows, table cap %d, %d rows above it, list capacity %d" % (mode, n_rows, cap, n_over, max(n_rows // 16, 1024)))
    assert n_over > max(n_rows // 16, 1024)                        # the list overflowed: the third exit ran
    if mode == "All":
        assert 90 <= cap <= 110
    assert bits_equal(got[True]["p"], got[False]["p"]) and bits_equal(got[True]["q"], got[False]["q"])
    assert max_abs_diff(got[True]["p"], ref.p) <= TOL
