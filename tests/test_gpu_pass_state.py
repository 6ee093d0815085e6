"""The outlier state between passes - skip bytes, the "first duplicated outlier line" limit, the multiset of outlier
distances - on p columns written by the test: after a pass the p column is replaced through Context.device_ptr(0), so the test
chooses which rows are outliers and where the limit lands, instead of taking whatever the data produce.  tests/pass_state_model.py
builds the scenarios and says what the device must hold (tests/test_pass_state_model.py ties it to the oracle and checks that each
scenario reaches its kernel path and that every fit goes through).  Kernels under test: k1_classify_hist (narrow, wide, the file
position branch), nf_k1_classify, k_fold_outliers, nf_fold_outliers, the compaction behind fetch_outlier_rows, fhx_reset_passes.

Everything compared here is an integer (or a bit pattern): array_equal and ==, no tolerance."""
import numpy as np
import pytest

import pass_state_model as pm
from conftest import bits_equal

pytestmark = pytest.mark.gpu

BIN_ARRAYS = (("lb", "A_BIN_LB"), ("ub", "A_BIN_UB"), ("s2", "A_BIN_SUMCC"), ("s1", "A_BIN_POSS"), ("s7", "A_BIN_POSS7"))


@pytest.fixture(scope="module")
def scenarios():
    return {sc.name: sc for sc in pm.all_scenarios()}


def _load(c, sc, rows=None):
    """parameters, fragments and the file rows `rows` (default: all, in the scenario's load order) -> the file row of every local row"""
    from fithic_amd.engine import MODES
    P = sc.params
    c.set_params(P["resolution"], P["L"], P["U"], P["n_bins"], P["mapp_thres"], MODES[P["mode"]])
    c.load_fragments(*sc.frag_columns())
    if rows is None:
        rows = np.arange(sc.n) if sc.load_order is None else sc.load_order
    c.load_pairs(sc.chr1[rows], sc.mid1[rows], sc.chr2[rows], sc.mid2[rows], sc.count[rows])
    if not np.array_equal(rows, np.arange(sc.n)):
        c.set_global_rows(rows)
    return rows


def _check_stats(c, st, m, limit, what):
    """the statistics of the pass_stats that just ran, field by field, and its histograms, against the model's next K1"""
    from fithic_amd import _capi
    want, keys, cc, npairs = m.next_k1(limit)
    got = st.as_dict()
    for f in pm.STAT_FIELDS:
        assert got[f] == want[f], (what, f, got[f], want[f])
    assert np.array_equal(c.get_array(_capi.A_DIST_KEYS), keys), what
    assert np.array_equal(c.get_array(_capi.A_HIST_SUMCC), cc) and np.array_equal(c.get_array(_capi.A_HIST_NPAIRS), npairs), what


def _check_fit(c, info, m, what):
    from fithic_amd import _capi
    arrays, _, frag = m.next_bins()
    for key, which in BIN_ARRAYS:
        assert np.array_equal(c.get_array(getattr(_capi, which)), arrays[key]), (what, key)
    n_tests = m.n_tests(frag)
    assert info.bh_total_tests == n_tests and info.outlier_thres == 1.0 / n_tests, what


def _write_p(c, rnd, thres, rows):
    """the round's p column (file order) onto the device in the order the rows were loaded; checks what the device says about it"""
    p = rnd.p_column(thres)
    with np.errstate(invalid="ignore"):
        mine = np.isin(rows, np.flatnonzero(p < thres))
    assert np.array_equal(np.sort(rows[mine]), rnd.rows[np.isin(rnd.rows, rows)])
    local = np.ascontiguousarray(p[rows])
    c.copy(c.device_ptr(0), local.ctypes.data, 8 * len(local), 0)
    assert np.array_equal(c.fetch_outlier_rows(), np.flatnonzero(mine))
    assert np.array_equal(c.fetch_flags(len(rows), outlier=True)[0], mine.astype(np.uint8))


def _check_state(c, sc, m, total, rows, what):
    from fithic_amd import _capi
    assert total == m.total(), what
    assert np.array_equal(c.fetch_flags(len(rows), outlier=False, skip=True)[1], m.skip_bytes()), what          # both in load order
    if sc.fixed:
        assert np.array_equal(c.get_array(_capi.A_OUTLIER_DIST_HIST), m.dist_hist(sc.n_dist(rows))), what
    else:
        assert np.array_equal(c.get_array(_capi.A_OUTLIER_DISTS), m.dists_sorted()), what


def _snapshot(c, st, info, n):
    from fithic_amd import _capi
    out = dict(stats=st.as_dict(), n_tests=info.bh_total_tests, bins=info.n_bins_made, **c.fetch(n, p=True, q=True))
    for which in ("A_HIST_SUMCC", "A_HIST_NPAIRS", "A_DIST_KEYS") + tuple(w for _, w in BIN_ARRAYS):
        out[which] = c.get_array(getattr(_capi, which))
    return out


def _same_snapshot(a, b):
    assert a["stats"] == b["stats"] and a["n_tests"] == b["n_tests"] and a["bins"] == b["bins"]
    assert bits_equal(a["p"], b["p"]) and bits_equal(a["q"], b["q"])
    for k in a:
        if k.startswith("A_"):
            assert np.array_equal(a[k], b[k]), k


def drive(sc, c=None):
    """One context through the scenario: load, pass, then for every round write p, fold, pass - each step against the model.
    Returns the snapshot of the first pass."""
    from fithic_amd import _capi
    own = c is None
    c = _capi.Context(0) if own else c           # raises if there is no GPU or the library is missing: no fallback
    try:
        rows = _load(c, sc)
        whole = pm.Model(sc)
        local = whole if sc.load_order is None else pm.Model(sc, rows)        # a second model in load order when that differs
        st, info = c.run_pass()
        first = _snapshot(c, st, info, sc.n)
        for k, rnd in enumerate([None] + list(sc.schedule)):
            what = (sc.name, k)
            if rnd is not None:
                _write_p(c, rnd, info.outlier_thres, rows)
                total = c.next_pass()
                local.fold(rnd.rows)
                if local is not whole:
                    whole.fold(rnd.rows)
                _check_state(c, sc, local, total, rows, what)
                assert c.get_skip_limit() == whole.limit(), what
                if rnd.last:
                    break
                st, info = c.run_pass()
            _check_stats(c, st, local, None if local is whole else whole.limit(), what)      # None: the reference's walk itself
            _check_fit(c, info, local, what)
        return first
    finally:
        if own:
            c.close()


def test_scenario_names(scenarios):
    assert sorted(scenarios) == sorted(NARROW + LONE + IRREGULAR + FETCH + ["wide", "permuted", "five", "threshold"])


NARROW = ["narrow%d" % n for n in (4101, 4102, 4103, 4104)]
LONE = ["lone%d" % t for t in (1200, 1201, 2402, 2403, 4100, 4102)]
IRREGULAR = ["%s%d" % (kind, n) for kind in ("nonfixed", "offgrid") for n in (4095, 4096, 4097, 8193)]
FETCH = ["fetch%d" % n for n in (1023, 1024, 1025, 2049)]


@pytest.mark.parametrize("name", NARROW)
def test_narrow_k1_limit_at_every_position_of_a_row_group_and_in_the_tail(scenarios, name):
    """a. k1_classify_hist<512, false>: the limit on rows 4k .. 4k + 3 of its first and of its second workgroup and on every one of
    the n & 3 tail rows, flagged rows behind it in its own group of four and in later groups: those must be counted again"""
    drive(scenarios[name])


@pytest.mark.parametrize("name", LONE)
def test_limit_with_no_flag_before_or_behind_it(scenarios, name):
    """a. one row, an outlier twice: the only flagged row is the limit itself"""
    drive(scenarios[name])


def test_wide_k1_with_a_skip_mask(scenarios):
    """b. k1_classify_hist<1024, true> (more than 6144 bins inside the distance bounds) in passes 2 and later"""
    from fithic_amd import _capi
    sc = scenarios["wide"]
    c = _capi.Context(0)
    try:
        drive(sc, c)
        assert len(c.get_array(_capi.A_HIST_SUMCC)) > pm.K1_LDS_BINS and c.stats().n_skipped > 0
    finally:
        c.close()


def test_rows_loaded_out_of_order_are_skipped_by_file_position(scenarios):
    """c. set_global_rows(permutation): flags, outlier rows and the limit are file positions; K1's `grow` branch in one context"""
    drive(scenarios["permuted"])


def test_two_contexts_share_the_limit():
    """c. every third row on a second context; the test hands min(limit) to both after each next_pass, as the distributed entry
    points would.  Totals, skip bytes and the outlier histogram add up to the model of the whole file, and so do the statistics and
    histograms of the next pass_stats; each context's own statistics and bins are those of the model of its rows."""
    from fithic_amd import _capi
    sc = pm.split_scenario()
    ctxs = [_capi.Context(0) for _ in sc.parts]
    try:
        whole, models = pm.Model(sc), [pm.Model(sc, part) for part in sc.parts]
        for c, part in zip(ctxs, sc.parts):
            _load(c, sc, part)
        nd, limit = sc.n_dist(), pm.INT64_MAX
        for k, rnd in enumerate([None] + list(sc.schedule)):
            what = (sc.name, k)
            if rnd is not None:
                for c, part, info in zip(ctxs, sc.parts, infos):
                    _write_p(c, rnd, info.outlier_thres, part)
                totals = [c.next_pass() for c in ctxs]
                whole.fold(rnd.rows)
                for c, m, part, total in zip(ctxs, models, sc.parts, totals):
                    m.fold(rnd.rows)
                    _check_state(c, sc, m, total, part, what)
                    assert c.get_skip_limit() == min(limit, m.limit()), what          # the common limit it was given, or its own duplicate
                assert sum(totals) == whole.total()
                limit = min(c.get_skip_limit() for c in ctxs)
                assert limit == whole.limit(), what
                for c in ctxs:
                    c.set_skip_limit(limit)
                hist = sum(c.get_array(_capi.A_OUTLIER_DIST_HIST) for c in ctxs)
                assert np.array_equal(hist, whole.dist_hist(nd)), what
            stats = [c.pass_stats() for c in ctxs]
            want, _, cc, npairs = whole.next_k1()
            assert pm.sum_stats([s.as_dict() for s in stats]) == want, what
            assert np.array_equal(sum(c.get_array(_capi.A_HIST_SUMCC) for c in ctxs), cc), what
            assert np.array_equal(sum(c.get_array(_capi.A_HIST_NPAIRS) for c in ctxs), npairs), what
            infos = []
            for c, m, st in zip(ctxs, models, stats):
                _check_stats(c, st, m, whole.limit(), what)
                infos.append(c.fit())                           # on the context's own statistics: p exists again, with its own threshold
                _check_fit(c, infos[-1], m, what)
                c.pvalues()
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("name", IRREGULAR)
def test_irregular_midpoints_skip_on_wave_and_tile_edges(scenarios, name):
    """d. nf_k1_classify and nf_fold_outliers (-r 0, and -r N on loci that share no grid): skipped rows on a wave edge, on the edge of
    a 4096-row tile and in the last, partial tile; inter-chromosomal and repeated distances in a list that grows for three passes"""
    drive(scenarios[name])


def test_five_rounds(scenarios):
    """e. a row that is an outlier in rounds 1, 2 and 4, a round without outliers, a duplicate above the limit (it stays) and one
    below it (it moves down)"""
    drive(scenarios["five"])


def test_threshold_and_spare_index(scenarios):
    """f. p == 1 / N is no outlier, the double below it is, the double above it and NaN are not, 0.0, -0.0 and 5e-324 are; an
    inter-chromosomal outlier is counted at its distance rounded up to the grid - here onto the spare last index - or at 0"""
    drive(scenarios["threshold"])


@pytest.mark.parametrize("name", FETCH)
def test_fetch_outlier_rows_around_its_scan_tile(scenarios, name):
    """g. 1023, 1024, 1025 and 2049 rows: outliers on the tile's edges, none at all (an empty result), every row"""
    drive(scenarios[name])


def test_reset_and_reload_start_from_the_first_pass(scenarios):
    """h. after the five rounds of (e): reset_passes clears skip bytes, limit and outlier histogram; the next pass is the first pass
    again, bit for bit, and next_pass counts from zero.  The same after load_pairs on a context that carries state."""
    from fithic_amd import _capi
    sc = scenarios["five"]
    c = _capi.Context(0)
    try:
        first = drive(sc, c)
        assert c.get_skip_limit() == pm.FIVE_LOW and c.stats().n_skipped > 0
        for again in ("reset", "reload"):
            if again == "reset":
                c.reset_passes()
            else:
                _load(c, sc)
            assert not c.fetch_flags(sc.n, outlier=False, skip=True)[1].any(), again
            assert c.get_skip_limit() == _capi.INT64_MAX and not c.get_array(_capi.A_OUTLIER_DIST_HIST).any(), again
            st, info = c.run_pass()
            _same_snapshot(_snapshot(c, st, info, sc.n), first)
            m = pm.Model(sc)
            for rnd in sc.schedule[:2]:                             # and the state builds up again as it did
                _write_p(c, rnd, info.outlier_thres, np.arange(sc.n))
                total = c.next_pass()
                m.fold(rnd.rows)
                _check_state(c, sc, m, total, np.arange(sc.n), again)
                assert c.get_skip_limit() == m.limit()
                st, info = c.run_pass()
                _check_stats(c, st, m, None, again)
            assert m.total() == len(sc.schedule[0].rows) + len(sc.schedule[1].rows) and c.stats().n_skipped > 0
    finally:
        c.close()
