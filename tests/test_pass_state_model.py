"""The inputs of tests/test_gpu_pass_state.py, checked without a GPU: tests/pass_state_model.py is tied to the oracle (the device's
representation of the outlier state - a flag byte per row and one limit - against the reference's walk over its sorted multiset;
the histogram of outlier distances against the distances themselves), every scenario reaches what it is for, and the oracle's fit
goes through on every round, so that no GPU case can pass without testing anything or stop at a failed fit."""
import numpy as np
import pytest

import pass_state_model as pm
from oracle import fithic_oracle as fo


def _rounds(sc, sel=None):
    """(round number, Round or None, Model) before the first round and after each one"""
    m = pm.Model(sc, sel)
    yield 0, None, m
    for k, rnd in enumerate(sc.schedule, 1):
        m.fold(rnd.rows)
        yield k, rnd, m


@pytest.fixture(scope="module")
def scenarios():
    return list(pm.all_scenarios())


def test_flags_and_limit_are_the_references_walk(scenarios):
    """the device keeps `flag byte per row` and `limit`; K1 skips flags & (line <= limit).  That must be fithic.py:408-412's walk with
    a forward-only cursor over the sorted multiset of line numbers - after every round of every scenario, and on random schedules."""
    for sc in scenarios:
        for k, _, m in _rounds(sc):
            assert np.array_equal((m.skip_bytes() != 0) & (np.arange(sc.n) <= m.limit()), fo.effective_skip_mask(sc.n, m.outlier_lines)), (sc.name, k)
    rng = np.random.default_rng(408)
    seen_dup = 0
    for _ in range(3000):
        n = int(rng.integers(1, 41))
        flags, limit, lines = np.zeros(n, bool), pm.INT64_MAX, []
        for _ in range(int(rng.integers(1, 6))):
            rows = np.flatnonzero(rng.random(n) < rng.choice([0.0, 0.1, 0.3, 0.7]))
            dup = rows[flags[rows]]                               # what the fold kernels do: atomicMin over the rows flagged before
            if len(dup):
                limit = min(limit, int(dup.min()))
                seen_dup += 1
            flags[rows] = True
            lines.extend(rows.tolist())
            assert np.array_equal(flags & (np.arange(n) <= limit), fo.effective_skip_mask(n, lines)), (n, lines)
    assert seen_dup > 1000


def test_histogram_of_outlier_distances_loses_nothing(scenarios):
    """fixed size: the device keeps bincount(index) instead of the distances.  make_bins fed index * resolution for every entry
    must make the bins it makes from the true distances (an inter-chromosomal distance is rounded UP to the grid: bins end there)"""
    checked = 0
    for sc in scenarios:
        if not sc.fixed:
            continue
        for k, _, m in _rounds(sc):
            if k == 0 or sc.schedule[k - 1].last:
                continue
            m.next_k1()
            true = m.next_bins()[0]
            hist = m.dist_hist(sc.n_dist())
            assert hist.sum() == m.total()
            coded = m.next_bins(np.repeat(np.arange(len(hist)) * sc.res, hist))[0]
            for key in true:
                assert np.array_equal(true[key], coded[key]), (sc.name, k, key)
            checked += 1
    assert checked > 60


def test_every_scenario_reaches_what_it_is_for(scenarios):
    by = {sc.name: sc for sc in scenarios}
    # a. the limit at each residue mod 4 in K1's first and second workgroup, and on every tail row; flagged rows behind it in its
    # own group of four and in later groups
    for n in (4101, 4102, 4103, 4104):
        sc = by["narrow%d" % n]
        limits = [m.limit() for k, _, m in _rounds(sc) if k >= 2]
        assert limits == sorted(limits, reverse=True) and len(set(limits)) == len(limits)
        body = [v for v in limits if v < n - (n & 3)]
        assert {v % 4 for v in body if v < pm.K1_GROUP_ROWS} == {0, 1, 2, 3} and {v % 4 for v in body if v >= pm.K1_GROUP_ROWS} == {0, 1, 2, 3}
        assert max(body) < 2 * pm.K1_GROUP_ROWS and [v for v in limits if v >= n - (n & 3)] == list(range(n - 1, n - (n & 3) - 1, -1))
        for k, _, m in _rounds(sc):
            if k >= 2:
                behind = np.flatnonzero(m.skip_bytes())
                behind = behind[behind > m.limit()]
                assert len(behind) >= 1 or m.limit() == n - 1
                if m.limit() % 4 != 3 and m.limit() < n - (n & 3):
                    assert (behind // 4 == m.limit() // 4).any() and (behind // 4 > m.limit() // 4).any()
    # the limit alone: no flag before or behind it
    lone = [sc for sc in scenarios if sc.name.startswith("lone")]
    assert {sc.schedule[0].rows[0] % 4 for sc in lone} == {0, 1, 2, 3} and any(sc.schedule[0].rows[0] >= sc.n - (sc.n & 3) for sc in lone)
    for sc in lone:
        m = list(_rounds(sc))[-1][2]
        assert m.limit() == sc.schedule[0].rows[0] and m.skip_bytes().sum() == 1 and m.total() == 2
    # b. more bins inside the distance bounds than K1's 12-byte window holds
    wide = by["wide"]
    st = pm.Model(wide).next_k1()[0]
    assert wide.params["U"] == float("inf")
    lo, hi = -(-wide.params["L"] // wide.res), st["n_dist"] - 1               # launch_k1: hi = min(U / res, n_dist - 1)
    assert hi - lo + 1 > pm.K1_LDS_BINS and wide.fixed and wide.n & 3
    assert {m.limit() % 4 for k, _, m in _rounds(wide) if k >= 2} == {0, 1, 2, 3}
    # c. loaded out of order: K1's tail rows are flagged rows from the head of the file, their local positions behind every limit
    perm = by["permuted"]
    assert sorted(perm.load_order.tolist()) == list(range(perm.n)) and not np.array_equal(perm.load_order, np.arange(perm.n))
    tail = perm.load_order[perm.n - (perm.n & 3):]
    for k, _, m in _rounds(perm):
        if k >= 2:
            skipped = fo.effective_skip_mask(perm.n, m.outlier_lines)
            assert skipped[tail].sum() >= 2 and m.limit() < perm.n - 3          # skipped by file position, not by local position
            assert (m.skip_bytes()[perm.load_order[:8]] != 0).any()              # loaded first, flagged, behind the limit
    # two contexts: both hold the longest chromosome's last slot (one histogram length), outliers, and rows on both sides of the limit
    split = pm.split_scenario()
    assert sorted(np.concatenate(split.parts).tolist()) == list(range(split.n))
    for part in split.parts:
        assert split.n_dist(part) == split.n_dist() and not np.array_equal(part, np.arange(part[0], part[0] + len(part)))
        m = pm.Model(split, part)
        for r in split.schedule:
            m.fold(r.rows)
        assert np.isin(split.schedule[0].rows, part).sum() >= 3 and m.limit() != pm.INT64_MAX         # outliers and a duplicate of its own
    # e. five rounds: a triple occurrence (rounds 1, 2, 4), an empty round, a duplicate above the limit, one below
    five = by["five"]
    ms = [(m.limit(), m.total()) for _, _, m in _rounds(five)]
    assert len(five.schedule) == 5 and len(five.schedule[2].rows) == 0
    assert [pm.FIVE_T in r.rows for r in five.schedule] == [True, True, False, True, False]
    assert [lim for lim, _ in ms] == [pm.INT64_MAX, pm.INT64_MAX, pm.FIVE_Z, pm.FIVE_Z, pm.FIVE_Z, pm.FIVE_LOW]
    seen = np.concatenate([r.rows for r in five.schedule[:3]])
    assert np.intersect1d(five.schedule[3].rows, seen).tolist() == [pm.FIVE_T] and pm.FIVE_T > pm.FIVE_Z > pm.FIVE_LOW
    assert ms[3][1] == ms[2][1]
    # f. the threshold's neighbourhood; an inter-chromosomal outlier off the grid, one on the spare index, one at distance 0
    thr = by["threshold"]
    p = thr.schedule[0].p_column(1e-6)
    T = pm.THRESHOLD_ROWS
    assert p[T["thres"]] == 1e-6 and p[T["below"]] == np.nextafter(1e-6, 0) and p[T["above"]] == np.nextafter(1e-6, 1) and np.isnan(p[T["nan"]])
    assert p[T["zero"]] == 0 and not np.signbit(p[T["zero"]]) and p[T["negzero"]] == 0 and np.signbit(p[T["negzero"]]) and p[T["denormal"]] == 5e-324
    for sc in (thr, five):
        rows = sc.schedule[0].rows
        nd = sc.n_dist()
        assert sc.inter[pm.ROW_CLAMPED] and sc.inter[pm.ROW_ZERO_DIST] and pm.ROW_CLAMPED in rows and pm.ROW_ZERO_DIST in rows
        assert sc.dist[pm.ROW_CLAMPED] % sc.res != 0 and sc.dist[pm.ROW_ZERO_DIST] == 0
        # the largest index there is: ceil(d / res) <= slots of the longest chromosome = n_dist - 1, the spare one - the clamp's edge
        assert -(-sc.dist[pm.ROW_CLAMPED] // sc.res) == nd - 1 == sc.dist_index(np.array([pm.ROW_CLAMPED]), nd)[0]
        assert sc.dist[pm.ROW_CLAMPED] // sc.res == nd - 2
    for sc in scenarios:
        if sc.name.startswith(("narrow", "permuted", "five", "threshold")):
            out = np.concatenate([r.rows for r in sc.schedule])
            assert sc.fixed and (sc.inter[out] & (sc.dist[out] % sc.res != 0)).any(), sc.name
    # g. around the scan tile: its edges, nothing, everything
    for n in (1023, 1024, 1025, 2049):
        sc = by["fetch%d" % n]
        assert sc.schedule[0].rows.tolist() == sorted({0, min(1023, n - 1), min(1024, n - 1), n - 1})
        assert len(sc.schedule[1].rows) == 0 and len(sc.schedule[2].rows) == n and sc.schedule[2].last
    # d. irregular midpoints: a skipped row on a wave edge, on the tile edge, in the last partial tile; inter-chromosomal outliers
    # and equal distances in the list; the list grows in every round
    for kind in ("nonfixed", "offgrid"):
        for n in (4095, 4096, 4097, 8193):
            sc = by["%s%d" % (kind, n)]
            assert not sc.fixed and (sc.res == 0) == (kind == "nonfixed")
            first = sc.schedule[0].rows
            assert {63, 64, n - 1} <= set(first.tolist()) and (n < 4097 or {4095, 4096} <= set(first.tolist()))
            assert sc.inter[first].sum() >= 3
            d = sc.dist[first]
            assert len(np.unique(d)) < len(d)
            sizes = [m.total() for _, _, m in _rounds(sc)]
            assert sizes == sorted(set(sizes)) and len(sizes) == 4
            assert [m.limit() for _, _, m in _rounds(sc)][2:] == [n - 1, sc.schedule[2].rows[0]]


def _fit_checks(sc, m, k, limit=None):
    st, keys, cc, _ = m.next_k1(limit)
    arrays, bins, frag = m.next_bins()
    R = m.fit(bins, frag)                              # SystemExit / ZeroDivisionError here: the reference would not finish this pass
    assert R.N == m.n_tests(frag) and R.N > 0 and len(bins) >= 4, (sc.name, k)
    assert (arrays["s1"] > 0).all() and (arrays["s7"] > 0).all(), (sc.name, k)
    return st, keys, cc


def test_oracle_fit_goes_through_on_every_round(scenarios):
    """no bin mean on which the reference's spline stage exits, in no round that a pass follows; outliers stay at or below 2 % of the
    rows; counts fall with the distance (the mean count of the nearer half of the distances above that of the farther half)"""
    for sc in scenarios + [pm.split_scenario()]:
        for k, rnd, m in _rounds(sc):
            if rnd is not None and rnd.last:
                assert k == len(sc.schedule)
                continue
            assert m.total() <= 0.02 * sc.n, (sc.name, k)
            st, keys, cc = _fit_checks(sc, m, k)
            if k == 0:
                sel = ~sc.inter & fo.in_range(sc.dist, sc.params["L"], sc.params["U"])
                mid = np.median(sc.dist[sel])
                assert sc.count[sel & (sc.dist <= mid)].mean() > 2 * sc.count[sel & (sc.dist > mid)].mean(), sc.name
    split = pm.split_scenario()
    for part in split.parts:                               # each context fits on its own statistics, under the common limit
        for (k, _, m), (_, _, w) in zip(_rounds(split, part), _rounds(split)):
            _fit_checks(split, m, k, w.limit())


def test_shards_add_up_to_the_whole():
    split = pm.split_scenario()
    for (k, _, w), (_, _, a), (_, _, b) in zip(_rounds(split), _rounds(split, split.parts[0]), _rounds(split, split.parts[1])):
        want = w.next_k1()
        got = [m.next_k1(w.limit()) for m in (a, b)]
        assert pm.sum_stats([g[0] for g in got]) == want[0], k
        assert np.array_equal(got[0][2] + got[1][2], want[2]) and np.array_equal(got[0][3] + got[1][3], want[3])
        assert min(a.limit(), b.limit()) == w.limit() and a.total() + b.total() == w.total()
        nd = split.n_dist()
        assert np.array_equal(a.dist_hist(nd) + b.dist_hist(nd), w.dist_hist(nd))
