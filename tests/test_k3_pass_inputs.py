"""The inputs of tests/test_gpu_k3_pass.py, checked without a GPU: the model of tests/k3_columns.py is tied to the oracle's
Benjamini-Hochberg, and the columns must reach every branch the GPU tests are there for - or those would pass without testing it.

No GPU test of that file skips: a row set whose fit does not go through fails its test there (the sizes were chosen so that every
fit does)."""
import numpy as np
import pytest

import k3_columns as kc


def _all_columns():
    for case in kc.size_cases():
        yield kc.make(case)
    yield from kc.strip_columns()
    yield from kc.far_below_sequence()
    for n_small, _, seed in kc.LARGE_CASES:
        yield kc.large_column(n_small, seed)


@pytest.fixture(scope="module")
def columns():
    return list(_all_columns())


def test_values_stay_inside_the_engines_contract(columns):
    for c in columns:
        ok = np.isnan(c.p) | ((c.p >= 0.0) & (c.p <= 1.0))
        assert ok.all() and c.N > 0, c.name


def test_model_survivors_cover_every_row_the_oracle_ranks_below_one(columns):
    """every row with q < 1 is below the restated cutoff, and the oracle's q is 1.0 exactly on every row the cutoff spares"""
    from oracle import fithic_oracle as fo
    for c in columns:
        q = fo.benjamini_hochberg(c.p, c.N)
        kept = kc.survivors(c.p, c.N)
        nan = np.isnan(c.p)
        assert np.array_equal(np.isnan(q), nan), c.name
        with np.errstate(invalid="ignore"):
            assert not (~kept & (q < 1.0)).any(), c.name
        assert (q[~kept & ~nan] == 1.0).all(), c.name


def test_cutoff_restates_the_oracles_pruning_bound():
    """on a column where a bin in the middle saturates: the survivors are exactly the values below that bin's edge"""
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.random(3000) * 1e-6, 0.01 + 0.98 * rng.random(5000), np.ones(100), [np.nan] * 4])
    rng.shuffle(p)
    # (about 3000 + 5000 (e' - 0.01) / 0.98 values below the end e' of a bin: [0.5, 0.625) gives 0.5 * 12000 < 6138, the next bin
    # 0.625 * 12000 >= 6775)
    ck, kept = kc.cutoff(p, 12000.0)
    edge = np.array([ck], np.uint64).view(np.float64)[0]
    assert edge == 0.625 and 3000 < kept == np.count_nonzero(p < edge)
    assert (ck >> kc.TOP_SHIFT) << kc.TOP_SHIFT == ck
    # N = 1: nothing saturates unless a single value is all there is
    assert kc.cutoff(p, 1.0) == (kc.KEY_KEEP_ALL, len(p) - 4)
    assert kc.cutoff(np.array([1.0, np.nan]), 1.0) == (0x3FF0000000000000, 0)
    # -0.0 is counted with +0.0
    assert kc.keys(np.array([-0.0, 0.0, 5e-324])).tolist() == [0, 0, 1]


def test_generators_hold_what_they_promise():
    for n in kc.SIZES:
        for at in (-1, 0):
            c = kc.threshold(n, 3, at)
            assert kc.cutoff(c.p, c.N)[1] == kc.dense_min(n) + at
        assert 100 * kc.dense_min(n) >= 35 * n > 100 * (kc.dense_min(n) - 1)
        s = kc.sparse(n, 4)
        assert (s.p[~kc.survivors(s.p, s.N)] == 1.0).all() and abs(kc.cutoff(s.p, s.N)[1] - 0.005 * n) <= 1
        assert kc.cutoff(*kc.all_survive(n, 5)[1:]) == (kc.KEY_KEEP_ALL, n)
        c = kc.nothing_saturates(n, 6)
        assert kc.cutoff(c.p, c.N) == (kc.KEY_KEEP_ALL, n - 3) and (c.p == 1.0).sum() > 100
        assert kc.cutoff(*kc.nothing_survives(n, 7)[1:])[1] == 0 and kc.cutoff(*kc.nan_only(n, 8)[1:]) == (kc.KEY_KEEP_ALL, 0)
        for frac in (0.05, 0.5):
            c = kc.nan_ends(n, 9, frac)
            assert np.isnan(c.p[[0, n - 1]]).all()
            for member in (0, 1):
                c = kc.nan_pairs(n, 10, frac, member)
                kept, nan = kc.survivors(c.p, c.N), np.isnan(c.p)
                pairs = np.flatnonzero(nan[member:n // 2 * 2:2] & kept[1 - member:n // 2 * 2:2])
                assert len(pairs) >= 300 and pairs[0] == 0 and pairs[-1] == n // 2 - 1 and not nan[1 - member::2].any()
            c = kc.nan_chunk(n, 11, frac)
            assert np.isnan(c.p[3 * kc.CHUNK:4 * kc.CHUNK]).all() and np.isnan(c.p[n - 1]) and not np.isnan(c.p[:3 * kc.CHUNK]).any()
        c = kc.zeros(n, 12, 0.4)
        kept = kc.survivors(c.p, c.N)
        for z in kc.ZEROS:
            assert (kept & (c.p == z) & (np.signbit(c.p) == np.signbit(z))).sum() > 50, z
        c = kc.ties(n, 13, 0.2)
        assert len(np.unique(c.p[kc.survivors(c.p, c.N)])) == 7


def test_strip_columns_place_their_survivors():
    want = {"strip_third_does_not_fit": ([5, 2043, 1, 0], [True, True, False, True], [2048]),
            "strip_exactly_full": ([2048], [True], [2048]),
            "strip_dense_tile_first": ([2049, 10], [False, True], [10]),
            "strip_fourth_does_not_fit": ([600, 600, 600, 600], [True, True, True, False], [1800]),
            "strip_short_last_group": ([300, 300, 300, 300, 2000, 49], [True, True, True, True, True, False], [1200, 2000])}
    for c in kc.strip_columns():
        totals, plan, fill = want[c.name]
        kept = kc.survivors(c.p, c.N)
        tot = kc.tile_survivors(kept)
        assert tot.tolist() == totals and kc.strip_plan(tot, 4) == plan and kc.strip_fill(tot, 4) == fill, c.name
        assert kc.strip_plan(tot, 1) == [False] * len(totals)
        assert kc.predict(c.p, c.N)[0] == 1                          # below 35 %: the scattered variant, the one that has a strip
        for t, n_t in enumerate(totals):
            rows = min(kc.TILE, len(c.p) - t * kc.TILE)
            corners = [r for r in kc.CORNERS if r < rows][:n_t]
            assert kept[t * kc.TILE + np.array(corners, np.int64)].all(), (c.name, t)
    last = kc.strip_columns()[-1]
    assert len(last.p) % 2 == 1 and len(last.p) % kc.TILE != 0 and -(-len(last.p) // kc.TILE) % 4 != 0
    assert sorted(kc.CORNERS) == [0, 126, 897, 1023, 15360, 15486, 16257, 16383]
    # the fourth-tile column also splits under two and three tiles per workgroup
    tot = kc.tile_survivors(kc.survivors(*kc.strip_columns()[3][1:]))
    assert kc.strip_plan(tot, 2) == [True] * 4 and kc.strip_plan(tot, 3) == [True, True, True, True]


def test_every_named_branch_is_predicted_at_least_once(columns):
    seen = {k: set() for k in (0, 4, 5, 6)}
    zero_tile = False
    for case in kc.size_cases():
        c = kc.make(case)
        for warm in (False, True):                               # each case runs on a context's first pass and on a later one
            info = kc.predict(c.p, c.N, (len(c.p), kc.cutoff(c.p, c.N)[1]) if warm else None, prefilled=warm)
            for k in seen:
                seen[k].add(info[k])
            if info[1] >= kc.dense_min(len(c.p)):
                assert info[0] == 2                              # far_below never takes the dense path from a column built for it
        zero_tile |= bool((kc.tile_survivors(kc.survivors(c.p, c.N)) == 0).any())
    for n_small, env, seed in kc.LARGE_CASES:
        c = kc.large_column(n_small, seed)
        info = kc.predict(c.p, c.N, small_off=env.get("FHX_K3_SMALL") == "0", legacy=env.get("FHX_K3_SORT") == "legacy")
        assert info[1] == n_small
        seen[4].add(info[4])
        seen[0].add(info[0])
    last = None
    far = []
    for c in kc.far_below_sequence():
        info = kc.predict(c.p, c.N, last, prefilled=last is None)
        far.append((info[5], info[0]))
        for k in seen:
            seen[k].add(info[k])
        last = (len(c.p), info[1])
    assert far == [(0, 1), (1, 0), (0, 1), (1, 0), (0, 2)]
    assert seen[0] == {0, 1, 2} and seen[5] == {0, 1} and seen[6] == {0, 1} and seen[4] >= {0, 1, 2, 3}, seen
    plans = [kc.strip_plan(kc.tile_survivors(kc.survivors(c.p, c.N)), 4) for c in kc.strip_columns()]
    assert any(True in pl[g:g + 4] and False in pl[g:g + 4] for pl in plans for g in range(0, len(pl), 4))      # both inside one group
    assert any(kc.STRIP in kc.strip_fill(kc.tile_survivors(kc.survivors(c.p, c.N)), 4) for c in kc.strip_columns())
    assert zero_tile and any(0 in kc.tile_survivors(kc.survivors(c.p, c.N)) for c in kc.strip_columns())


def test_chosen_cross_product_covers_sizes_and_parities():
    cases = kc.size_cases()
    assert len({cid for cid, *_ in cases}) == len(cases)
    for n in kc.SIZES:
        assert {name for name, _, _ in kc.EVERY_SIZE} <= {cid.rsplit("-", 1)[0] for cid, m, _, _ in cases if m == n}
        assert sum(1 for _, m, _, _ in cases if m == n) >= 4
    for name, gen, kw in kc.SOME_SIZES:
        sizes = [m for _, m, g, k in cases if g is gen and k == kw]
        assert any(m & 1 for m in sizes) and any(not m & 1 for m in sizes), name
