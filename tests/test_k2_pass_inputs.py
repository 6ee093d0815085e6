"""The inputs of tests/test_gpu_k2_pass.py, checked without a GPU: the generators of tests/k2_rows.py must reach every outcome of
k2_classify under both kinds of kernels, or the GPU tests would pass without testing anything."""
import os

import numpy as np

import k2_rows as kr
from conftest import bits_equal, GOLDEN


def _sets_a_to_c():
    """the Rows of the GPU tests a (scipy fixture), b (class boundaries), c (small totals)"""
    fx = kr.fixture_rows()
    totals = sorted(fx)
    for j, nt in enumerate(totals):
        other = totals[(j + 1) % len(totals)]
        yield kr.two_sided(nt, fx[nt][:2], other, fx[other][:2])
    for n_intra, n_inter in kr.BOUNDARY_PAIRS:
        if max(n_intra, n_inter) < 2 ** 31:                     # the wide total is run on a context with FHX_TOTALS_WIDE
            yield kr.boundary_case(n_intra, n_inter)
    for _, r in kr.small_total_cases():
        yield r


def test_oracle_reproduces_the_scipy_fixture_bit_for_bit():
    from oracle import fithic_oracle as fo
    g = np.load(os.path.join(GOLDEN, "f3_bdtrc.npz"))
    sel = g["k"] == np.floor(g["k"])
    assert int(sel.sum()) == 12956
    assert bits_equal(fo.bdtrc(g["k"][sel], g["n"][sel].astype(np.float64), g["p"][sel]), g["val"][sel])


def test_restated_thresholds_separate_the_classes():
    """thresholds() is cls_row restated: on both sides of each threshold the restated bdtrc_class changes as cls_lookup says"""
    for n_total in kr.BOUNDARY_TOTALS:
        counts = kr.boundary_counts(n_total)
        counts = counts[(counts >= 2) & (counts <= n_total)]
        thr = kr.thresholds(n_total, counts)
        for c, (tA, tB, tC, tD, tE) in zip(counts, thr):
            for t in (tA, tB, tC, tD, tE):
                if not 0.0 < t < 1.0:
                    continue
                for x in kr._neighbours(float(t), 3, 3):
                    if not 0.0 < x < 1.0:
                        continue
                    if x <= tA:
                        want = kr.PSERIES
                    elif x > tB:
                        want = kr.PSERIES if x >= tC else (kr.CF_SWAPPED if x >= tD else kr.CF_BD)
                    else:
                        want = kr.CF_BCF if x <= tE else kr.CF_BD
                    assert int(kr.bdtrc_class(np.array([c]), n_total, np.array([x]))[0]) == want, (n_total, c, x)


def test_every_outcome_is_reached_on_both_binomials_and_both_kernel_kinds():
    per = np.zeros((2, 7), np.int64)                  # [binomial][outcome]
    kinds = {c: set() for c in (kr.PSERIES, kr.CF_BCF, kr.CF_BD, kr.CF_SWAPPED)}
    for r in _sets_a_to_c():
        o = r.outcomes()
        for side in (0, 1):
            per[side] += np.bincount(o[r.is_inter == side], minlength=7)
        for c in kinds:
            if (o == c).any():
                kinds[c].add(kr.plan_small_n(r.n_intra, r.n_inter))
    assert (per >= 64).all(), {kr.OUTCOME_NAMES[c]: per[:, c].tolist() for c in range(7)}
    assert all(v == {False, True} for v in kinds.values()), kinds


def test_small_n_is_on_for_one_table_only_and_for_both():
    seen = set()
    for _, r in kr.small_total_cases():
        seen.add((bool(kr.small_n(r.n_intra) and r.n_intra >= 1), bool(kr.small_n(r.n_inter) and r.n_inter >= 1)))
    assert seen == {(False, False), (True, False), (False, True), (True, True)}


def test_handback_selection_is_not_empty():
    cases = list(kr.handback_cases())
    assert sum(n for _, _, n in cases) > 200
    for name, r, n_back in cases:
        o = r.outcomes()
        if name.startswith("handback"):
            assert n_back > 0, name
            assert ((o == kr.CF_SWAPPED) & ~kr.handed_back(r.count, r.totals(), r.prior) & (r.count < kr.K2H_KCAP)).sum() > 0 or "generic" in name, name
        if "generic" in name:
            assert ((o == kr.CF_SWAPPED) & (r.count >= kr.K2H_KCAP)).sum() >= 100, name
    # the example of the issue
    assert kr.handed_back(np.array([80]), 100.0, np.array([0.9]))[0]


def test_layout_cases_hold_what_they_promise():
    for m in (127, 128, 129, 255, 256, 257):
        r = kr.heavy_bucket_case(m, 40 + m)
        sw = r.outcomes() == kr.CF_SWAPPED
        assert int((sw & (r.count == 7) & (r.is_inter == 0)).sum()) == m
        assert len(np.unique(r.outcomes())) == 7
    for which in (kr.CF_BCF, kr.CF_BD):
        for m in (1023, 1024, 1025):
            r = kr.sorted_class_case(which, m, 60 + m)
            assert int((r.outcomes() == which).sum()) == m
    for m in kr.ROW_COUNTS:
        assert len(kr.mixed_rows(m, 80 + m)) == m
    assert len(np.unique(kr.mixed_rows(4097, 80 + 4097).outcomes())) == 7


def test_oracle_has_few_nan_outside_the_domain_edges():
    from oracle import fithic_oracle as fo
    sets = list(_sets_a_to_c())
    sets += [r for _, r, _ in kr.handback_cases()]
    sets += [kr.mixed_rows(m, 80 + m) for m in kr.ROW_COUNTS if m >= 255]
    sets += [kr.heavy_bucket_case(m, 40 + m) for m in (127, 128, 129, 255, 256, 257)]
    sets += [kr.sorted_class_case(w, m, 60 + m) for w in (kr.CF_BCF, kr.CF_BD) for m in (1023, 1024, 1025)]
    for r in sets:
        deliberate = ~(r.prior <= 1.0) | (r.count - 1.0 > r.totals())              # NaN prior, prior above 1, count beyond the total
        ref = fo.bdtrc(r.count.astype(np.float64) - 1, r.totals(), r.prior)
        assert np.isnan(ref[~deliberate]).sum() <= 0.01 * len(r), (r.n_intra, r.n_inter)
