"""k2h_heavy with one convergence compare per wave step (cf_swapped_step, fhx_bdtrc.hpp): every lane of a wave has to behave like a
live row, so lanes behind a bucket's entries run a copy of its last entry and lanes that finish go on as copies of a lane that has
not.  None of that may leave a trace.  Through the fhx_debug_k2_rows hook, each case under the default heavy kernel (two rows per
lane), FHX_K2H_ROWS=4 and FHX_K2_LEGACY=1 (heavy_variants of test_gpu_k2_pass.py): p bit-equal across the three and to
Context.bdtrc_array, within 1e-10 of the oracle, the number of rows handed back as predicted, the fused histogram within check_hist's
inequalities.

The order of a bucket's entries in the sorted queue is free (k2h_scatter), so which rows share a wave is not known here.  The cases
are built so that what they claim holds for EVERY order: see early_finish_buckets."""
import numpy as np
import pytest

import k2_rows as kr
from test_gpu_k2_pass import check_hist, heavy_variants

gpu = pytest.mark.gpu          # two tests below only prepare the others and need no GPU

C3_TOTAL = 645040870.0
OTHER_TOTAL = 1.0e6
BUCKET_SIZES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)          # 1, 63..65, 64 R - 1 .. 64 R + 1 for R = 2 and R = 4
CF_CAP = 300


@pytest.fixture(scope="module")
def ctx():
    from fithic_amd import _capi
    c = _capi.Context(0)          # raises if there is no GPU or the library is missing: no fallback
    yield c
    c.close()


def predicted_redo(r):
    return int(kr.handed_back(r.count, r.totals(), r.prior).sum())


def run_variants(ctx, monkeypatch, r, what, want_redo=None):
    """the three variants (each already checked against bdtrc_array, the oracle and the class counts, and against each other);
    then the hand-back count and the histogram"""
    want = predicted_redo(r) if want_redo is None else want_redo
    out = heavy_variants(ctx, monkeypatch, r, what)
    for (p, by_class, n_redo, hist), legacy in zip(out, (False, False, True)):
        assert n_redo == (0 if legacy else want), (what, legacy, n_redo, want)
        check_hist(r, p, hist, exact=legacy)
    return out


# ---- 1. padding ---------------------------------------------------------------------------------------------------------------
def one_bucket(m, count, inter, seed):
    """m swapped-class rows of ONE (binomial, count) bucket under C3's total, inside a shuffled mix of every class whose swapped
    rows avoid that bucket"""
    rng = np.random.default_rng(seed)
    n_intra, n_inter = (OTHER_TOTAL, C3_TOTAL) if inter else (C3_TOTAL, OTHER_TOTAL)
    prior = np.clip((count / C3_TOTAL) * np.exp(np.abs(rng.normal(0.7, 0.8, m)) + 0.05), 0.0, 0.5)
    bucket = kr.Rows(n_intra, n_inter, np.full(m, count, np.int32), prior, np.full(m, 1 if inter else 0, np.uint8))
    assert (bucket.outcomes() == kr.CF_SWAPPED).all() and not kr.handed_back(bucket.count, bucket.totals(), bucket.prior).any()
    rest = kr.mixed_rows(600, seed + 1, n_intra, n_inter)
    same = (rest.count == count) & ((rest.is_inter != 0) == inter) & (rest.outcomes() == kr.CF_SWAPPED)
    rest = rest.take(np.flatnonzero(~same))
    n_rest = len(rest)
    return kr.Rows.concat([rest, bucket]), n_rest                      # not shuffled: the first n_rest rows are the unrelated ones


@gpu
@pytest.mark.parametrize("inter", [False, True])
@pytest.mark.parametrize("count", [2, 17, 1022])
def test_padding_lanes_leave_no_trace(ctx, monkeypatch, count, inter):
    """One bucket of 1 .. 64 R + 1 rows: up to 64 R - 1 lanes of its last task hold a copy of the bucket's last entry.  The unrelated
    rows' p are the bits they have without the bucket, the class counts and the histogram's total are the live rows' (a copy that
    was stored, counted or handed back would show in one of them)."""
    alone = None
    for m in BUCKET_SIZES:
        r, n_rest = one_bucket(m, count, inter, 500 + count)          # same seed: the same unrelated rows for every m
        out = run_variants(ctx, monkeypatch, r, (count, inter, m))
        p, by_class, n_redo, hist = out[0]
        assert by_class["cf_swapped"] == int((r.outcomes() == kr.CF_SWAPPED).sum())
        assert int(hist.sum()) == int((~np.isnan(p)).sum())
        if alone is None:
            rest = r.take(np.arange(n_rest))
            alone = ctx.debug_k2_rows(rest.n_intra, rest.n_inter, rest.count, rest.prior, rest.is_inter)[0]
        assert np.array_equal(p[:n_rest].view(np.int64), alone.view(np.int64)), (count, inter, m)


# ---- 2. lanes that finish at different steps in one wave --------------------------------------------------------------------------
EARLY_TOTALS = (2.0e3, 6.0e3, 2.0e4, 6.0e4, 2.0e5, 6.0e5, 1.0e6)
EARLY_COUNTS = (2, 3, 5, 8, 13, 20, 30, 40)
PER_BUCKET = 256                                                      # one task of four rows per lane, two of two: no padding


def swapped_iterations(count, total, prior):
    """iterations of Cephes' continued fraction for swapped-class rows, from the oracle's C loop (its n at the exit: < 300 when the
    row converged, 300 when it ran to the cap)"""
    from oracle import fithic_oracle as fo
    _, branch, iters = fo.bdtrc_stats(np.asarray(count, np.float64) - 1.0, total, prior)
    assert (branch == 6).all()                                        # incbcf, swapped
    return iters


_EARLY = {}


def early_finish_buckets():
    """{total: [(count, priors, iterations)]}: 256 priors per (total, count), spread over (count / total, 0.95), all of the swapped
    class and inside cf_swapped_regular.  Computed once."""
    if not _EARLY:
        for total in EARLY_TOTALS:
            for count in EARLY_COUNTS:
                lo = count / total
                cand = lo + (0.95 - lo) * (np.arange(1, 4097) / 4097.0) ** 3          # denser towards count / total
                cnt = np.full(len(cand), count, np.int32)
                keep = np.flatnonzero((kr.outcome(cnt, total, cand) == kr.CF_SWAPPED) & ~kr.handed_back(cnt, total, cand))
                if len(keep) < PER_BUCKET:
                    continue
                pri = cand[keep[np.linspace(0, len(keep) - 1, PER_BUCKET).astype(np.int64)]]
                _EARLY.setdefault(total, []).append((count, pri, swapped_iterations(cnt[:PER_BUCKET], total, pri)))
    return _EARLY


def bucket_kinds(iters):
    """what a bucket of 256 rows guarantees WHATEVER the order of its entries (tasks of 128 or 256 entries, all full):
    a: every row finishes early - so does every wave;
    b: 1..127 rows run to the cap - the task that holds one of them holds at most 127, so it holds an early row too;
    c: one row is slower than all others - in its task the other row slots hold only rows that finish before it does, so
       every lane of those slots is done while the slot of the slowest row still runs."""
    late = int((iters >= CF_CAP).sum())
    slowest = np.sort(iters)[-2:]
    return {"a": late == 0, "b": 1 <= late <= 127, "c": slowest[1] > slowest[0]}


def test_the_early_finish_set_holds_every_kind_of_wave():
    """no GPU needed for this one, but it guards the next: asserted from the oracle's iteration counts before any GPU call"""
    seen = {"a": 0, "b": 0, "c": 0}
    n = 0
    for total, buckets in early_finish_buckets().items():
        for count, pri, iters in buckets:
            n += 1
            for k, v in bucket_kinds(iters).items():
                seen[k] += bool(v)
    print("%d buckets: all early %d, early beside capped %d, one slowest row %d" % (n, seen["a"], seen["b"], seen["c"]))
    assert n >= 30 and min(seen.values()) >= 3, seen


@gpu
@pytest.mark.parametrize("j", range(len(EARLY_TOTALS)))
def test_lanes_finish_at_different_steps(ctx, monkeypatch, j):
    """the buckets of one total as the intra binomial, the next total's as the inter one: rows that converge after a few iterations
    beside rows that run to the cap, in every mixture"""
    b = early_finish_buckets()
    n_intra, n_inter = EARLY_TOTALS[j], EARLY_TOTALS[(j + 1) % len(EARLY_TOTALS)]
    kinds = [bucket_kinds(it) for t in (n_intra, n_inter) for _, _, it in b.get(t, [])]
    assert kinds and any(k["a"] or k["b"] or k["c"] for k in kinds)
    side = lambda t: (np.concatenate([np.full(len(pri), c, np.int32) for c, pri, _ in b.get(t, [])] or [np.zeros(0, np.int32)]),
                      np.concatenate([pri for _, pri, _ in b.get(t, [])] or [np.zeros(0)]))
    r = kr.two_sided(n_intra, side(n_intra), n_inter, side(n_inter)).shuffled(np.random.default_rng(70 + j))
    assert (r.outcomes() == kr.CF_SWAPPED).all()
    run_variants(ctx, monkeypatch, r, (n_intra, n_inter), want_redo=0)


# ---- 3. and 4. rows outside cf_swapped_regular -----------------------------------------------------------------------------------
def test_irregular_input_is_a_property_of_the_bucket():
    """cf_swapped_regular(bb, aa, 1 - prior) can fail for a swapped-class row only through aa > bb, i.e. count > (total + 1) / 2 -
    1 - prior lies in [2^-53, 1) for every prior the class admits.  So a task holds regular rows or rows irregular on input, never
    both: the hook cannot put a hand-back row and a regular row of the same count into one task, and case 3 below interleaves them
    with regular rows of the same counts under the OTHER binomial's total instead.  (No GPU needed.)"""
    rng = np.random.default_rng(2)
    for total in kr.HANDBACK_TOTALS:
        cs, _ = kr.handback_rows(total, rng)
        assert len(cs) and (cs > (total + 1.0) / 2.0).all()
        for c in np.unique(cs):
            pri = rng.uniform(0.0, 1.0, 400)
            cnt = np.full(len(pri), c, np.int32)
            sw = kr.outcome(cnt, total, pri) == kr.CF_SWAPPED
            assert kr.handed_back(cnt, total, pri)[sw].all()


@gpu
def test_handbacks_beside_regular_rows(ctx, monkeypatch):
    """3. kr.handback_cases() with, for every count that is handed back under one total, regular rows of the same count under a total
    large enough for it: the hand-back bucket and the regular one run in the same launch, the number handed back is the predicted
    one and every row - the regular ones among them - has the per-lane kernel's bits (run_and_check)."""
    rng = np.random.default_rng(21)
    total_back = 0
    for name, r, want_back in kr.handback_cases():
        back = kr.handed_back(r.count, r.totals(), r.prior)
        extra = []
        for side, big in ((0, r.n_intra), (1, r.n_inter)):
            counts = np.unique(r.count[back & (r.is_inter != side)])    # handed back under the other side's total
            counts = counts[(counts <= (big + 1.0) / 2.0) & (counts >= 2)]
            if len(counts):
                cnt = np.repeat(counts, 5).astype(np.int32)
                pri = np.clip((cnt / big) * np.exp(np.abs(rng.normal(0.5, 0.5, len(cnt))) + 0.05), 0.0, 0.9)
                sel = (kr.outcome(cnt, big, pri) == kr.CF_SWAPPED) & ~kr.handed_back(cnt, big, pri)
                extra.append(kr.Rows(r.n_intra, r.n_inter, cnt[sel], pri[sel], np.full(int(sel.sum()), side, np.uint8)))
        both = kr.Rows.concat([r] + extra).shuffled(rng) if extra else r
        assert predicted_redo(both) == want_back
        run_variants(ctx, monkeypatch, both, name, want_redo=want_back)
        total_back += want_back
    assert total_back > 200


@gpu
@pytest.mark.parametrize("m", [1, 64, 129, 256, 257])
def test_every_row_of_a_task_irregular_on_input(ctx, monkeypatch, m):
    """4. A bucket with count > (total + 1) / 2: no lane of its tasks is regular, there is nothing to copy from.  Every row comes
    back through the redo list with the per-lane kernel's bits."""
    rng = np.random.default_rng(90 + m)
    total, count = 100.0, 80
    pri = rng.uniform(0.81, 0.99, 4 * m + 64)
    cnt = np.full(len(pri), count, np.int32)
    sel = np.flatnonzero(kr.handed_back(cnt, total, pri))[:m]
    assert len(sel) == m
    r = kr.two_sided(total, (cnt[sel], pri[sel]), OTHER_TOTAL, kr.pool_rows(OTHER_TOTAL, 200, rng)).shuffled(rng)
    want = predicted_redo(r)
    assert want >= m
    run_variants(ctx, monkeypatch, r, m, want_redo=want)
