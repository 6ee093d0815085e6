"""The one-compare-per-wave convergence test of cf_swapped_step (fhx_bdtrc.hpp), restated in numpy for four rows per lane, against
the per-row condition it replaced:  |d| > fl(T |c2|)  and  |c2| > 2^-600  with  c2 = fl(p2 q0),  d = fma(p0, q2, -c2).

The fast path forms e = fma(-T, |c2|, |d|) per row, takes the minimum of the lane's eight values e[r], |c2[r]| on their HIGH WORDS read
as binary32 (np.fmin: like v_min*_f32 it skips a NaN operand) and compares it once with the high word of 2^-600.  What must hold is
one implication: where the fast path passes, the replaced condition holds for all four rows - the other direction only costs a visit
to the exact block.  fma is computed exactly here (python fractions), then rounded once.

One case is NOT covered by that implication and is pinned separately: |d| == fl(T |c2|) where that product was rounded up.  The fast
path passes it (|d| > T |c2| exactly, which is the premise the kernel's proof needs), the two-rounding compare did not."""
from fractions import Fraction

import numpy as np
import pytest

T = 1e-15                                   # kCfLazyT
GUARD = 2.0 ** -600
GUARD_HI = np.array([0x1A700000], np.uint32).view(np.float32)[0]          # high word of 2^-600 as binary32
BANDS = (-700, -650, -610, -600, -590, -300, -30, 0, 17)                  # log2 of the magnitudes of p0, q0, p2, q2
N_RANDOM = 10 ** 6


def hi32(x):
    """the high words of doubles, read as binary32"""
    return (np.ascontiguousarray(x, np.float64).view(np.uint64) >> np.uint64(32)).astype(np.uint32).view(np.float32)


def fma_exact(a, b, c):
    """fl(a * b + c) with one rounding, element by element (finite operands; float(Fraction) rounds to nearest even)"""
    out = np.empty(len(a), np.float64)
    for i, (x, y, z) in enumerate(zip(a.tolist(), b.tolist(), c.tolist())):
        out[i] = float(Fraction(x) * Fraction(y) + Fraction(z))
    return out


def fma_fast(a, b, c):
    """fl(a * b + c) for whole arrays (Boldo and Melquiond's emulation): Dekker's exact product a b = h + l, two error-free sums,
    the two small terms added with rounding to odd, one final addition.  Valid while no partial product underflows (checked);
    a product that vanishes beside c == 0 gives 0; everything else goes through the exact path."""
    a, b, c = (np.ascontiguousarray(v, np.float64) for v in (a, b, c))
    lo, hi = 2.0 ** -900, 2.0 ** 900
    with np.errstate(all="ignore"):
        h = a * b
        ok = (np.abs(h) > lo) & (np.abs(h) < hi) & (np.abs(a) > 2.0 ** -960) & (np.abs(a) < hi) & (np.abs(b) > 2.0 ** -960) & (np.abs(b) < hi) & \
             ((c == 0) | ((np.abs(c) > lo) & (np.abs(c) < hi)))
        nothing = ~ok & (h == 0) & (c == 0) & np.isfinite(a) & np.isfinite(b)
    out = np.zeros(len(a), np.float64)
    rest = np.flatnonzero(~ok & ~nothing)
    if np.isfinite(a[rest]).all() and np.isfinite(b[rest]).all() and np.isfinite(c[rest]).all():
        out[rest] = fma_exact(a[rest], b[rest], c[rest])
    else:                                                                   # non-finite operands: the value class is all that matters
        with np.errstate(all="ignore"):
            out[rest] = a[rest] * b[rest] + c[rest]
    idx = np.flatnonzero(ok)
    x, y, z = a[idx], b[idx], c[idx]
    split = 134217729.0                                                     # 2^27 + 1

    def two_sum(u, w):
        t = u + w
        bb = t - u
        return t, (u - (t - bb)) + (w - bb)
    with np.errstate(all="ignore"):
        hh = x * y
        t = split * x
        xh = t - (t - x)
        xl = x - xh
        t = split * y
        yh = t - (t - y)
        yl = y - yh
        ll = ((xh * yh - hh) + xh * yl + xl * yh) + xl * yl                 # hh + ll == x y exactly
        s, err = two_sum(hh, z)
        th, tl = two_sum(ll, s)
        v, verr = two_sum(tl, err)
        # v rounded to odd: where the sum was inexact and v came out even, step one ulp towards the lost part
        bits = v.view(np.int64).copy()
        fix = (verr != 0) & ((bits & 1) == 0)
        away = fix & ((verr > 0) == (v > 0)) & (v != 0)
        bits = np.where(away, bits + 1, np.where(fix & (v != 0), bits - 1, bits))
        r = th + bits.view(np.float64)
    out[idx] = r
    return out


def parent_rows(p0, q0, p2, q2):
    """the replaced per-row condition; also returns c2 and d"""
    with np.errstate(all="ignore"):
        c2 = p2 * q0
    d = fma_fast(p0, q2, -c2)
    with np.errstate(all="ignore"):
        ok = (np.abs(d) > T * np.abs(c2)) & (np.abs(c2) > GUARD)
    return ok, c2, d


def fold_passes(c2, d):
    """the fast path for lanes of four rows: c2, d of shape (n, 4) -> n booleans"""
    n = c2.shape[0]
    e = fma_fast(np.full(4 * n, -T), np.abs(c2).ravel(), np.abs(d).ravel()).reshape(n, 4)
    with np.errstate(all="ignore"):
        he, hc = hi32(e), np.abs(hi32(c2))
        a = np.fmin(np.fmin(he[:, 0], he[:, 1]), he[:, 2])                  # v_min3_f32
        b = np.fmin(np.fmin(hc[:, 0], hc[:, 1]), hc[:, 2])                  # v_min3_f32 with |.| on the c2 operands
        m = np.fmin(np.fmin(a, b), he[:, 3])                                # v_min3_f32
        m = np.fmin(m, hc[:, 3])                                            # v_min_f32
        return m > GUARD_HI, e


def check_implication(p0, q0, p2, q2, what):
    ok, c2, d = parent_rows(p0.ravel(), q0.ravel(), p2.ravel(), q2.ravel())
    ok, c2, d = ok.reshape(-1, 4), c2.reshape(-1, 4), d.reshape(-1, 4)
    fast, _ = fold_passes(c2, d)
    wrong = np.flatnonzero(fast & ~ok.all(axis=1))
    assert len(wrong) == 0, (what, len(wrong), c2[wrong[:3]], d[wrong[:3]])
    return fast, ok


def test_vector_fma_is_the_exact_one():
    rng = np.random.default_rng(3)
    n = 20000
    a = rng.standard_normal(n) * 2.0 ** rng.integers(-300, 18, n)
    b = rng.standard_normal(n) * 2.0 ** rng.integers(-300, 18, n)
    with np.errstate(all="ignore"):
        c = -(a * b) * (1.0 + rng.integers(-3, 4, n) * 2.0 ** -52)          # heavy cancellation, as d = p0 q2 - c2 has
    c[::7] = rng.standard_normal(len(c[::7]))
    assert np.array_equal(fma_fast(a, b, c).view(np.int64), fma_exact(a, b, c).view(np.int64))
    tc = np.abs(a) * T * (1.0 + rng.integers(-2, 3, n) * 2.0 ** -52)
    assert np.array_equal(fma_fast(np.full(n, -T), np.abs(a), tc).view(np.int64), fma_exact(np.full(n, -T), np.abs(a), tc).view(np.int64))


@pytest.mark.parametrize("band", BANDS)
def test_fast_path_implies_the_per_row_condition_on_random_states(band):
    """10^6 quadruples per magnitude band, grouped into lanes of four rows.  Half of them are states near convergence (p2/q2 within a
    few 1e-15 of p0/q0 - where the test decides), the others unrelated values; a fifth of the lanes get one row from another band."""
    rng = np.random.default_rng(1000 + band)
    n = N_RANDOM
    scale = 2.0 ** (band + rng.uniform(-4, 0, n))
    p0 = rng.uniform(0.5, 1.0, n) * scale * rng.choice([-1.0, 1.0], n)
    q0 = rng.uniform(0.5, 1.0, n) * scale * rng.choice([-1.0, 1.0], n)
    p2 = rng.uniform(0.5, 1.0, n) * scale * rng.choice([-1.0, 1.0], n)
    q2 = rng.uniform(0.5, 1.0, n) * scale * rng.choice([-1.0, 1.0], n)
    near = rng.random(n) < 0.5
    g = rng.uniform(0.25, 1.0, n)
    with np.errstate(all="ignore"):
        p2 = np.where(near, p0 * g, p2)
        q2 = np.where(near, q0 * g * (1.0 + rng.uniform(-4e-15, 4e-15, n)), q2)
    lanes = n // 4
    pick = np.flatnonzero(rng.random(lanes) < 0.2)
    mix = pick * 4 + rng.integers(0, 4, len(pick))
    f = 2.0 ** rng.choice([-640.0, -300.0, -20.0, 20.0], len(mix))
    with np.errstate(all="ignore"):
        p0[mix], q0[mix], p2[mix], q2[mix] = p0[mix] * f, q0[mix] * f, p2[mix] * f, q2[mix] * f
    sh = (lanes, 4)
    fast, ok = check_implication(p0[:4 * lanes].reshape(sh), q0[:4 * lanes].reshape(sh), p2[:4 * lanes].reshape(sh), q2[:4 * lanes].reshape(sh), band)
    if band >= -290:                                                        # well above the guard: the test is not vacuous
        assert fast.any() and (~fast).any() and ok.all(axis=1).any()
        # and it is tight: a lane that passes the per-row condition fails the fold only next to a threshold (lanes of this band
        # alone: a row scaled down by 2^-300 has c2 above the guard and e = |d| - T |c2| ~ 1e-15 |c2| below it - a false alarm)
        plain = np.ones(lanes, bool)
        plain[pick] = False
        assert (ok.all(axis=1) & ~fast)[plain].mean() < 1e-3
    if band <= -610:                                                        # c2 ~ 2^(2 band) lies below the guard: never passes
        assert not fast.any()


def _lanes(rows, filler):
    """each adversarial row in each of the four slots of a lane whose other rows pass comfortably"""
    out = []
    for row in rows:
        for slot in range(4):
            lane = [filler] * 4
            lane[slot] = row
            out.append(lane)
    a = np.array(out, np.float64)                                           # (lanes, 4 rows, 4 values)
    return a[:, :, 0], a[:, :, 1], a[:, :, 2], a[:, :, 3]


FILLER = (1.0, 0.75, 0.5, 0.625)                                            # c2 = 0.375, d = 0.25: passes both conditions


def test_zeros_subnormals_and_the_guard():
    tiny, sub = 2.0 ** -1022, 5e-324
    rows = []
    for z in (0.0, -0.0, sub, -sub, 2.0 ** -1040, tiny, -tiny):
        rows += [(z, 1.0, 1.0, 1.0), (1.0, z, 1.0, 1.0), (1.0, 1.0, z, 1.0), (1.0, 1.0, 1.0, z), (z, z, z, z), (1.0, z, z, 1.0), (z, 1.0, 1.0, z)]
    p0, q0, p2, q2 = _lanes(rows, FILLER)
    fast, ok = check_implication(p0, q0, p2, q2, "zeros and subnormals")
    with np.errstate(all="ignore"):
        zero_c2 = (p2 * q0 == 0).any(axis=1)
    assert zero_c2.any() and not fast[zero_c2].any()
    # c2 straddling 2^-600 by one ulp of the high word (2^-20 relative), d far above T |c2|
    g = np.array([GUARD], np.float64).view(np.uint64)[0]
    rows, want = [], []
    for dh in (-2, -1, 0, 1, 2):
        for low in (0, 1, 0xFFFFFFFF):
            c2 = np.array([(int(g) + (dh << 32)) | low], np.uint64).view(np.float64)[0]
            for sgn in (1.0, -1.0):
                rows.append((1.0, 2.0 ** -300, sgn * c2 * 2.0 ** 300, 2.0))  # c2 = p2 q0 exactly, d = 2 - c2
                want.append(dh >= 1)                                         # passes only with a high word ABOVE the guard's
    p0, q0, p2, q2 = _lanes(rows, FILLER)
    fast, ok = check_implication(p0, q0, p2, q2, "guard")
    assert np.array_equal(fast, np.repeat(want, 4))
    assert ok.all(axis=1)[np.repeat([dh > 0 or (dh == 0 and low > 0) for dh in (-2, -1, 0, 1, 2) for low in (0, 1, 0xFFFFFFFF) for _ in (0, 1)], 4)].all()


def _lanes_with_d(c2_list, offsets):
    """(c2, d) of lanes of four rows: a row with the given c2 and d = +-fl(T |c2|) moved by k ulps, in each slot of a lane whose
    other rows pass comfortably.  Both conditions are functions of (c2, d) alone, and a d this close to T |c2| cannot be reached
    through a chosen quadruple (c2 + d needs a hundred bits), so these lanes are given as c2 and d."""
    c2s, ds, ks = [], [], []
    for c2 in c2_list:
        for k in offsets:
            d = T * abs(c2)
            for _ in range(abs(k)):
                d = np.nextafter(d, np.inf if k > 0 else 0.0)
            for sgn in (1.0, -1.0):
                for slot in range(4):
                    lc, ld = [0.375] * 4, [0.25] * 4
                    lc[slot], ld[slot] = c2, sgn * d
                    c2s.append(lc)
                    ds.append(ld)
                    ks.append((c2, d, k))
    return np.array(c2s), np.array(ds), ks


def _conditions(c2, d):
    with np.errstate(all="ignore"):
        ok = (np.abs(d) > T * np.abs(c2)) & (np.abs(c2) > GUARD)
    fast, _ = fold_passes(c2, d)
    assert not (fast & ~ok.all(axis=1)).any()
    return fast, ok.all(axis=1)


def test_d_on_both_sides_of_the_threshold():
    """d one ulp below and above fl(T |c2|): below fails both, above passes both.  And d == fl(T |c2|): the two-rounding compare
    says no; the fold says yes exactly where the product was rounded up, i.e. where |d| > T |c2| in exact arithmetic."""
    rng = np.random.default_rng(8)
    c2_list = [s * m * 2.0 ** e for m in [1.0, 1.25, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52] + list(rng.uniform(1.0, 2.0, 40))
               for e in (-300, -40, 0, 1, 16, 33) for s in (1.0, -1.0)]
    c2, d, meta = _lanes_with_d(c2_list, (-1, 1))
    fast, ok = _conditions(c2, d)
    k = np.array([m[2] for m in meta])
    assert not fast[k < 0].any() and not ok[k < 0].any()
    assert fast[k > 0].all() and ok[k > 0].all()
    # the tie: outside the implication (see the module's docstring)
    c2, d, meta = _lanes_with_d(c2_list, (0,))
    with np.errstate(all="ignore"):
        ok = ((np.abs(d) > T * np.abs(c2)) & (np.abs(c2) > GUARD)).all(axis=1)
    fast, _ = fold_passes(c2, d)
    assert not ok.any()
    exact = np.array([Fraction(m[1]) > Fraction(T) * Fraction(abs(m[0])) for m in meta])
    assert np.array_equal(fast, exact) and exact.any() and (~exact).any()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_what_the_fold_returns_for_nan_and_infinity(bad):
    """A non-finite e or c2 reads as a binary32 NaN and the minimum skips it: with one such row among regular ones the fold PASSES
    (the replaced compare sent that row to the window check).  Only a lane whose eight values are all non-finite fails.  This is the
    statement the kernel's comment has to cover: no infinity arises inside cf_swapped_regular, and a NaN in p or q stays until
    cf_swapped_uniform's final check hands the row back."""
    rows = [(bad, 1.0, 1.0, 1.0), (1.0, bad, 1.0, 1.0), (1.0, 1.0, bad, 1.0), (1.0, 1.0, 1.0, bad), (bad, bad, bad, bad)]
    p0, q0, p2, q2 = _lanes(rows, FILLER)
    okr, c2, d = parent_rows(p0.ravel(), q0.ravel(), p2.ravel(), q2.ravel())
    okr, c2, d = okr.reshape(-1, 4), c2.reshape(-1, 4), d.reshape(-1, 4)
    assert not np.isfinite(d).all(axis=1).any()                             # every lane holds a row with a non-finite d
    fast, e = fold_passes(c2, d)
    hidden = np.isnan(hi32(e)) & (np.isnan(hi32(c2)) | (np.abs(c2) > GUARD))  # rows none of whose two values the minimum sees as a failure
    assert np.array_equal(fast, hidden.any(axis=1))                         # the rest of each lane is the passing filler
    assert fast.any()
    # in a lane that passes, a row for which the replaced condition was false is one the minimum did not see (an infinite d beside a
    # finite c2 passed the replaced compare as well: |inf| > T |c2|)
    assert (okr[fast] | np.isnan(hi32(e[fast]))).all()
    assert (~okr[fast]).any() or not np.isnan(bad)
    # a lane of nothing but non-finite rows: the minimum is NaN, the compare is false
    q = np.full((1, 4), bad)
    okr, c2, d = parent_rows(q.ravel(), q.ravel(), q.ravel(), q.ravel())
    fast, _ = fold_passes(c2.reshape(1, 4), d.reshape(1, 4))
    assert not fast.any()
