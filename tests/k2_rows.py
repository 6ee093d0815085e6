"""Rows for the tests of K2 as a pass runs it (tests/test_gpu_k2_pass.py) and the checks that keep those tests from passing
vacuously (tests/test_k2_pass_inputs.py): numpy restatements of the predicates in fhx_bdtrc.hpp / fhx_k2.hip - IEEE `*`, `-`, `/`
and comparisons only, so every decision is the device's - and seeded generators of (count, prior, binomial) rows.  No GPU here."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# what becomes of a row in k2_classify: dev::BranchClass 0..4, then K2_CLOSED and K2_CLOSED_LOCAL
TRIVIAL, PSERIES, CF_BCF, CF_BD, CF_SWAPPED, CLOSED_POW, CLOSED_LOCAL = range(7)
OUTCOME_NAMES = ("trivial", "pseries", "cf_bcf", "cf_bd", "cf_swapped", "closed_pow", "closed_local")
CLASS_KEYS = ("pseries", "cf_bcf", "cf_bd", "cf_swapped", "closed_pow")        # Context.k2_class_rows / debug_k2_rows
K_MAXGAM = 171.624376956302725
K2_TB_COUNTS = 128
K2H_KCAP = 1023
BOUNDARY_TOTALS = (645040870.0, 7150761687.0, 1.0e6, 5000.0, 170.0, 3.0)
BOUNDARY_COUNTS = (0, 1, 2, 3, 126, 127, 128, 129, 1022, 1023, 1024, 5000)
ROW_COUNTS = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)


class Rows:
    """count, prior and is_inter of some rows under the two totals (as the binomials see them, i.e. already narrowed)"""

    def __init__(self, n_intra, n_inter, count, prior, is_inter):
        self.n_intra, self.n_inter = float(n_intra), float(n_inter)
        self.count = np.ascontiguousarray(count, np.int32)
        self.prior = np.ascontiguousarray(prior, np.float64)
        self.is_inter = np.ascontiguousarray(is_inter, np.uint8)
        assert len(self.count) == len(self.prior) == len(self.is_inter)

    def __len__(self):
        return len(self.count)

    def totals(self):
        return np.where(self.is_inter != 0, self.n_inter, self.n_intra)

    def outcomes(self):
        return outcome(self.count, self.totals(), self.prior)

    def take(self, sel):
        return Rows(self.n_intra, self.n_inter, self.count[sel], self.prior[sel], self.is_inter[sel])

    def shuffled(self, rng):
        return self.take(rng.permutation(len(self)))

    @staticmethod
    def concat(parts):
        assert len({(r.n_intra, r.n_inter) for r in parts}) == 1
        return Rows(parts[0].n_intra, parts[0].n_inter, np.concatenate([r.count for r in parts]),
                    np.concatenate([r.prior for r in parts]), np.concatenate([r.is_inter for r in parts]))


def two_sided(n_intra, rows_intra, n_inter, rows_inter):
    """(count, prior) pairs of the intra binomial and of the inter one in one Rows"""
    ci, pi = rows_intra
    ce, pe = rows_inter
    return Rows(n_intra, n_inter, np.concatenate([ci, ce]), np.concatenate([pi, pe]),
                np.concatenate([np.zeros(len(ci), np.uint8), np.ones(len(ce), np.uint8)]))


# ---- the device's predicates, restated ------------------------------------------------------------------------------------
def bdtrc_class(count, n_total, p):
    """dev::bdtrc_class (== dev::bdtrc_class_tb with tB = aa / (aa + bb)), element-wise"""
    count = np.asarray(count)
    p = np.asarray(p, np.float64)
    n_total = np.broadcast_to(np.asarray(n_total, np.float64), p.shape)
    with np.errstate(all="ignore"):
        fk = count.astype(np.float64) - 1.0
        trivial = np.isnan(p) | (p < 0.0) | (p > 1.0) | (n_total < fk) | (fk < 0) | (fk == n_total) | (count == 1) | (p <= 0.0) | (p >= 1.0)
        aa, bb, xx = fk + 1.0, n_total - fk, p
        ps_direct = (bb * xx <= 1.0) & (xx <= 0.95)
        w = 1.0 - xx
        swapped = xx > aa / (aa + bb)
        ps_swapped = swapped & (aa * w <= 1.0) & (w <= 0.95)
        a, b, x = np.where(swapped, bb, aa), np.where(swapped, aa, bb), np.where(swapped, w, xx)
        y = x * (a + b - 2.0) - (a - 1.0)
        cls = np.where(y < 0.0, np.where(swapped, CF_SWAPPED, CF_BCF), CF_BD)
        cls = np.where(ps_direct | ps_swapped, PSERIES, cls)
        return np.where(trivial, TRIVIAL, cls).astype(np.int32)


def outcome(count, n_total, p):
    """bdtrc_class plus k2_classify's split of the closed form (count == 1, bdtrc_is_closed_form) at prior 0.01"""
    count = np.asarray(count)
    p = np.asarray(p, np.float64)
    n_total = np.broadcast_to(np.asarray(n_total, np.float64), p.shape)
    cls = bdtrc_class(count, n_total, p)
    with np.errstate(invalid="ignore"):
        closed = (count == 1) & (p >= 0.0) & (p <= 1.0) & (n_total > 0.0)
        return np.where(closed, np.where(p < 0.01, CLOSED_LOCAL, CLOSED_POW), cls).astype(np.int32)


def class_rows(outcomes):
    """what fhx_k2_class_rows / the hook report for rows with these outcomes"""
    return {k: int((outcomes == c).sum()) for k, c in zip(CLASS_KEYS, (PSERIES, CF_BCF, CF_BD, CF_SWAPPED, CLOSED_POW))}


def small_n(total):
    """BinomTables::small_n, and whether it makes the pass launch the SMALL_N kernels (plan_k2)"""
    return (total + 1.0) < K_MAXGAM


def plan_small_n(n_intra, n_inter):
    return bool((small_n(n_intra) and n_intra >= 1.0) or (small_n(n_inter) and n_inter >= 1.0))


def handed_back(count, n_total, p):
    """rows k2h_heavy appends to the redo list: swapped class, count below the generic bucket, outside cf_swapped_regular(bb, aa, 1 - p)"""
    count = np.asarray(count)
    p = np.asarray(p, np.float64)
    n_total = np.broadcast_to(np.asarray(n_total, np.float64), p.shape)
    fk = count.astype(np.float64) - 1.0
    aa, bb, w1 = fk + 1.0, n_total - fk, 1.0 - p
    regular = (w1 > 1e-150) & (w1 < 1.0) & (bb >= 1.0) & (bb < 4.5e15) & (aa >= 1.0) & (aa <= bb)
    return (outcome(count, n_total, p) == CF_SWAPPED) & (count < K2H_KCAP) & ~regular


def _cls_pred(which, aa, bb, xx):
    w = 1.0 - xx
    if which == 0:
        return (bb * xx <= 1.0) & (xx <= 0.95)
    if which == 2:
        return (aa * w <= 1.0) & (w <= 0.95)
    if which == 3:
        return w * (bb + aa - 2.0) - (bb - 1.0) < 0.0
    return xx * (aa + bb - 2.0) - (aa - 1.0) < 0.0


def thresholds(n_total, counts):
    """dev::cls_row on the host: tA, tB, tC, tD, tE per count (n x 5), by the same bisection over the bit patterns below 1.0"""
    counts = np.asarray(counts)
    fk = counts.astype(np.float64) - 1.0
    aa, bb = fk + 1.0, float(n_total) - fk
    one = np.int64(0x3FF0000000000000)
    as_f = lambda bits: bits.view(np.float64)

    def largest_true(which):
        lo, hi = np.zeros(len(counts), np.int64), np.full(len(counts), one, np.int64)
        for _ in range(63):
            mid = lo + ((hi - lo) >> 1)
            t = _cls_pred(which, aa, bb, as_f(mid)) & (hi - lo > 1)
            lo, hi = np.where(t, mid, lo), np.where(t | (hi - lo <= 1), hi, mid)
        return np.where(_cls_pred(which, aa, bb, np.zeros(len(counts))), as_f(lo), -1.0)

    def smallest_true(which):
        lo, hi = np.full(len(counts), -1, np.int64), np.full(len(counts), one - 1, np.int64)
        for _ in range(63):
            mid = lo + ((hi - lo) >> 1)
            live = hi - lo > 1
            t = _cls_pred(which, aa, bb, as_f(np.maximum(mid, 0))) & live
            lo, hi = np.where(live & ~t, mid, lo), np.where(t, mid, hi)
        return np.where(_cls_pred(which, aa, bb, as_f(np.full(len(counts), one - 1, np.int64))), as_f(hi), 2.0)

    with np.errstate(all="ignore"):
        return np.stack([largest_true(0), aa / (aa + bb), smallest_true(2), smallest_true(3), largest_true(4)], axis=1)


# ---- generators (seeded: the same rows every time) ---------------------------------------------------------------------------
def _neighbours(v, below, above):
    out, lo, hi = [v], v, v
    for _ in range(below):
        lo = np.nextafter(lo, -1.0)
        out.append(lo)
    for _ in range(above):
        hi = np.nextafter(hi, 2.0)
        out.append(hi)
    return out


def fixture_rows():
    """{total: (count, prior, scipy's value)} of the integer-k rows of f3_bdtrc.npz that the hook accepts (no negative prior)"""
    g = np.load(os.path.join(GOLDEN, "f3_bdtrc.npz"))
    k, n, p, val = g["k"], g["n"], g["p"], g["val"]
    ok = (k == np.floor(k)) & ~(p < 0.0) & (k + 1 >= 0) & (k + 1 <= 2 ** 20)
    return {float(nt): ((k[ok & (n == nt)] + 1).astype(np.int32), p[ok & (n == nt)], val[ok & (n == nt)]) for nt in np.unique(n[ok])}


def boundary_counts(n_total):
    c = set(BOUNDARY_COUNTS)
    for d in (-1, 0, 1):
        if 0 <= n_total + d <= 2 ** 20:
            c.add(int(n_total) + d)
    return np.array(sorted(c), np.int32)


def boundary_rows(n_total, thr=None):
    """(count, prior) around every class boundary of the total: each of the five thresholds of each count with three doubles on
    both sides, the domain edges, 0.95 and 0.05 with neighbours, the closed-form switch 0.01 with its neighbours, NaN.
    thr: the thresholds as the device computed them (debug_classify), default: thresholds() here."""
    counts = boundary_counts(n_total)
    if thr is None:
        thr = thresholds(n_total, counts)
    cs, ps = [], []
    for c, row in zip(counts, thr):
        pri = [0.0, 1.0, 5e-324, 1.0 - 2.0 ** -53, np.nan] + _neighbours(0.95, 1, 1) + _neighbours(0.05, 1, 1) + _neighbours(0.01, 1, 1)
        for t in row:
            if 0.0 <= t <= 1.0:
                pri += [v for v in _neighbours(float(t), 3, 3) if 0.0 <= v <= 1.0]
        cs += [c] * len(pri)
        ps += pri
    return np.array(cs, np.int32), np.array(ps, np.float64)


BOUNDARY_PAIRS = tuple(zip(BOUNDARY_TOTALS, BOUNDARY_TOTALS[2:] + BOUNDARY_TOTALS[:2]))     # (intra, inter): each total once on each side


def boundary_case(n_intra, n_inter, thr_intra=None, thr_inter=None):
    return two_sided(n_intra, boundary_rows(n_intra, thr_intra), n_inter, boundary_rows(n_inter, thr_inter))


SMALL_TOTALS = tuple(range(0, 173))          # 170 is the last total with small_n, 171 and 172 lie behind the switch
LARGE_TOTAL = 1.0e6


def small_total_rows(t, rng):
    """(count, prior) for a total of 0..172 (or the large one): the counts at both ends and in the middle, priors over six decades
    and around count / total"""
    t = int(t)
    counts = np.unique(np.clip([0, 1, 2, 3, t // 3, t // 2, t - 1, t, t + 1], 0, None)).astype(np.int32)
    cs, ps = [], []
    for c in counts:
        around = (c / max(t, 1)) * np.exp(rng.normal(0, 0.7, 3))
        pri = np.concatenate([10.0 ** rng.uniform(-6, 0, 3), np.clip(around, 0.0, 1.0), 1.0 - 10.0 ** rng.uniform(-6, -0.3, 2), [0.005, 0.5]])
        cs += [c] * len(pri)
        ps += list(pri)
    return np.array(cs, np.int32), np.array(ps, np.float64)


def small_total_cases(seed=5):
    """(name, Rows) per total t: small intra | large inter, large intra | small inter, both small (inter = 172 - t)"""
    rng = np.random.default_rng(seed)
    for t in SMALL_TOTALS:
        yield "intra%d" % t, two_sided(float(t), small_total_rows(t, rng), LARGE_TOTAL, pool_rows(LARGE_TOTAL, 48, rng))
        yield "inter%d" % t, two_sided(LARGE_TOTAL, pool_rows(LARGE_TOTAL, 48, rng), float(t), small_total_rows(t, rng))
        yield "both%d" % t, two_sided(float(t), small_total_rows(t, rng), float(172 - t), small_total_rows(172 - t, rng))


def pool_rows(n_total, m, rng, max_count=5000):
    """m (count, prior) pairs that spread over every outcome of a large total: counts geometric with a long tail, priors around
    count / total over several decades, plus tiny ones (power series), large ones (swapped power series), count 1 on both sides of
    0.01 and the constants"""
    cnt = np.minimum(rng.geometric(0.08, m) - 1 + (rng.random(m) < 0.05) * rng.integers(0, max_count, m), max_count).astype(np.int32)
    cnt[rng.random(m) < 0.15] = 1
    ratio = np.exp(rng.normal(0.0, 1.5, m))
    prior = np.clip(np.maximum(cnt, 1) * ratio / n_total, 0.0, 1.0)
    u = rng.random(m)
    prior = np.where(u < 0.15, 10.0 ** rng.uniform(-12, np.log10(1.0 / n_total), m), prior)             # bb * x <= 1
    prior = np.where((u >= 0.15) & (u < 0.25), 1.0 - 10.0 ** rng.uniform(-9, -1, m), prior)                # swapped, near 1
    prior = np.where((u >= 0.25) & (u < 0.32), 10.0 ** rng.uniform(-2.5, -0.5, m), prior)                  # around 0.01 and above
    prior = np.where((u >= 0.32) & (u < 0.34), rng.choice([0.0, 1.0, np.nan], m), prior)
    return cnt, prior


def mixed_rows(m, seed, n_intra=LARGE_TOTAL, n_inter=645040870.0):
    """m shuffled rows of both binomials over all outcomes"""
    rng = np.random.default_rng(seed)
    m_intra = (m + 1) // 2
    return two_sided(n_intra, pool_rows(n_intra, m_intra, rng), n_inter, pool_rows(n_inter, m - m_intra, rng)).shuffled(rng)


def rows_of_outcome(which, m, seed, n_intra=LARGE_TOTAL, n_inter=645040870.0, without=False, keep=None):
    """exactly m shuffled rows with outcome `which` (without = True: m rows of any other outcome); keep: a further filter on Rows"""
    rng = np.random.default_rng(seed)
    got, have = [], 0
    for _ in range(200):
        r = mixed_rows(max(4 * m, 4096), int(rng.integers(1 << 30)), n_intra, n_inter)
        sel = (r.outcomes() == which) != without
        if keep is not None:
            sel &= keep(r)
        got.append(r.take(np.flatnonzero(sel)))
        have += len(got[-1])
        if have >= m:
            return Rows.concat(got).take(np.arange(m))
    raise AssertionError("outcome %s is too rare in the pool" % OUTCOME_NAMES[which])


def heavy_bucket_case(m, seed, count=7, inter=False, filler=1500):
    """m rows of ONE (binomial, count) bucket of the swapped class - the unit k2h_heavy's tasks are cut from - inside a shuffled mix
    of every outcome whose swapped rows avoid that bucket"""
    rng = np.random.default_rng(seed)
    n_intra, n_inter = LARGE_TOTAL, 645040870.0
    total = n_inter if inter else n_intra
    prior = np.clip((count / total) * np.exp(np.abs(rng.normal(0.7, 0.8, m)) + 0.05), 0.0, 0.5)
    bucket = Rows(n_intra, n_inter, np.full(m, count, np.int32), prior, np.full(m, 1 if inter else 0, np.uint8))
    assert (bucket.outcomes() == CF_SWAPPED).all()
    rest = mixed_rows(filler, seed + 1, n_intra, n_inter)
    rest = rest.take(np.flatnonzero(~((rest.count == count) & ((rest.is_inter != 0) == inter) & (rest.outcomes() == CF_SWAPPED))))
    return Rows.concat([bucket, rest]).shuffled(rng)


def sorted_class_case(which, m, seed, filler=1500):
    """a pass whose class `which` (CF_BCF or CF_BD: the k2_queue_by_count kernels, tiles of 1024 entries) holds exactly m rows"""
    rng = np.random.default_rng(seed)
    return Rows.concat([rows_of_outcome(which, m, seed + 1), rows_of_outcome(which, filler, seed + 2, without=True)]).shuffled(rng)


HANDBACK_TOTALS = (100.0, 60.0, 170.0, 171.0, 400.0, 2000.0)


def handback_rows(n_total, rng):
    """(count, prior) of the swapped class that cf_swapped_regular rejects - count > (n + 1) / 2 under a high prior, e.g. n = 100,
    count = 80, prior = 0.9 - selected with the restated predicates"""
    n = int(n_total)
    counts = np.arange(n // 2, min(n, K2H_KCAP - 1) + 1)
    cs = np.repeat(counts, 6).astype(np.int32)
    base = np.clip(cs / n_total, 0.0, 1.0)
    ps = np.clip(base + (1.0 - base) * rng.uniform(0.02, 0.98, len(cs)), 0.0, 1.0)
    sel = handed_back(cs, n_total, ps)
    return cs[sel], ps[sel]


def generic_rows(n_total, m, rng):
    """(count, prior) of the swapped class with counts >= K2H_KCAP: the last bucket of the count sort, evaluated by k2h_generic"""
    cs = rng.integers(K2H_KCAP, 5001, 4 * m).astype(np.int32)
    cs[:3] = (K2H_KCAP, K2H_KCAP + 1, 5000)
    ps = np.clip((cs / n_total) * np.exp(np.abs(rng.normal(0.0, 0.3, len(cs))) + 0.01), 0.0, 0.9)
    sel = np.flatnonzero(outcome(cs, n_total, ps) == CF_SWAPPED)[:m]
    return cs[sel], ps[sel]


def handback_cases(seed=11):
    """(name, Rows, rows predicted to be handed back): the hand-back rows alone (with regular rows of the class around them), the
    generic bucket alone, and both together"""
    rng = np.random.default_rng(seed)
    for n_intra, n_inter in zip(HANDBACK_TOTALS, HANDBACK_TOTALS[1:] + HANDBACK_TOTALS[:1]):
        regular = rows_of_outcome(CF_SWAPPED, 300, int(rng.integers(1 << 30)), n_intra, n_inter, keep=lambda r: ~handed_back(r.count, r.totals(), r.prior))
        back = two_sided(n_intra, handback_rows(n_intra, rng), n_inter, handback_rows(n_inter, rng))
        r = Rows.concat([regular, back]).shuffled(rng)
        yield "handback%d_%d" % (n_intra, n_inter), r, int(handed_back(r.count, r.totals(), r.prior).sum())
    big = two_sided(LARGE_TOTAL, generic_rows(LARGE_TOTAL, 300, rng), 5000.0, generic_rows(5000.0, 300, rng))
    yield "generic", big.shuffled(rng), 0
    # both at once: a total of 2000 holds hand-back rows (count 1001..1022) and generic ones (count >= 1023)
    both = two_sided(2000.0, [np.concatenate(v) for v in zip(handback_rows(2000.0, rng), generic_rows(2000.0, 200, rng))],
                     LARGE_TOTAL, generic_rows(LARGE_TOTAL, 100, rng)).shuffled(rng)
    yield "handback_and_generic", both, int(handed_back(both.count, both.totals(), both.prior).sum())


def top_bins(p):
    """bins of the fused key histogram: bits(p) >> 50 with -0.0 -> 0, over the non-NaN values"""
    p = np.ascontiguousarray(p, np.float64)
    bits = p[~np.isnan(p)].view(np.uint64).copy()
    bits[bits == np.uint64(0x8000000000000000)] = 0
    return np.bincount((bits >> np.uint64(50)).astype(np.int64), minlength=4096)[:4096]
