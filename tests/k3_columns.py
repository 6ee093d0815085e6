"""p columns for K3 as a pass runs it (fhx_bh on the engine's own column), and a numpy model of which path each column takes.

The model restates fhx_k3.hip's decisions without looking at its results: the key of a p-value, the coarse key histogram, the
cutoff bin (k3_cutoff / bin_saturates), the number of rows below it, the threshold of the dense-q path, the sort that number of
survivors selects, the `far_below` guess carried from one fhx_bh to the next, and - per tile of 16 384 rows and for a given number
of tiles per workgroup - which tiles leave their survivors in the LDS strip and which ask for global slots.  tests/test_k3_pass_inputs.py
ties the model to the oracle and checks that the columns reach every branch; tests/test_gpu_k3_pass.py runs them.

Every value a generator writes lies in [0, 1] or is NaN: the engine's pass sorts 62 key bits (bdtrc returns nothing else), so 2.0
or +inf belong to fhx_bh_array and its tests."""
from collections import namedtuple

import numpy as np

TILE = 16384                      # CP_TILE: rows of one k3_compact tile
CHUNK = 1024                      # rows of one wave of a tile (64 lanes x CP_ITEMS)
ITEMS = 16                        # CP_ITEMS
WAVES = TILE // CHUNK
STRIP = 2048                      # CP_STRIP
DENSE_PERCENT = 35                # K3_DENSE_PERCENT
KS_MAX_KEYS = 131072              # the in-LDS tile sorts hold this many survivors
TOP_SHIFT, TOP_BINS = 50, 8192
KEY_KEEP_ALL = 0x7FF0000000000001
SORT_NONE, SORT_TILES, SORT_ONESWEEP, SORT_RADIX = 0, 1, 2, 3

Column = namedtuple("Column", "name p N")


# ---- the model ------------------------------------------------------------------------------------------------------------
def keys(p):
    """bit pattern of p, -0.0 taken as 0 (pvalue_key)"""
    k = np.ascontiguousarray(p, np.float64).view(np.uint64).copy()
    k[k == np.uint64(1 << 63)] = 0
    return k


def cutoff(p, N):
    """(cutoff key, rows below it): the first non-empty bin of key >> 50 with fl(fl(edge * N) / cum) >= 1, cum counting every value
    that is not NaN up to and including the bin; no such bin: every row that is not NaN is kept"""
    p = np.ascontiguousarray(p, np.float64)
    k = keys(p)[~np.isnan(p)]
    hist = np.bincount(np.minimum(k >> np.uint64(TOP_SHIFT), np.uint64(TOP_BINS - 1)).astype(np.int64), minlength=TOP_BINS)
    cum = np.cumsum(hist)
    filled = np.flatnonzero(hist)
    edge = (filled.astype(np.uint64) << np.uint64(TOP_SHIFT)).view(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        v = edge * np.float64(N)                     # rounded once ...
        v = v / cum[filled].astype(np.float64)       # ... and once more
    sat = np.flatnonzero(v >= 1.0)
    if len(sat) == 0:
        return KEY_KEEP_ALL, int(len(k))
    b = int(filled[sat[0]])
    return b << TOP_SHIFT, int(cum[b] - hist[b])


def survivors(p, N):
    """mask of the rows k3_compact keeps: not NaN and key below the cutoff key"""
    p = np.ascontiguousarray(p, np.float64)
    ck, kept = cutoff(p, N)
    m = ~np.isnan(p) & (keys(p) < np.uint64(ck))
    assert int(m.sum()) == kept
    return m


def dense_min(n):
    return (n * DENSE_PERCENT + 99) // 100


def far_below(n, last):
    """last = (rows, survivors) of the context's previous fhx_bh, or None"""
    return last is not None and last[0] == n and last[1] >= 0 and last[1] * 10 < n


def predict(p, N, last=None, prefilled=True, per=0, small_off=False, legacy=False):
    """the eight slots of fhx_k3_pass_info after fhx_bh(N) on column p.  last: what the context's previous fhx_bh saw (far_below);
    prefilled: this is the first fhx_bh behind fhx_pass_stats; per: the forced tiles per workgroup (0: the library's choice, 1 below
    6.7e7 rows); small_off / legacy: FHX_K3_SMALL=0 / FHX_K3_SORT=legacy in the environment"""
    n = len(p)
    kept = cutoff(p, N)[1]
    far = far_below(n, last)
    if kept == 0:
        sort = SORT_NONE
    elif kept <= KS_MAX_KEYS and not small_off:
        sort = SORT_TILES
    else:
        sort = SORT_RADIX if legacy else SORT_ONESWEEP
    return [0 if far else (2 if kept >= dense_min(n) else 1), kept, kept, per or 1, sort, int(far), int(prefilled), 0]


def tile_survivors(mask):
    pad = (-len(mask)) % TILE
    return np.concatenate([mask, np.zeros(pad, bool)]).reshape(-1, TILE).sum(axis=1)


def strip_plan(tile_tot, per):
    """per tile: True = its survivors go to the workgroup's LDS strip, False = it asks for global slots.  A tile joins the strip while
    strip_n + tot <= 2048; the strip empties behind each group of `per` consecutive tiles; per == 1: no strip"""
    plan, strip_n = [], 0
    for t, tot in enumerate(tile_tot):
        if t % per == 0:
            strip_n = 0
        if per > 1 and strip_n + tot <= STRIP:
            plan.append(True)
            strip_n += int(tot)
        else:
            plan.append(False)
    return plan


def strip_fill(tile_tot, per):
    """entries in the strip when each group of tiles writes it out"""
    plan = strip_plan(tile_tot, per)
    return [int(sum(tot for tot, s in zip(tile_tot[g:g + per], plan[g:g + per]) if s)) for g in range(0, len(tile_tot), per)]


# ---- the columns ----------------------------------------------------------------------------------------------------------
def tests_for(n):
    """N of the columns below: above the row count, as on a Hi-C map.  With it no bin of the small values saturates (edge * N / cum <
    1e-9 * 4 n) and the first bin at or above 0.25 does (0.25 * 4 n / cum >= 1): the rows below the cutoff are the small ones"""
    return 4.0 * n


def _small(rng, k):
    return rng.random(k) * 1e-9


def _big(rng, k):
    v = 0.3 + 0.7 * rng.random(k)
    v[rng.random(k) < 0.5] = 1.0
    return v


def _mix(rng, n, k, small=_small):
    """k small values at random rows, the rest in [0.3, 1] (half of them exactly 1.0)"""
    p = _big(rng, n)
    p[rng.choice(n, k, replace=False)] = small(rng, k)
    return p


def sparse(n, seed):
    rng = np.random.default_rng(seed)
    p = np.ones(n)
    k = max(1, round(0.005 * n))
    p[rng.choice(n, k, replace=False)] = _small(rng, k)
    return Column("sparse", p, tests_for(n))


def threshold(n, seed, at):
    """exactly dense_min - 1 (at = -1) or dense_min (at = 0) rows below the cutoff"""
    rng = np.random.default_rng(seed)
    return Column("threshold%+d" % at, _mix(rng, n, dense_min(n) + at), tests_for(n))


def all_survive(n, seed):
    return Column("all_survive", _small(np.random.default_rng(seed), n), tests_for(n))


def nothing_saturates(n, seed):
    """N = 1: every row that is not NaN is ranked, p == 1.0 included"""
    rng = np.random.default_rng(seed)
    p = rng.random(n)
    p[rng.choice(n, n // 20, replace=False)] = 1.0
    p[rng.choice(n, 5, replace=False)] = 0.0
    p[rng.choice(n, 3, replace=False)] = np.nan
    return Column("nothing_saturates", p, 1.0)


def nothing_survives(n, seed):
    return Column("nothing_survives", np.ones(n), tests_for(n))


def nan_ends(n, seed, frac):
    rng = np.random.default_rng(seed)
    p = _mix(rng, n, round(frac * n))
    p[0] = p[n - 1] = np.nan
    return Column("nan_ends_%g" % frac, p, tests_for(n))


def nan_pairs(n, seed, frac, nan_member):
    """pairs (2 j, 2 j + 1) with one member NaN and the other one kept: the first pair, the last whole pair, 300 more"""
    rng = np.random.default_rng(seed)
    p = _mix(rng, n, round(frac * n))
    j = np.unique(np.concatenate([[0, n // 2 - 1], rng.choice(n // 2, 300, replace=False)]))
    p[2 * j + nan_member] = np.nan
    p[2 * j + 1 - nan_member] = _small(rng, len(j))
    return Column("nan_%s_%g" % ("even" if nan_member == 0 else "odd", frac), p, tests_for(n))


def nan_chunk(n, seed, frac):
    """a whole wave chunk of NaN in the middle of a tile, and the column's last (partial) chunk"""
    rng = np.random.default_rng(seed)
    p = _mix(rng, n, round(frac * n))
    p[3 * CHUNK:4 * CHUNK] = np.nan
    p[(n - 1) // CHUNK * CHUNK:] = np.nan
    return Column("nan_chunk_%g" % frac, p, tests_for(n))


def nan_only(n, seed):
    return Column("nan_only", np.full(n, np.nan), tests_for(n))


ZEROS = np.array([0.0, -0.0, 5e-324, 1e-323, 1.5e-323, 2.2250738585072014e-308])


def zeros(n, seed, frac):
    """zeros of both signs, the smallest subnormals and the smallest normal value among ordinary small values"""
    def small(rng, k):
        v = _small(rng, k)
        z = rng.random(k) < 0.7
        v[z] = rng.choice(ZEROS, int(z.sum()))
        return v
    return Column("zeros_%g" % frac, _mix(np.random.default_rng(seed), n, round(frac * n), small), tests_for(n))


def ties(n, seed, frac):
    def small(rng, k):
        return rng.choice(_small(rng, 7), k)
    return Column("ties_%g" % frac, _mix(np.random.default_rng(seed), n, round(frac * n), small), tests_for(n))


def row_in_tile(wave, item, lane):
    """the row of a tile that lane `lane` of wave `wave` holds as item `item` (k3_compact: two consecutive rows per lane and step)"""
    return wave * CHUNK + ((item >> 1) * 64 + lane) * 2 + (item & 1)


CORNERS = [row_in_tile(w, r, l) for w in (0, WAVES - 1) for r in (0, ITEMS - 1) for l in (0, 63)]


def strip_column(name, n, totals, seed):
    """survivors per tile as `totals` says: the corners first (lane 0 and 63, item 0 and 15 of the first and the last wave), the rest at
    random rows of the tile; every other row is 1.0 or lies in [0.3, 1)"""
    rng = np.random.default_rng(seed)
    assert len(totals) == (n + TILE - 1) // TILE
    p = _big(rng, n)
    for t, tot in enumerate(totals):
        rows = min(TILE, n - t * TILE)
        first = [r for r in CORNERS if r < rows][:tot]
        rest = np.setdiff1d(np.arange(rows), first)
        at = np.concatenate([first, rng.choice(rest, tot - len(first), replace=False)]).astype(np.int64)
        p[t * TILE + at] = _small(rng, tot)
    assert sum(totals) < dense_min(n)
    return Column(name, p, tests_for(n))


def strip_columns():
    """built for four tiles per workgroup"""
    return [strip_column("strip_third_does_not_fit", 4 * TILE, [5, 2043, 1, 0], 501),
            strip_column("strip_exactly_full", TILE, [2048], 502),
            strip_column("strip_dense_tile_first", 2 * TILE, [2049, 10], 503),
            strip_column("strip_fourth_does_not_fit", 4 * TILE, [600, 600, 600, 600], 504),
            strip_column("strip_short_last_group", 6 * TILE - 4097, [300, 300, 300, 300, 2000, 49], 505)]


# ---- which column meets which row count --------------------------------------------------------------------------------------
SIZES = [TILE - 1, TILE, TILE + 1, TILE + 1023, TILE + 1024, TILE + 1025, 3 * TILE + 127, 3 * TILE + 129, 5 * TILE - 1, 8 * TILE + 2]
EVERY_SIZE = [("sparse", sparse, {}), ("threshold-1", threshold, {"at": -1}), ("threshold+0", threshold, {"at": 0}),
              ("all_survive", all_survive, {})]
# (each of these meets one odd and one even row count; the fractions put one run on the scattered and one on the dense path)
SOME_SIZES = [("nothing_saturates", nothing_saturates, {}), ("nothing_survives", nothing_survives, {}), ("nan_only", nan_only, {}),
              ("nan_ends", nan_ends, {"frac": 0.05}), ("nan_ends", nan_ends, {"frac": 0.5}),
              ("nan_even", nan_pairs, {"frac": 0.05, "nan_member": 0}), ("nan_even", nan_pairs, {"frac": 0.5, "nan_member": 0}),
              ("nan_odd", nan_pairs, {"frac": 0.05, "nan_member": 1}), ("nan_odd", nan_pairs, {"frac": 0.5, "nan_member": 1}),
              ("nan_chunk", nan_chunk, {"frac": 0.05}), ("nan_chunk", nan_chunk, {"frac": 0.5}),
              ("zeros", zeros, {"frac": 0.05}), ("zeros", zeros, {"frac": 0.4}),
              ("ties", ties, {"frac": 0.2}), ("ties", ties, {"frac": 0.45})]


def size_cases():
    """[(id, n, generator, kwargs)]: the chosen part of sizes x generators"""
    odd = [n for n in SIZES if n & 1]
    even = [n for n in SIZES if not n & 1]
    out = [("%s-%d" % (name, n), n, gen, kw) for n in SIZES for name, gen, kw in EVERY_SIZE]
    for j, (name, gen, kw) in enumerate(SOME_SIZES):
        for n in (odd[j % len(odd)], even[j % len(even)]):
            out.append(("%s%s-%d" % (name, "_%g" % kw["frac"] if "frac" in kw else "", n), n, gen, kw))
    return out


def make(case):
    cid, n, gen, kw = case
    return gen(n, 1000 + SIZES.index(n), **kw)


LARGE_ROWS = 400001


def large_column(n_small, seed):
    """LARGE_ROWS rows, n_small of them below the cutoff"""
    return Column("large_%d" % n_small, _mix(np.random.default_rng(seed), LARGE_ROWS, n_small), tests_for(LARGE_ROWS))


# (survivors, environment, seed): dense + one-sweep with compact indices as payload; scattered + one-sweep; the tile sorts at their
# limit; the count / scan / scatter passes; the radix path forced on a set the tile sorts would take
LARGE_CASES = [(150000, {}, 601), (KS_MAX_KEYS + 1, {}, 602), (KS_MAX_KEYS, {}, 603),
               (KS_MAX_KEYS + 1, {"FHX_K3_SORT": "legacy"}, 604), (KS_MAX_KEYS, {"FHX_K3_SMALL": "0"}, 605)]

FAR_BELOW_ROWS = 3 * TILE + 129


def far_below_sequence():
    """five fhx_bh on one context: sparse, all survive, sparse, all survive, all survive - a different N each time"""
    n = FAR_BELOW_ROWS
    cols = [sparse(n, 701), all_survive(n, 702), sparse(n, 703), all_survive(n, 704), all_survive(n, 705)]
    return [Column(c.name, c.p, c.N * (1.0 + 0.25 * k)) for k, c in enumerate(cols)]
