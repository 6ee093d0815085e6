"""The state a context carries from one pass to the next - the skip byte of every row, the "first duplicated outlier line" limit
(fithic.py:408-412) and the multiset of outlier distances that makeBinsFromInteractions subtracts - modelled on the
oracle, for tests/test_gpu_pass_state.py (which places outliers on purpose by writing the p column) and tests/test_pass_state_model.py
(which ties this model to the oracle and checks that every scenario reaches what it is for).  Plain numpy, imports only `oracle`.

A scenario is fragments, contact rows in file order (and the order in which they are loaded, if that differs), parameters and a
schedule: for each round the rows that get p < thres, the value each of them gets, and the filler of every other row.  The Model
holds the reference's two multisets as Python lists, exactly as fithic.py keeps them, and answers after each round what the device
must hold and what K1 and the bins of the next fit must be."""
import numpy as np

from oracle import fithic_oracle as fo

INT64_MAX = (1 << 63) - 1
RES = 10000
# the kernels' granules the row counts are chosen from
K1_LANE_ROWS, K1_GROUP_ROWS, WAVE, SORT_TILE, SCAN_TILE, K1_LDS_BINS = 4, 512 * 4, 64, 4096, 1024, 6144

FILLERS = ("thres", "one", "half", "nan", "above")          # above = nextafter(thres, 1): the double behind the threshold
OUTLIER_VALUES = ("below", "zero", "negzero", "denormal", "halfthres")
STAT_FIELDS = ("n_rows", "inter_count", "inter_sum", "intra_all_count", "intra_all_sum", "in_range_count", "in_range_sum", "max_count",
               "n_dist", "n_skipped")


def filler_value(kind, thres):
    return {"thres": thres, "one": 1.0, "half": 0.5, "nan": np.nan, "above": np.nextafter(thres, 1.0)}[kind]


def outlier_value(kind, thres):
    return {"below": np.nextafter(thres, 0.0), "zero": 0.0, "negzero": -0.0, "denormal": 5e-324, "halfthres": thres / 2}[kind]


class Round:
    """rows: the outlier rows (file positions, ascending); values: an OUTLIER_VALUES index per outlier row; fillers: a FILLERS index
    per row of the file.  last: nothing runs behind this round's next_pass (the all-outlier round leaves nothing to fit)."""

    def __init__(self, n, rows, rng, fillers=None, values=None, last=False):
        self.rows = np.unique(np.asarray(rows, np.int64))
        assert len(self.rows) == len(rows) and (len(self.rows) == 0 or (0 <= self.rows[0] and self.rows[-1] < n))
        self.values = rng.integers(0, len(OUTLIER_VALUES), len(self.rows)) if values is None else np.asarray(values)
        self.fillers = rng.integers(0, 4, n) if fillers is None else np.asarray(fillers)
        self.last = last

    def p_column(self, thres):
        p = np.array([filler_value(k, thres) for k in FILLERS])[self.fillers]
        p[self.rows] = np.array([outlier_value(k, thres) for k in OUTLIER_VALUES])[self.values]
        return p


class Scenario:
    def __init__(self, name, frags, chr1, mid1, chr2, mid2, count, names, params, schedule, load_order=None):
        self.name, self.frags, self.names, self.params, self.schedule = name, frags, list(names), dict(params), schedule
        self.chr1, self.chr2 = np.asarray(chr1, np.int32), np.asarray(chr2, np.int32)
        self.mid1, self.mid2, self.count = np.asarray(mid1, np.int64), np.asarray(mid2, np.int64), np.asarray(count, np.int64)
        self.load_order = None if load_order is None else np.asarray(load_order, np.int64)     # local row j holds file row load_order[j]
        self.n = len(self.count)
        self.res = self.params["resolution"]
        self.inter = self.chr1 != self.chr2
        self.dist = np.abs(self.mid1 - self.mid2)
        self.fixed = self.res > 0 and all(len(np.unique(np.concatenate([self.mid1[self.chr1 == c], self.mid2[self.chr2 == c]]) % self.res)) <= 1
                                          for c in range(len(self.names)))

    def pairs(self, sel=None):
        sel = slice(None) if sel is None else sel
        return fo.Pairs(self.chr1[sel], self.mid1[sel], self.chr2[sel], self.mid2[sel], self.count[sel], self.names)

    def frag_columns(self):
        """(chr ids, mids, hits, sort rank of the chromosome names) as Context.load_fragments takes them"""
        ids = np.array([self.names.index(f[0]) for f in self.frags], np.int32)
        rank = np.argsort(np.argsort(self.names)).astype(np.int32)
        return ids, np.array([f[1] for f in self.frags], np.int32), np.array([f[2] for f in self.frags], np.int32), rank

    def n_dist(self, sel=None):
        """fixed size: slots of the longest chromosome of the loaded rows + the spare index"""
        sel = slice(None) if sel is None else sel
        return int(max(self.mid1[sel].max(), self.mid2[sel].max()) // self.res) + 2

    def dist_index(self, rows, n_dist):
        """where k_fold_outliers counts an outlier row: the grid distance, rounded UP for an inter-chromosomal row (bins end on grid
        distances, so the next grid distance lies in the bin of the true one), clamped to the spare index"""
        d = self.dist[rows]
        return np.minimum(np.where(self.inter[rows], -(-d // self.res), d // self.res), n_dist - 1)


class Model:
    """sel: the file rows this context holds (default: all) - a shard folds its own outliers and is told the limit"""

    def __init__(self, sc, sel=None):
        self.sc = sc
        self.gidx = np.arange(sc.n) if sel is None else np.asarray(sel, np.int64)
        self.whole = sel is None
        self.outlier_lines, self.outlier_dists = [], []       # the reference's two multisets (never cleared, fithic.py:336-370)
        self.rounds = 0

    def fold(self, rows):
        rows = np.asarray(rows, np.int64)
        rows = rows[np.isin(rows, self.gidx)]
        self.outlier_lines.extend(int(v) for v in rows)
        self.outlier_dists.extend(int(v) for v in self.sc.dist[rows])
        self.rounds += 1

    def total(self):
        return len(self.outlier_lines)

    def skip_bytes(self):
        """one byte per held row: the union of all outlier rows so far"""
        return np.isin(self.gidx, np.asarray(self.outlier_lines, np.int64)).astype(np.uint8)

    def limit(self):
        lines, counts = np.unique(np.asarray(self.outlier_lines, np.int64), return_counts=True)
        return int(lines[counts > 1][0]) if (counts > 1).any() else INT64_MAX

    def dist_hist(self, n_dist):
        return np.bincount(self.sc.dist_index(np.asarray(self.outlier_lines, np.int64), n_dist), minlength=n_dist).astype(np.int64)

    def dists_sorted(self):
        return np.sort(np.asarray(self.outlier_dists, np.int64))

    def skip_mask(self, limit=None):
        if limit is None:
            assert self.whole
            return fo.effective_skip_mask(self.sc.n, self.outlier_lines)          # the reference's walk itself
        return (self.skip_bytes() != 0) & (self.gidx <= limit)

    def next_k1(self, limit=None):
        """what the next pass_stats must return: (stats dict, dist_keys, sumcc, npairs); fixed size: the two histograms are dense
        (index = distance / resolution, length n_dist) and dist_keys is empty"""
        sc, P = self.sc, self.sc.params
        mask = self.skip_mask(limit) if self.rounds else np.zeros(len(self.gidx), bool)
        pairs = sc.pairs(self.gidx)
        keys, sums, icnt, isum, intra_all, rng_sum = fo.read_interactions(pairs, P["L"], P["U"], mask)
        inter, d = sc.inter[self.gidx], sc.dist[self.gidx]
        in_rng = ~mask & ~inter & fo.in_range(d, P["L"], P["U"])
        st = dict(n_rows=len(self.gidx), inter_count=icnt, inter_sum=isum, intra_all_count=int((~mask & ~inter).sum()), intra_all_sum=intra_all,
                  in_range_count=int(in_rng.sum()), in_range_sum=rng_sum, max_count=int(sc.count[self.gidx].max()), n_skipped=int(mask.sum()))
        keys_again, rows_of = np.unique(d[in_rng], return_counts=True)
        assert np.array_equal(keys_again, keys)
        rows_of = rows_of.astype(np.int64)
        self.k1 = (keys, sums, st)
        if not sc.fixed:
            st["n_dist"] = len(keys)
            return st, keys, sums, rows_of
        nd = st["n_dist"] = sc.n_dist(self.gidx)
        cc, npairs = np.zeros(nd, np.int64), np.zeros(nd, np.int64)
        assert (keys % sc.res == 0).all()
        cc[keys // sc.res], npairs[keys // sc.res] = sums, rows_of
        return st, np.zeros(0, np.int64), cc, npairs

    def next_bins(self, outlier_dists=None):
        """the bins of the fit behind the last next_k1(): make_bins with the outlier distances, then the possible pairs ->
        (dict of lb, ub, s2, s1, s7 arrays, bins, frag).  outlier_dists: another encoding of the multiset (the histogram's)"""
        sc, P = self.sc, self.sc.params
        keys, sums, st = self.k1
        od = self.outlier_dists if outlier_dists is None else outlier_dists
        bins = fo.make_bins(keys, sums, P["n_bins"], st["in_range_sum"], od if self.rounds else None)
        if sc.res:
            frag = fo.generate_frag_pairs(sc.frags, bins, sc.res, P["L"], P["U"], P["mapp_thres"], st["inter_count"])
        else:
            frag = fo.generate_frag_pairs_nonfixed(sc.frags, bins, P["L"], P["U"], P["mapp_thres"], st["inter_count"])
        return {k: np.array([b[k] for b in bins], np.int64) for k in ("lb", "ub", "s2", "s1", "s7")}, bins, frag

    def n_tests(self, frag):
        st, mode = self.k1[2], self.sc.params["mode"]
        return {fo.ALL: frag["poss_in_range"] + st["inter_count"], fo.INTER_ONLY: st["inter_count"], fo.INTRA_ONLY: frag["poss_in_range"]}[mode]

    def fit(self, bins, frag):
        """the rest of the oracle's pass on these bins: raises what the reference raises when its spline stage exits"""
        keys, _, st = self.k1
        P = self.sc.params
        x, y, _ = fo.calculate_probabilities(bins, st["in_range_sum"])
        ones = np.ones(len(self.gidx))
        return fo.fit_spline(self.sc.pairs(self.gidx), keys, x, y, ones, ones, P["mode"], P["L"], P["U"], 0.5, 2.0,
                             (st["inter_count"], st["inter_sum"], st["intra_all_sum"], st["in_range_sum"]), frag)


def sum_stats(parts):
    return {k: (max if k in ("max_count", "n_dist") else sum)(p[k] for p in parts) for k in STAT_FIELDS}


# ---- rows -----------------------------------------------------------------------------------------------------------------
FIXED_CHROMS = (("chr1", 300, 5000), ("chr2", 220, 2500), ("chr3", 100, 5000))       # name, loci, offset of the midpoints in their bins


def _grid_frags(chroms, res):
    return [(name, k * res + off, 1) for name, n_loci, off in chroms for k in range(n_loci)]


def _grid_rows(rng, n, chroms, res, special, max_bins, scale=300.0):
    """n rows on the chromosomes' grids: `special` first, then a shuffled mix of intra rows whose counts fall with the distance
    (about 1 / d of them at distance d, so the far bins are thin but not empty) and 10 % inter-chromosomal rows"""
    rows = list(special)
    weights = np.array([c[1] for c in chroms], np.float64)
    while len(rows) < n:
        if rng.random() < 0.1 and len(chroms) > 1:
            a, b = rng.choice(len(chroms), 2, replace=False)
            rows.append((a, int(rng.integers(chroms[a][1])), b, int(rng.integers(chroms[b][1])), 1 + int(rng.poisson(0.8))))
            continue
        c = int(rng.choice(len(chroms), p=weights / weights.sum()))
        top = min(max_bins, chroms[c][1] - 1)
        d = 0 if rng.random() < 0.01 else int(np.exp(rng.uniform(0.0, np.log(top + 1))))
        d = min(max(d, 0), top)
        i = int(rng.integers(chroms[c][1] - d))
        rows.append((c, i, c, i + d, 1 + int(rng.poisson(scale / (1.0 + d) ** 1.1 * rng.lognormal(0, 0.3)))))
    rows = np.array(rows[:n], np.int64)
    off = np.array([c[2] for c in chroms], np.int64)
    return rows[:, 0], rows[:, 1] * res + off[rows[:, 0]], rows[:, 2], rows[:, 3] * res + off[rows[:, 2]], rows[:, 4]


# the first rows of the narrow pool: both halves of an interleaved split reach the last slot of the longest chromosome (one
# histogram length on every context); first bin of chr2 x last bin of chr1: the largest index an outlier can have, the spare one;
# equal midpoints on two chromosomes: distance 0; the same far pair once more, so that both halves hold a clamped row
NARROW_SPECIAL = ((0, 0, 0, 299, 1), (0, 1, 0, 299, 1), (1, 0, 0, 299, 2), (0, 4, 2, 4, 1), (0, 299, 1, 0, 1), (2, 7, 0, 7, 3))
ROW_CLAMPED, ROW_ZERO_DIST = 2, 3
NARROW_PARAMS = dict(resolution=RES, L=RES, U=280 * RES, n_bins=12, mode=fo.ALL, mapp_thres=1)
_POOL = {}


def narrow_rows(n):
    """the first n rows of one pool: every narrow scenario shares its rows"""
    if "narrow" not in _POOL:
        _POOL["narrow"] = _grid_rows(np.random.default_rng(4104), 4104, FIXED_CHROMS, RES, NARROW_SPECIAL, 290)
    return [v[:n] for v in _POOL["narrow"]]


def _scenario(name, rows, schedule, params=NARROW_PARAMS, chroms=FIXED_CHROMS, frags=None, load_order=None):
    c1, m1, c2, m2, cnt = rows
    return Scenario(name, _grid_frags(chroms, params["resolution"]) if frags is None else frags, c1, m1, c2, m2, cnt, [c[0] for c in chroms], params,
                    schedule, load_order)


def _spread(rng, n, k, avoid=()):
    """k rows of the file that are none of `avoid`"""
    free = np.setdiff1d(np.arange(n), np.asarray(list(avoid), np.int64))
    return [int(v) for v in rng.choice(free, k, replace=False)]


def descending_limit_schedule(n, targets, rng, extra=12, also=()):
    """round 1 flags every target (and some rows around); each later round repeats ONE target, from the last to the first: the limit
    lands on each of them in turn, always with flagged rows behind it - in its own group of four and in later groups"""
    targets = sorted(set(int(t) for t in targets))
    others = list(also) + _spread(rng, n, extra, targets + list(also))
    rounds = [Round(n, targets + others, rng)]
    for t in reversed(targets):
        rounds.append(Round(n, [t] + _spread(rng, n, 1, targets + others), rng))
        others += [int(v) for v in rounds[-1].rows if v != t]
    return rounds


def alignment_targets(n):
    """the four positions of a 16-byte row group in K1's first and in its second workgroup, and every tail row (n & 3 of them)"""
    k0, k1 = 100, K1_GROUP_ROWS // 4 + 88
    return [4 * k0 + j for j in range(4)] + [4 * k1 + j for j in range(4)] + list(range(n - (n & 3), n))


def narrow_scenarios():
    """a. n = 4101..4104 (three rows in the tail, two, one, none)"""
    for n in (4101, 4102, 4103, 4104):
        rng = np.random.default_rng(n)
        yield _scenario("narrow%d" % n, narrow_rows(n), descending_limit_schedule(n, alignment_targets(n), rng, also=(ROW_CLAMPED, ROW_ZERO_DIST)))


def lone_limit_scenarios():
    """a. the limit with no skip flag before or behind it: one row, twice - at each residue and in the tail"""
    n = 4103
    for t in (1200, 1201, 2402, 2403, 4100, 4102):
        rng = np.random.default_rng(t)
        yield _scenario("lone%d" % t, narrow_rows(n), [Round(n, [t], rng), Round(n, [t], rng)])


WIDE_CHROMS = (("chr1", 7000, 5000),)
WIDE_PARAMS = dict(resolution=RES, L=RES, U=float("inf"), n_bins=10, mode=fo.INTRA_ONLY, mapp_thres=1)


def wide_scenario():
    """b. one chromosome of 7000 bins, no upper bound: the window K1 must cover has more than 6144 bins"""
    n = 4103
    if "wide" not in _POOL:
        _POOL["wide"] = _grid_rows(np.random.default_rng(7000), n, WIDE_CHROMS, RES, ((0, 0, 0, 6999, 1), (0, 1, 0, 6999, 1)), 6999, scale=3000.0)
    rng = np.random.default_rng(7001)
    return _scenario("wide", _POOL["wide"], descending_limit_schedule(n, alignment_targets(n), rng), WIDE_PARAMS, WIDE_CHROMS)


def permuted_scenario():
    """c. the rows of (a) loaded in a shuffled order: the limit is a file position.  The last loaded rows - K1's tail - are rows from
    the head of the file, flagged, in front of a limit that lies far below their local positions; rows from the end of the file
    are loaded first"""
    n = 4103
    rng = np.random.default_rng(31)
    order = rng.permutation(n)
    for local, row in ((n - 1, 7), (n - 2, 9), (n - 3, 4000), (0, 4090), (1, 11)):
        j = int(np.flatnonzero(order == row)[0])
        order[j], order[local] = order[local], order[j]
    base = [7, 9, 11, 4000, 4090, 500, 501, 502, 503, 2000, 2600, ROW_CLAMPED, ROW_ZERO_DIST]
    sched = [Round(n, base + _spread(rng, n, 6, base), rng)]
    for t in (2600, 503, 502, 501, 500, 9):
        sched.append(Round(n, [t], rng))
    return _scenario("permuted", narrow_rows(n), sched, load_order=order)


def split_scenario():
    """c. the same rows on two contexts, every third row on the second one; the schedule of (e)"""
    sc = five_round_scenario()
    sc.name = "split"
    sc.parts = [np.flatnonzero(np.arange(sc.n) % 3 != 2), np.flatnonzero(np.arange(sc.n) % 3 == 2)]
    return sc


FIVE_T, FIVE_Z, FIVE_ABOVE, FIVE_LOW = 3000, 2000, 3500, 700


def five_round_scenario():
    """e. round 1 flags T, Z, ABOVE, LOW and others; round 2 repeats T and Z (limit = Z); round 3 is empty; round 4 repeats T - a
    third time - and nothing else that was seen: its only duplicate lies above the limit, which stays; round 5 repeats LOW: down"""
    n = 4103
    rng = np.random.default_rng(5)
    base = [FIVE_T, FIVE_Z, FIVE_ABOVE, FIVE_LOW, ROW_CLAMPED, ROW_ZERO_DIST]
    first = base + _spread(rng, n, 10, base)
    r2 = [FIVE_T, FIVE_Z] + _spread(rng, n, 3, first)
    r4 = [FIVE_T] + _spread(rng, n, 3, first + r2)
    r5 = [FIVE_LOW] + _spread(rng, n, 2, first + r2 + r4)
    return _scenario("five", narrow_rows(n), [Round(n, first, rng), Round(n, r2, rng), Round(n, [], rng), Round(n, r4, rng), Round(n, r5, rng)])


THRESHOLD_ROWS = dict(thres=40, below=41, above=42, nan=43, zero=44, negzero=45, denormal=46)


def threshold_scenario():
    """f. one round whose p column holds, at known rows, thres, the doubles on both sides of it, NaN, both zeros and the smallest
    denormal; the inter row on the spare index and the inter row at distance 0 are outliers too"""
    n = 4101
    rng = np.random.default_rng(6)
    T = THRESHOLD_ROWS
    rows = sorted([T["below"], T["zero"], T["negzero"], T["denormal"], ROW_CLAMPED, ROW_ZERO_DIST])
    values = {T["below"]: 0, T["zero"]: 1, T["negzero"]: 2, T["denormal"]: 3, ROW_CLAMPED: 4, ROW_ZERO_DIST: 0}
    fillers = rng.integers(0, 4, n)
    fillers[T["thres"]], fillers[T["above"]], fillers[T["nan"]] = FILLERS.index("thres"), FILLERS.index("above"), FILLERS.index("nan")
    return _scenario("threshold", narrow_rows(n), [Round(n, rows, rng, fillers, [values[r] for r in rows])])


def fetch_scenarios():
    """g. row counts around the 1024-row scan tile of fetch_outlier_rows: outliers on the tile's edges, none at all, every row"""
    for n in (1023, 1024, 1025, 2049):
        rng = np.random.default_rng(n)
        edge = [r for r in (0, 1023, 1024, n - 1) if r < n]
        yield _scenario("fetch%d" % n, narrow_rows(n), [Round(n, sorted(set(edge)), rng), Round(n, [], rng), Round(n, list(range(n)), rng, last=True)])


# ---- irregular midpoints: -r 0, and -r N on loci that share no grid ---------------------------------------------------------
IRREGULAR_CHROMS = (("c0", 260), ("c1", 200))
OFFGRID_RES = 1000                  # the midpoints are multiples of 500: no chromosome's share one offset in bins of 1000


def _irregular_pool():
    if "irregular" not in _POOL:
        rng = np.random.default_rng(8193)
        mids = [np.cumsum(rng.integers(6, 60, n_loci)) * 500 for _, n_loci in IRREGULAR_CHROMS]       # multiples of 500: distances repeat
        frags = [(name, int(m), 1) for (name, _), mm in zip(IRREGULAR_CHROMS, mids) for m in mm]
        rows = []
        while len(rows) < 8193:
            if rng.random() < 0.1:
                rows.append((0, int(rng.choice(mids[0])), 1, int(rng.choice(mids[1])), 1 + int(rng.poisson(0.8))))
                continue
            c = int(rng.random() < 0.43)
            i = int(rng.integers(len(mids[c]) - 1))
            j = min(len(mids[c]) - 1, i + 1 + int(np.exp(rng.uniform(0.0, np.log(60.0))) - 1))
            d = (mids[c][j] - mids[c][i]) / RES
            rows.append((c, int(mids[c][i]), c, int(mids[c][j]), 1 + int(rng.poisson(200.0 / (1.0 + d) ** 1.1 * rng.lognormal(0, 0.3)))))
        _POOL["irregular"] = (frags, [np.array(v, np.int64) for v in zip(*rows)])
    return _POOL["irregular"]


def irregular_scenarios():
    """d. n around the 4096-row tile of nf_k1_classify, twice that and one; outliers on a wave edge (63, 64), on the tile edge (4095,
    4096) and on the last row; inter-chromosomal ones; rows of equal distance.  Round 1 flags them all (pass 2 skips them all),
    round 2 repeats the last row, round 3 the row at the tile edge: the list of distances grows over three passes."""
    frags, pool = _irregular_pool()
    for res in (0, OFFGRID_RES):
        for n in (4095, 4096, 4097, 8193):
            rng = np.random.default_rng(n + res)
            rows = [v[:n] for v in pool]
            dist, inter = np.abs(rows[1] - rows[3]), rows[0] != rows[2]
            edge = sorted(set(r for r in (63, 64, 4095, 4096, n - 1) if r < n))
            free = np.setdiff1d(np.arange(n), edge)
            inter_rows = [int(v) for v in free[inter[free]][:3]]
            vals, counts = np.unique(dist[free[~inter[free]]], return_counts=True)
            twin = [int(v) for v in free[~inter[free] & (dist[free] == vals[counts > 1][0])][:2]]
            first = sorted(set(edge + inter_rows + twin))
            tile_row = max(r for r in edge if r <= 4096 and r != n - 1) if n > 4096 else 64
            sched = [Round(n, first + _spread(rng, n, 4, first), rng)]
            sched.append(Round(n, [n - 1] + [int(v) for v in free[inter[free]][3:5]], rng))
            sched.append(Round(n, [tile_row], rng))
            params = dict(resolution=res, L=20000, U=float("inf") if res == 0 else 200 * res, n_bins=6, mode=fo.ALL, mapp_thres=1)
            yield _scenario("%s%d" % ("nonfixed" if res == 0 else "offgrid", n), rows, sched, params, IRREGULAR_CHROMS, frags)


def all_scenarios():
    yield from narrow_scenarios()
    yield from lone_limit_scenarios()
    yield wide_scenario()
    yield permuted_scenario()
    yield five_round_scenario()
    yield threshold_scenario()
    yield from fetch_scenarios()
    yield from irregular_scenarios()
