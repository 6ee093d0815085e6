"""Tables for the tests of k1_classify_hist's distance window (tests/test_gpu_k1_windows.py) and the checks that keep those
tests from passing vacuously (tests/test_k1_window_inputs.py).  No GPU here.  Three things:

1. numpy_k1: the count every K1 test holds the device to (tests/test_gpu_k1_keys.py imports it from here).  int64 throughout,
   np.add.at on the distances, nothing else.
2. a model of which workgroup meets which row - launch_k1's grid and the kernel's loop restated (launch, workgroup_of_rows) - and
   per_workgroup(): per (workgroup, window bin, path) the rows and the sum of counts that workgroup adds.  It only proves that a
   case reaches its seam; nothing on the device is compared with it.
3. the cases.  The 24 576-bin instantiation (more than 6144 distance values in the window) keeps a bin in LDS as a u32 sum - a
   wrap adds 2^32 to the bin in HBM - and a 15-bit row count with a guard bit, two bins to a word - the add that sets the guard
   bit moves 2^15 rows to HBM.  Window bins from 24 576 on and rows with a negative count take the HBM atomics.

   small_cases(): one chromosome at resolution 1, an inter row reaching locus 24 900 so that the window is wide, one workgroup.
   Every bin's rows start a group of four rows, which one lane takes in order: "BIG, BIG, then 2" is the order of the adds.
     A1 BIG, BIG: 2^32 - 2, no wrap            A2 BIG, BIG, 2: exactly 2^32, residue 0        A3 BIG, BIG, 3: one wrap, residue 1
     A4 eleven BIG: five wraps                  A5 BIG, BIG, then an inline 8191: the wrap comes from a keyed row
     A6-1 .. A6-4  A1 .. A4 on window bins 0, 24 575 (the last in LDS), 24 576 and 24 577 (HBM)
     A8 8 211 rows, three workgroups: bins whose residues sit in several workgroups, one of which wraps
     A9 a row with count -1 (fhx_load_pairs takes it, as the reference's int(float(text)) does): it goes past the packed window
   each once with -L 0 and once with -L 7 (A7: lo_idx odd - the half-word of a bin follows b = d - lo_idx, its HBM address d).

   large_table(): 256 * 4096 * 17 + 3 rows, every one of the 256 workgroups meets 69 632 of them; -L 1, so b and d differ in
   parity here too.  Counts are 1 and 2, except three rows of BIG in workgroups 9 - 11: with inline counts alone the sum of
   bin H could not pass 2^32 over all workgroups, which the table is asked to do (in no single workgroup).  LARGE_TARGETS
   lists what the workgroups 0 .. 8 and 64, 65, 255 get; the others get 300 rows over window bins 0 .. 24 700, among them 0,
   24 575, 24 576 and 24 700 in every one.  Everything else is filler: d = 0 (below -L) and inter rows, alternating.

   switch_cases(): N1 / N2, 9 003 rows on a chromosome of 7 000 loci with a window of 6144 (narrow kernel, five workgroups) and
   of 6145 bins (the 24 576-bin kernel), rows on lo - 1, lo, hi, hi + 1 of both and on every hundredth bin between."""
import functools

import numpy as np

STAT_FIELDS = ("n_rows", "inter_count", "inter_sum", "intra_all_count", "intra_all_sum", "in_range_count", "in_range_sum", "max_count",
               "n_dist", "n_skipped")
BIG = 2 ** 31 - 1
WRAP = 2 ** 32

# fhx_k1.hip: K1_THREADS / K1_LDS_BINS, K1_WIDE_THREADS / K1_WIDE_BINS, the grid caps of launch_k1, the flush's rotation
K1_THREADS, K1_CAP, K1_LDS_BINS = 512, 512, 6144
K1_WIDE_THREADS, K1_WIDE_CAP, K1_WIDE_BINS = 1024, 256, 24576
K1_ROT = 389
GUARD = 1 << 15


# ---- 1. the reference ------------------------------------------------------------------------------------------------------
def numpy_k1(rows, res, low, up):
    """rows: (chr1, idx1, chr2, idx2, count) with idx = the locus' bin on its chromosome -> (stats dict, sumCC, rows per distance)"""
    c1, i1, c2, i2, cnt = (np.asarray(v, np.int64) for v in rows)
    n_dist = int(max(i1.max(), i2.max())) + 2                # slots of the longest chromosome + the spare index
    inter = c1 != c2
    d = np.abs(i1 - i2)
    lo = -(-low // res)
    hi = n_dist - 1 if up is None else min(up // res, n_dist - 1)
    rng = ~inter & (d >= lo) & (d <= hi)
    st = dict(n_rows=len(cnt), inter_count=int(inter.sum()), inter_sum=int(cnt[inter].sum()), intra_all_count=int((~inter).sum()),
              intra_all_sum=int(cnt[~inter].sum()), in_range_count=int(rng.sum()), in_range_sum=int(cnt[rng].sum()),
              max_count=max(0, int(cnt.max())), n_dist=n_dist, n_skipped=0)       # the kernel's maximum starts at 0
    cc, npairs = np.zeros(n_dist, np.int64), np.zeros(n_dist, np.int64)
    np.add.at(cc, d[rng], cnt[rng])
    np.add.at(npairs, d[rng], 1)
    return st, cc, npairs


# ---- 2. which workgroup meets which row ------------------------------------------------------------------------------------
class Case:
    """a table (chr1, idx1, chr2, idx2, count), loci at resolution `res` with midpoint offset 0, and the run's -L / -U"""

    def __init__(self, name, rows, res, low, up):
        self.name, self.res, self.low, self.up = name, res, low, up
        self.rows = tuple(np.ascontiguousarray(v) for v in rows)
        assert len({len(v) for v in self.rows}) == 1

    def __len__(self):
        return len(self.rows[0])

    def __repr__(self):
        return "Case(%s)" % self.name

    def mids(self):
        """the five columns as Context.load_pairs takes them"""
        c1, i1, c2, i2, cnt = self.rows
        return (c1, i1, c2, i2, cnt) if self.res == 1 else (c1, i1 * self.res, c2, i2 * self.res, cnt)


class Launch:
    """launch_k1 restated: the window [lo, hi] in slots, which instantiation, how many workgroups"""

    def __init__(self, n, n_dist, res, low, up):
        self.n, self.n_dist = n, n_dist
        self.lo = -(-low // res)
        self.hi = n_dist - 1 if up is None else min(up // res, n_dist - 1)
        self.width = self.hi - self.lo + 1
        self.wide = self.width > K1_LDS_BINS
        self.threads, cap, self.bins = (K1_WIDE_THREADS, K1_WIDE_CAP, K1_WIDE_BINS) if self.wide else (K1_THREADS, K1_CAP, K1_LDS_BINS)
        groups = -(-n // 4)
        self.blocks = max(1, min(cap, -(-groups // self.threads)))

    def rotation(self, block):
        """the flush of workgroup `block` starts at this bin; (the product before the %, the start)"""
        return block * K1_ROT, (block * K1_ROT) % self.bins


def launch(case):
    c1, i1, c2, i2, cnt = case.rows
    return Launch(len(cnt), int(max(i1.max(), i2.max())) + 2, case.res, case.low, case.up)


def workgroup_of_rows(n, blocks, threads):
    """rows 4g .. 4g + 3 are one lane's step: lane g mod (blocks * threads) of the grid; the n & 3 tail rows go to workgroup 0"""
    g = np.arange(n, dtype=np.int64) >> 2
    wg = ((g % (blocks * threads)) // threads).astype(np.int16)
    wg[(n >> 2) << 2:] = 0
    return wg


class PerWorkgroup:
    """entries (workgroup, window bin b, path): `lds` says the rows went into the workgroup's LDS window, else straight to HBM"""

    def __init__(self, launch_, wg, b, lds, rows, sums):
        self.launch, self.wg, self.b, self.lds, self.rows, self.sum = launch_, wg, b, lds, rows, sums

    def at(self, wg, b, lds=True):
        """(rows, sum of counts) workgroup `wg` adds to bin `b` on that path"""
        k = np.flatnonzero((self.wg == wg) & (self.b == b) & (self.lds == lds))
        return (int(self.rows[k[0]]), int(self.sum[k[0]])) if len(k) else (0, 0)

    def workgroups(self, b, lds=True):
        return sorted(set(self.wg[(self.b == b) & (self.lds == lds)].tolist()))

    def bins(self):
        return sorted(set(self.b.tolist()))

    def total(self, b):
        sel = self.b == b
        return int(self.rows[sel].sum()), int(self.sum[sel].sum())


def per_workgroup(case):
    L = launch(case)
    c1, i1, c2, i2, cnt = case.rows
    wg = workgroup_of_rows(L.n, L.blocks, L.threads)
    d = np.abs(i1.astype(np.int64) - i2)
    sel = np.flatnonzero((c1 == c2) & (d >= L.lo) & (d <= L.hi))
    b, c, w = d[sel] - L.lo, cnt[sel].astype(np.int64), wg[sel].astype(np.int64)
    lds = (b < L.bins) & ((c >= 0) | (not L.wide))          # one(): WIDE && b < BINS && c >= 0, !WIDE && b < BINS
    key = (w * L.width + b) * 2 + lds
    uk, inv = np.unique(key, return_inverse=True)
    rows, sums = np.zeros(len(uk), np.int64), np.zeros(len(uk), np.int64)
    np.add.at(rows, inv, 1)
    np.add.at(sums, inv, c)
    return PerWorkgroup(L, uk // 2 // L.width, uk // 2 % L.width, (uk & 1).astype(bool), rows, sums)


# ---- 3. the cases ------------------------------------------------------------------------------------------------------------
FAR = 24900                                   # locus of the inter row that makes chromosome 0 long enough for a wide window
SCENARIOS = {"A1": (BIG, BIG), "A2": (BIG, BIG, 2), "A3": (BIG, BIG, 3), "A4": (BIG,) * 11, "A5": (BIG, BIG, 8191)}
SMALL_BIN = {"A1": 100, "A2": 101, "A3": 4098, "A4": 4099, "A5": 12345}     # window bins, both parities
EDGE_BINS = (0, K1_WIDE_BINS - 1, K1_WIDE_BINS, K1_WIDE_BINS + 1)
A8_BINS = dict(no_wrap=100, one_wraps=101, exact=102, five_wraps=103)
A9_BINS = dict(alone=50, shared=51)
LOWS = (0, 7)                                 # -L of the small cases; with 7 lo_idx is odd (A7)


def _table(rows):
    return tuple(np.array(v, np.int64) for v in zip(*rows))


def _group_aligned(rows):
    while len(rows) & 3:
        rows.append((0, 1, 1, 1, 1))              # inter filler up to the next group of four rows


def _base_rows(lo):
    rows = [(0, FAR, 1, 3, 5), (0, 0, 0, lo + 7, 1), (0, 2, 0, lo + 2 + 7, 2), (0, 5, 1, 0, 8192)]
    if lo:
        rows += [(0, 10, 0, 10 + lo - 1, 3), (0, 0, 0, 0, BIG)]      # below -L
    return rows


def _put(rows, b, lo, counts):
    """the rows of window bin b, from a group boundary on: one lane adds them in this order"""
    _group_aligned(rows)
    for k, c in enumerate(counts):
        rows.append((0, k, 0, k + lo + b, c))


def small_case(name, lo):
    tag = "%s-L%d" % (name, lo)
    if name in SCENARIOS:
        rows = _base_rows(lo)
        _put(rows, SMALL_BIN[name], lo, SCENARIOS[name])
        rows.append((0, 3, 0, 3 + lo + 9, 4))                          # a tail
    elif name.startswith("A6-"):
        rows = [(0, FAR, 1, 3, 5), (0, 5, 1, 0, 8192)]               # no other in-range row: the four bins are all that is hit
        for b in EDGE_BINS:
            _put(rows, b, lo, SCENARIOS["A" + name[3:]])
    elif name == "A8":
        return _a8(tag, lo)
    elif name == "A9":
        rows = _base_rows(lo)
        _put(rows, A9_BINS["alone"], lo, (-1,))
        _put(rows, A9_BINS["shared"], lo, (5, -1, 8192))
    else:
        raise KeyError(name)
    return Case(tag, _table(rows), 1, lo, None)


def _a8(tag, lo):
    """8 211 rows: workgroups 0, 1, 2 take rows 0 .. 4095, 4096 .. 8191 and 8192 .. 8207; the three tail rows go to workgroup 0"""
    rng = np.random.default_rng(8)
    n = 8211
    b = rng.integers(200, 20000, size=n)
    cnt = rng.choice((1, 2, 9, 8191, 8192), size=n)
    i1 = rng.integers(0, 50, size=n)
    c2 = np.where(rng.random(n) < 0.3, 1, 0)
    i2 = np.where(c2 == 1, rng.integers(0, 40, size=n), i1 + lo + b)
    c1 = np.zeros(n, np.int64)
    i1[0], c2[0], i2[0], cnt[0] = FAR, 1, 3, 5

    def put(row, bin_, counts):                      # from a group boundary on
        assert row % 4 == 0
        for k, c in enumerate(counts):
            c2[row + k], i1[row + k], i2[row + k], cnt[row + k] = 0, k, k + lo + bin_, c

    W0, W1, W2 = 0, 4096, 8192
    put(W0 + 4, A8_BINS["no_wrap"], (BIG,))                       # 2^32 - 2 over two workgroups, no wrap in either
    put(W1 + 4, A8_BINS["no_wrap"], (BIG,))
    put(W0 + 8, A8_BINS["one_wraps"], (BIG,))                     # residues in three workgroups, workgroup 1 wraps
    put(W1 + 8, A8_BINS["one_wraps"], (BIG, BIG, 3))
    put(W2 + 4, A8_BINS["one_wraps"], (7,))
    put(W0 + 12, A8_BINS["exact"], (1,))                          # workgroup 2 holds exactly 2^32: residue 0 beside two residues
    put(W1 + 12, A8_BINS["exact"], (8191, 8192))
    put(W2 + 8, A8_BINS["exact"], (BIG, BIG, 2))
    put(W0 + 16, A8_BINS["five_wraps"], (BIG,) * 11)              # three lanes of workgroup 0
    put(W1 + 16, A8_BINS["five_wraps"], (BIG,))
    put(W2 + 0, A8_BINS["five_wraps"], (BIG, 1))
    return Case(tag, (c1, i1, c2, i2, cnt), 1, lo, None)


SMALL_NAMES = ("A1", "A2", "A3", "A4", "A5", "A6-1", "A6-2", "A6-3", "A6-4", "A8", "A9")


def small_cases():
    return [small_case(name, lo) for lo in LOWS for name in SMALL_NAMES]


# the large table: rows of window bin H (and of its neighbours) per workgroup
LARGE_N = 256 * 4096 * 17 + 3
LARGE_PER_WG = 4096 * 17
LARGE_LOW = 1
H = 1001                                      # odd: H ^ 1 = H - 1 shares its word, H + 1 lies in the next one
LARGE_H_ROWS = {0: GUARD - 1, 1: GUARD, 2: GUARD + 1, 3: 2 * GUARD - 1, 4: 2 * GUARD, 5: 2 * GUARD + 1, 6: LARGE_PER_WG}
LARGE_PAIRED = {7: H ^ 1, 8: H + 1}           # 34 000 rows on H and 34 000 on this bin, alternating
LARGE_PAIRED_ROWS = 34000
LARGE_LATE = (64, 65, 255)                    # 40 000 rows each on bin 24 575 - blockIdx
LARGE_LATE_ROWS = 40000
LARGE_BIG_WGS = (9, 10, 11)                   # one row of BIG on H each
LARGE_REST_ROWS = 300
LARGE_LAST_BIN = 24700
LARGE_TARGETS = dict(h_rows=LARGE_H_ROWS, paired=LARGE_PAIRED, late=LARGE_LATE)


def late_bin(block):
    return K1_WIDE_BINS - 1 - block


@functools.lru_cache(maxsize=1)
def large_table():
    """-> Case; built once per process (int32 columns: 5 x 71 MB)"""
    n, lo = LARGE_N, LARGE_LOW
    wg = workgroup_of_rows(n, K1_WIDE_CAP, K1_WIDE_THREADS)
    order = np.argsort(wg, kind="stable")                       # a workgroup's rows in the order of its loop
    start = np.concatenate([[0], np.cumsum(np.bincount(wg, minlength=K1_WIDE_CAP))])
    rng = np.random.default_rng(17)
    b = np.full(n, -1, np.int32)                                # -1: filler
    cnt = rng.integers(1, 3, size=n, dtype=np.int32)
    for w in range(K1_WIDE_CAP):
        mine = order[start[w]:start[w + 1]]
        assert len(mine) == LARGE_PER_WG + (3 if w == 0 else 0)
        if w in LARGE_H_ROWS:
            b[mine[:LARGE_H_ROWS[w]]] = H
            continue
        if w in LARGE_PAIRED:
            b[mine[0:2 * LARGE_PAIRED_ROWS:2]] = H
            b[mine[1:2 * LARGE_PAIRED_ROWS:2]] = LARGE_PAIRED[w]
            continue
        taken = 0
        if w in LARGE_LATE:
            b[mine[:LARGE_LATE_ROWS]] = late_bin(w)
            taken = LARGE_LATE_ROWS
        pos = mine[taken + rng.permutation(len(mine) - taken)[:LARGE_REST_ROWS]]
        b[pos] = rng.integers(0, LARGE_LAST_BIN + 1, size=LARGE_REST_ROWS)
        b[pos[:4]] = (0, K1_WIDE_BINS - 1, K1_WIDE_BINS, LARGE_LAST_BIN)
        if w in LARGE_BIG_WGS:
            b[pos[4]], cnt[pos[4]] = H, BIG
    fill = b < 0
    inter = fill & ((np.arange(n) & 1) == 1)
    zeros = np.zeros(n, np.int32)
    i2 = np.where(fill, 0, b + lo).astype(np.int32)             # filler: d = 0 < lo, or the other chromosome's locus 0
    return Case("large", (zeros, zeros, inter.astype(np.int32), i2, cnt), 1, lo, None)


# narrow / wide switch
SWITCH_LOCI, SWITCH_LO, SWITCH_HI = 7000, 300, 300 + K1_LDS_BINS - 1
SWITCH_N = 9003


def switch_bins():
    """distances of the rows: lo - 1, lo, hi, hi + 1 of both windows (N2's hi is N1's hi + 1) and every hundredth bin between"""
    return sorted({SWITCH_LO - 1, SWITCH_LO, SWITCH_HI, SWITCH_HI + 1, SWITCH_HI + 2} | set(range(SWITCH_LO, SWITCH_HI, 100)))


def switch_cases():
    rng = np.random.default_rng(61)
    n = SWITCH_N
    bins = np.array(switch_bins())
    d = bins[rng.integers(len(bins), size=n)]
    d[:len(bins)] = bins                                          # every one at least once, early rows ...
    d[-len(bins):] = bins[::-1]                                   # ... and late ones: first and last workgroup
    i1 = (rng.random(n) * (SWITCH_LOCI - d)).astype(np.int64)
    cnt = rng.choice((1, 2, 5, 8191, 8192, BIG), size=n, p=(.4, .3, .15, .05, .05, .05))
    c1 = np.zeros(n, np.int64)
    c2 = np.where(rng.random(n) < 0.1, 1, 0)
    i2 = np.where(c2 == 1, rng.integers(0, 100, size=n), i1 + d)
    c2[:len(bins)] = c2[-len(bins):] = 0
    i2[:len(bins)], i2[-len(bins):] = (i1 + d)[:len(bins)], (i1 + d)[-len(bins):]
    i1[100], c2[100], i2[100] = 0, 0, SWITCH_LOCI - 1             # the chromosome's last locus
    rows = (c1, i1, c2, i2, cnt)
    return [Case("N1", rows, 1, SWITCH_LO, SWITCH_HI), Case("N2", rows, 1, SWITCH_LO, SWITCH_HI + 1)]
