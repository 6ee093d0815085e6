"""TEST INFRASTRUCTURE - the built matrices of tests/test_gpu_kr_shapes.py and a model of which seam of fhx_kr.hip each one reaches,
no GPU needed (tests/test_kr_shape_inputs.py checks that every case has the property it is named for, and holds the oracle the GPU
is compared with to a plain high-precision reference).

Restated from fithic_amd/csrc/fhx_kr.hip, constants as named there:
  row -> workgroup   launch_spmv: n_blocks = ceil(n / 4) row blocks of 4 waves (THREADS = 256 = 4 wave64), per = ceil(n_blocks / 8),
                     grid = max(1, 8 * per); kr_spmv: blk = (bid & 7) * per + (bid >> 3), out when blk >= n_blocks, row = 4 * blk + wave,
                     out when row >= n                                                                       (row_writes)
  chunk walk         for (base = 0; base < L; base += 2 * KR_CHUNK): the chunk at base, and the one at base + KR_CHUNK when
                     base + KR_CHUNK < L; KR_CHUNK = 256 cells, lane l loads cells 4l..4l+3 whole, so a chunk is read whole and the
                     cells past the row end are predicated; KR_PAD = 256 cells stand behind the last row              (chunk_walk)
  tile counts        TILE = 1024 elements per partial (tiles_of), kr_finish stages TILE partials per LDS buffer        (finish_buffers)
  formats            kr_to_f32 refuses a value that is not a binary32 number; kr_pack16 refuses a column offset above 65535 from the
                     row's first column and a value that is not an integer in [0, 65535]                              (value_bytes)
  compaction         kr_count_kept / kr_compact walk a row in steps of 64 cells (one per lane), a ballot prefix places the kept
                     cells of a step and base advances by the step's popcount                                          (compact_steps)

A matrix is given as the rows of an interactions file: locus indices x, y and counts z.  The assembly is M + M.T of the coo
matrix, so a row written once as (i, j), i != j, is the cell (i, j) and the cell (j, i), and a row written (i, i) counts twice."""
import numpy as np

KR_CHUNK = 256
KR_PAD = 256
TILE = 1024
WAVE = 64
ROWS_PER_BLOCK = 4
XCDS = 8


# ---- the model -------------------------------------------------------------------------------------------------------------
def row_writes(n):
    """how often each of the n rows is written by one kr_spmv / kr_spmv_packed launch"""
    n_blocks = (n + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK
    per = (n_blocks + XCDS - 1) // XCDS
    grid = max(1, per * XCDS)
    writes = np.zeros(n, np.int64)
    idle = 0
    for bid in range(grid):
        blk = (bid & (XCDS - 1)) * per + (bid >> 3)
        if blk >= n_blocks:
            idle += 1
            continue
        for wave in range(ROWS_PER_BLOCK):
            row = blk * ROWS_PER_BLOCK + wave
            if row < n:
                writes[row] += 1
    return writes, grid, idle


def chunk_walk(L):
    """-> [(base, second)] of a row of L cells, the number of cells read behind the row end, and the valid cells of the last
    chunk that is read"""
    steps, read_to = [], 0
    base = 0
    while base < L:
        second = base + KR_CHUNK < L
        steps.append((base, second))
        read_to = base + (2 if second else 1) * KR_CHUNK
        base += 2 * KR_CHUNK
    last_valid = L - (read_to - KR_CHUNK) if steps else 0
    return steps, max(0, read_to - L), last_valid


def tiles_of(n):
    return max(1, (n + TILE - 1) // TILE)


def finish_buffers(n):
    """LDS buffers kr_finish walks for a vector of n elements; only the first starts its unrolled blocks at i = 1"""
    return (tiles_of(n) + TILE - 1) // TILE


def compact_steps(keep):
    """keep: bool per cell of one row in column order -> the kept lanes of every 64-cell step, as tuples"""
    keep = np.asarray(keep, bool)
    return [tuple(np.flatnonzero(keep[s:s + WAVE]).tolist()) for s in range(0, len(keep), WAVE)]


def value_bytes(A):
    """the format a balance streams, by the sentences of kr_to_f32 and kr_pack16: 8 unless every value is a binary32 number; then 2
    when every value is an integer in [0, 65535] and no row spans more than 65 535 columns, else 4.  A: a CSR with indptr, indices,
    data"""
    if not np.array_equal(A.data.astype(np.float32).astype(np.float64), A.data):
        return 8
    lengths = np.diff(A.indptr)
    first = A.indices[A.indptr[:-1][lengths > 0]]
    offs = A.indices - np.repeat(first, lengths[lengths > 0])
    small = np.all(A.data == np.floor(A.data)) and A.data.min() >= 0 and A.data.max() <= 65535
    return 2 if small and offs.max() <= 65535 else 4


# ---- matrices --------------------------------------------------------------------------------------------------------------
class Mat:
    """file rows (x, y, z) over n loci, and what the case is about"""

    def __init__(self, n, x, y, z, **about):
        self.n = int(n)
        self.x, self.y = np.ascontiguousarray(x, np.int64), np.ascontiguousarray(y, np.int64)
        self.z = np.ascontiguousarray(z, np.float64)
        assert len(self.x) == len(self.y) == len(self.z) and (len(self.x) == 0 or 0 <= min(self.x.min(), self.y.min()))
        assert len(self.x) == 0 or max(self.x.max(), self.y.max()) < self.n
        self.about = about

    def load(self, kr):
        zeros = np.zeros(len(self.x), np.int32)
        kr.load_loci(np.zeros(self.n, np.int32), np.arange(self.n, dtype=np.int32))
        kr.load_pairs(zeros, self.x.astype(np.int32), zeros, self.y.astype(np.int32), self.z)


def _mat(n, cells, **about):
    a = np.array(cells, np.float64).reshape(-1, 3)
    return Mat(n, a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), a[:, 2], **about)


def assemble_plain(m):
    """the cells of M + M.T with a Python float loop: the rows as written (x, y) first, then the rows transposed, each in file
    order, every cell added left to right -> {(row, col): value}"""
    cells = {}
    for rows, cols in ((m.x, m.y), (m.y, m.x)):
        for r, c, v in zip(rows.tolist(), cols.tolist(), m.z.tolist()):
            cells[(r, c)] = cells[(r, c)] + v if (r, c) in cells else v
    return cells


def sorted_keys(m):
    """the 2m cell keys in the order the stable sort leaves them"""
    return np.sort(np.concatenate([m.x * m.n + m.y, m.y * m.n + m.x]), kind="stable")


# -- 1. assembly order
RUN_A = [1.0] * 3000 + [2.0 ** 53] + [1.0] * 3000
RUN_B = [1.0, 2.0 ** 53] + [1.0] * 10
DIAG_C = (0.7, 0.1)


def assembly_long_run():
    """(a) the cell (1, 2) written 6001 times; 1021 cells of row 0 whose transposes sort behind it stand in front"""
    p, q, fill = 1, 2, 1021
    n = q + 1 + fill
    cells = [(p, q, v) for v in RUN_A] + [(0, c, 1 + c % 7) for c in range(q + 1, n)]
    return _mat(n, cells, cell=(p, q), run=RUN_A)


def assembly_both_ways():
    """(b) the cell (1, 3) written alternately as (1, 3) and (3, 1)"""
    p, q = 1, 3
    cells = [((p, q, v) if k % 2 == 0 else (q, p, v)) for k, v in enumerate(RUN_B)]
    return _mat(5, cells + [(0, 4, 2.0)], cell=(p, q), run=RUN_B[0::2] + RUN_B[1::2], file_order=RUN_B)


def assembly_diagonal():
    """(c) the diagonal cell (2, 2) on two file rows a, b: added as a, b, a, b"""
    a, b = DIAG_C
    return _mat(4, [(2, 2, a), (0, 1, 3.0), (2, 2, b)], cell=(2, 2), run=[a, b, a, b])


EMPTY_RUNS = [(0, 1), (200, 270), (491, 500)]


def assembly_empty_loci():
    """(d) loci without a cell: the first, 70 in the middle, the last 9; the last row that has cells has 300"""
    n, last = 500, 490
    rng = np.random.default_rng(41)
    empty = np.zeros(n, bool)
    for lo, hi in EMPTY_RUNS:
        empty[lo:hi] = True
    live = np.flatnonzero(~empty)
    cells = [(i, i, rng.integers(1, 64) / 8.0) for i in live]
    others = rng.choice(live[live < last], 299, replace=False)
    cells += [(c, last, rng.integers(1, 64) / 8.0) for c in others]
    return _mat(n, cells, empty=empty, last=last)


# -- 2. row lengths
HUB_LENGTHS = [1, 3, 4, 5, 63, 64, 65, 252, 255, 256, 257, 260, 511, 512, 513, 767, 768, 769, 1024, 1025, 1300]
LAST_HUBS = [513, 257]


def row_lengths(last):
    """one hub row of every length of HUB_LENGTHS: the hub stands behind its block of leaves, every locus has a diagonal, a leaf
    has its diagonal and the hub.  The 1-cell hub is locus 0, so column 0 belongs to row 0 alone; the hub of `last` cells is the
    last row.  Counts are integers below 300 (a diagonal, written once, counts twice)."""
    rng = np.random.default_rng(1000 + last)
    order = [1] + [L for L in HUB_LENGTHS if L not in (1, last)] + [last]
    cells, hubs, at = [], {}, 0
    for L in order:
        hub = at + L - 1
        hubs[L] = hub
        for leaf in range(at, hub):
            cells.append((leaf, leaf, rng.integers(1, 150)))
            cells.append((leaf, hub, rng.integers(1, 300)))
        cells.append((hub, hub, rng.integers(1, 150)))
        at = hub + 1
    return _mat(at, cells, hubs=hubs, last=last)


def vectors(n, seed):
    """lognormal values with random signs, and the same with inf and with nan at element 0"""
    rng = np.random.default_rng(seed)
    v = rng.lognormal(0, 1, n) * rng.choice([-1.0, 1.0], n)
    vi, vn = v.copy(), v.copy()
    vi[0], vn[0] = np.inf, np.nan
    return {"lognormal": v, "inf at 0": vi, "nan at 0": vn}


# -- 3. few rows
FEW_ROWS = [1, 2, 3, 5, 29, 31, 32, 33, 37]


def few_rows(n):
    """band of half-width 2 with integer counts"""
    rng = np.random.default_rng(300 + n)
    return _mat(n, [(i, j, rng.integers(1, 50)) for i in range(n) for j in range(i, min(n, i + 3))])


# -- 4. format limits
LIMIT_N = 65540
FAR = 65535                                                       # the last column offset kr_pack16 takes
# name -> (cell, count, value_bytes of the balance)
LIMITS = {
    "band": (None, None, 2),
    "offset 65535 count 65535": ((0, FAR), 65535.0, 2),
    "offset 65536": ((0, FAR + 1), 7.0, 4),
    "count 65536": ((100, 101), 65536.0, 4),
    "count 2^24": ((100, 101), 2.0 ** 24, 4),
    "count 2^24+2": ((100, 101), 2.0 ** 24 + 2, 4),
    "count 2^24+1": ((100, 101), 2.0 ** 24 + 1, 8),
    "count 0.5": ((100, 101), 0.5, 4),
    "count 0.1": ((100, 101), 0.1, 8),
}


def format_limit(name):
    """diagonal and first off-diagonal, the band cut on both sides of locus FAR + 1, so that FAR is the last column of row FAR and
    FAR + 1 the last of row FAR + 1: the transposed row of a far cell then has the same largest offset as the row itself.  One
    cell is set (the band's own) or added (the far ones)"""
    n = LIMIT_N
    rng = np.random.default_rng(77)
    i = np.arange(n)
    up = i[(i + 1 < n) & (i != FAR) & (i != FAR + 1)]
    x, y = np.concatenate([i, up]), np.concatenate([i, up + 1])
    z = rng.integers(1, 200, len(x)).astype(np.float64)
    cell, count, value_bytes = LIMITS[name]
    if cell is not None:
        at = np.flatnonzero((x == cell[0]) & (y == cell[1]))
        if len(at):
            z[at[0]] = count
        else:
            x, y, z = np.append(x, cell[0]), np.append(y, cell[1]), np.append(z, count)
    return Mat(n, x, y, z, cell=cell, count=count, value_bytes=value_bytes)


# -- 5. removal
# cells of a long row in column order: D its diagonal, W a weak leaf (its one cell is this one, count 1), K a kept leaf (diagonal
# and this cell).  Steps of 64.
LONG_ROWS = {
    63: "D" + "WK" * 31,                                          # alternate cells, the row ends inside a step
    64: "D" + "W" * 63,                                           # all but position 0; ends on a step edge
    65: "W" * 63 + "D" + "K",                                     # all but position 63, then one cell in a step of its own
    128: "W" * 64 + "D" + "K" * 63,                               # one whole step, then a step that loses nothing
    129: "K" * 63 + "D" + "W" * 64 + "K",                         # a whole step removed between two kept ones
    200: "D" + "WK" * 31 + "W" + "WK" * 32 + "K" * 64 + "K" * 8,  # even lanes kept, then odd lanes kept
}


def removal(extra_hub=False):
    """hubs with the rows of LONG_ROWS.  A weak leaf has row sum 1, every other locus more, so remove_sparse(0.0) removes
    exactly the weak leaves.  extra_hub: one more locus with three weak leaves and nothing else - kept (row sum 3), its reduced
    row empty."""
    rng = np.random.default_rng(55)
    cells, at, rows, weak = [], 0, {}, []
    for L, pattern in LONG_ROWS.items():
        assert len(pattern) == L and pattern.count("D") == 1
        hub = at + pattern.index("D")
        rows[L] = hub
        for k, kind in enumerate(pattern):
            locus = at + k
            if kind == "W":
                weak.append(locus)
                cells.append((min(locus, hub), max(locus, hub), 1))
            else:
                cells.append((locus, locus, rng.integers(1, 100)))
                if kind == "K":
                    cells.append((min(locus, hub), max(locus, hub), rng.integers(2, 300)))
        at += L
    lonely = None
    if extra_hub:
        lonely = at
        for leaf in (at + 1, at + 2, at + 3):
            weak.append(leaf)
            cells.append((lonely, leaf, 1))
        at += 4
    return _mat(at, cells, rows=rows, weak=np.array(weak, np.int64), lonely=lonely)


# -- 6. long reductions
M20 = 1 << 20
DOT_SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 4097, M20 - 1, M20, M20 + 1, 1024 * 1032 + 1, 1024 * 1033 + 5, 2 * M20 + 3]
LONG_N = M20 + 1033


def dot_vectors(n):
    rng = np.random.default_rng(9000 + n % 1000003)
    a = rng.lognormal(0, 1, n) * rng.choice([-1.0, 1.0], n)
    b = rng.lognormal(0, 1, n) * rng.choice([-1.0, 1.0], n)
    return a, b


def long_tridiagonal():
    n = LONG_N
    rng = np.random.default_rng(66)
    i = np.arange(n)
    x, y = np.concatenate([i, i[:-1]]), np.concatenate([i, i[:-1] + 1])
    return Mat(n, x, y, rng.integers(1, 20, len(x)).astype(np.float64))


# -- 7. loop exits
LOOP_ROW_LENGTHS = {1, 2, 3, 130, 257}
LOOP_CASES = ["heavy 0", "heavy 1", "band 0", "band 1", "chain"]


def loop_exit(name):
    """about 900 loci, integer counts.  "heavy k": hubs of 130 and 257 cells over leaves of 1 (the hub alone), 2 (diagonal and
    hub) and 3 cells (diagonal, hub and one other leaf).  "band k": diagonal and first off-diagonal.  In both, one cell in a hundred counts 60 000 and the
    others 1.  "chain": a path without diagonals, every count 1 or 2."""
    n = 900
    if name == "chain":
        rng = np.random.default_rng(12)
        return _mat(n, [(i, i + 1, rng.integers(1, 3)) for i in range(n - 1)])
    rng = np.random.default_rng(int(name.split()[1]))
    if name.startswith("band"):
        m = _mat(n, [(i, j, 1) for i in range(n) for j in range(i, min(n, i + 2))])
        m.z[rng.random(len(m.z)) < 0.01] = 60000.0
        return m
    cells, at = [], 0
    for L in (257, 130, 257, 130, 130):
        hub, leaves = at, list(range(at + 1, at + L))
        cells.append((hub, hub, 1))
        k = 0
        while k < len(leaves):
            kind = rng.integers(0, 3) if k + 1 < len(leaves) else rng.integers(0, 2)
            cells.append((hub, leaves[k], 1))
            if kind == 1:
                cells.append((leaves[k], leaves[k], 1))
            elif kind == 2:
                a, b = leaves[k], leaves[k + 1]
                cells += [(hub, b, 1), (a, a, 1), (b, b, 1), (a, b, 1)]
                k += 1
            k += 1
        at += L
    m = _mat(at, cells)
    m.z[rng.random(len(m.z)) < 0.01] = 60000.0
    return m
