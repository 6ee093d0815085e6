"""The inputs of tests/test_gpu_kr_shapes.py, checked without a GPU: every matrix of tests/kr_shapes.py must have the property it is
named for and reach the seam of fhx_kr.hip it is aimed at (by the model restated in kr_shapes.py, whose constants are read back from
the source here), or the GPU test would pass without aiming at anything.  And the oracle the GPU is compared with bit for bit
(oracle/kr_oracle.c through oracle/hickry_oracle.py) is itself held to a plain reference: exact integer arithmetic where every sum
stays below 2^53, math.fsum within the standard bound of recursive summation (which holds for any order of the adds) elsewhere."""
import functools
import math
import os
import re

import numpy as np
import pytest

import kr_shapes as ks
from oracle import hickry_oracle as ho

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fithic_amd", "csrc", "fhx_kr.hip")
U = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _built(kind, arg=None):
    m = getattr(ks, kind)() if arg is None else getattr(ks, kind)(arg)
    return m, ho.assemble(m.x, m.y, m.z, m.n)


def _lengths(A):
    return np.diff(A.indptr)


def _row(A, r):
    return A.indices[A.indptr[r]:A.indptr[r + 1]], A.data[A.indptr[r]:A.indptr[r + 1]]


def _symmetric_cells(A):
    rows = np.repeat(np.arange(A.n), _lengths(A))
    return set(zip(rows.tolist(), A.indices.tolist())) == set(zip(A.indices.tolist(), rows.tolist()))


# ---- the model is the source's -----------------------------------------------------------------------------------------------
def test_the_model_restates_the_constants_and_expressions_of_the_source():
    with open(SRC) as f:
        src = f.read()
    for name, value in (("TILE", ks.TILE), ("THREADS", ks.ROWS_PER_BLOCK * ks.WAVE), ("KR_CHUNK", ks.KR_CHUNK), ("KR_PAD", ks.KR_PAD)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), src), name
    assert src.count("const int64_t blk = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);") == 2      # kr_spmv, kr_spmv_packed
    assert src.count("const int64_t per = (n_blocks + 7) / 8;") == 3 and "const int64_t n_blocks = (n + 3) / 4;" in src
    assert src.count("const int64_t row = blk * 4 + (threadIdx.x >> 6);") == 2
    assert src.count("for (int64_t base = b; base < e; base += 2 * KR_CHUNK)") == 2
    assert src.count("const bool second = base + KR_CHUNK < e;") == 2
    assert "for (int64_t j0 = b; j0 < e; j0 += 64)" in src and "for (int64_t base = 0; base < n_tiles; base += TILE)" in src
    assert "(n + krd::TILE - 1) / krd::TILE" in src


def test_chunk_walk_model():
    assert ks.chunk_walk(0) == ([], 0, 0)
    assert ks.chunk_walk(1) == ([(0, False)], 255, 1)
    assert ks.chunk_walk(256) == ([(0, False)], 0, 256)           # one full chunk, the second not taken
    assert ks.chunk_walk(257) == ([(0, True)], 255, 1)            # the second chunk for one cell
    assert ks.chunk_walk(512) == ([(0, True)], 0, 256)
    assert ks.chunk_walk(513) == ([(0, True), (512, False)], 255, 1)
    assert ks.chunk_walk(768) == ([(0, True), (512, False)], 0, 256)
    assert ks.chunk_walk(769) == ([(0, True), (512, True)], 255, 1)
    assert max(ks.chunk_walk(L)[1] for L in range(1, 2000)) == 255 <= ks.KR_PAD


# ---- 1. assembly order ---------------------------------------------------------------------------------------------------------
def _left_to_right(values):
    s = values[0]
    for v in values[1:]:
        s = s + v
    return s


@pytest.mark.parametrize("kind", ["assembly_long_run", "assembly_both_ways", "assembly_diagonal"])
def test_assembly_runs_depend_on_the_order_of_their_adds(kind):
    m, A = _built(kind)
    run = m.about["run"]
    want = _left_to_right(run)
    others = {float(np.sum(np.array(run))), _left_to_right(sorted(run))}
    assert others != {want}, "every order gives the same bits: a wrong order would not show"
    r, c = m.about["cell"]
    cols, vals = _row(A, r)
    assert vals[cols == c][0] == want == ks.assemble_plain(m)[(r, c)]
    plain = ks.assemble_plain(m)                                  # the oracle's whole matrix equals the Python loop's
    rows = np.repeat(np.arange(A.n), _lengths(A))
    assert sorted(plain) == list(zip(rows.tolist(), A.indices.tolist()))
    assert np.array_equal(_bits(A.data), _bits([plain[k] for k in sorted(plain)]))


def test_assembly_long_run_starts_at_1021_of_a_tile_and_crosses_five():
    m, A = _built("assembly_long_run")
    assert _left_to_right(m.about["run"]) == 2.0 ** 53 + 3000 and len(m.about["run"]) == 6001
    keys = ks.sorted_keys(m)
    r, c = m.about["cell"]
    head = int(np.searchsorted(keys, r * m.n + c, "left"))
    assert head % ks.TILE == 1021 and int(np.searchsorted(keys, r * m.n + c, "right")) - head == 6001
    assert (head + 6000) // ks.TILE - head // ks.TILE >= 5
    assert np.all(m.x[:6001] == r) and np.all(m.y[:6001] == c)   # all written as (x, y)


def test_assembly_both_ways_differs_from_plain_file_order():
    m, A = _built("assembly_both_ways")
    r, c = m.about["cell"]
    written = [(int(a), int(b)) for a, b in zip(m.x[:12], m.y[:12])]
    assert written == [(r, c), (c, r)] * 6
    grouped, filed = _left_to_right(m.about["run"]), _left_to_right(m.about["file_order"])
    assert grouped != filed
    assert _row(A, r)[1][_row(A, r)[0] == c][0] == grouped
    assert _row(A, c)[1][_row(A, c)[0] == r][0] == _left_to_right(ks.RUN_B[1::2] + ks.RUN_B[0::2])       # its own rows first there


def test_assembly_diagonal_is_not_twice_the_sum():
    m, A = _built("assembly_diagonal")
    a, b = ks.DIAG_C
    assert ((a + b) + a) + b != 2 * (a + b)
    assert _row(A, 2)[1][_row(A, 2)[0] == 2][0] == ((a + b) + a) + b


def test_assembly_empty_loci():
    m, A = _built("assembly_empty_loci")
    empty, last = m.about["empty"], m.about["last"]
    assert [hi - lo for lo, hi in ks.EMPTY_RUNS] == [1, 70, 9] and ks.EMPTY_RUNS[0][0] == 0 and ks.EMPTY_RUNS[-1][1] == m.n
    assert np.array_equal(_lengths(A) == 0, empty) and _lengths(A)[last] == 300 and empty[last + 1:].all()
    for lo, hi in ks.EMPTY_RUNS:
        assert len(set(A.indptr[lo:hi + 1].tolist())) == 1        # flat
    sums = A.dot(np.ones(m.n))
    assert np.all(_bits(sums[empty]) == 0)                        # +0.0
    assert ks.chunk_walk(300) == ([(0, True)], 212, 44) and A.indptr[last + 1] == A.nnz


# ---- 2. row lengths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("last", ks.LAST_HUBS)
def test_row_lengths_have_one_hub_of_every_length_and_the_named_last_row(last):
    m, A = _built("row_lengths", last)
    hubs, lengths = m.about["hubs"], _lengths(A)
    assert sorted(hubs) == ks.HUB_LENGTHS == sorted(set(ks.HUB_LENGTHS))
    for L, hub in hubs.items():
        assert lengths[hub] == L
    leaves = np.ones(m.n, bool)
    leaves[list(hubs.values())] = False
    assert np.all(lengths[leaves] == 2)
    assert hubs[last] == m.n - 1 and lengths[-1] == last and ks.chunk_walk(last)[1:] == (255, 1)       # 255 cells into the padding
    rows = np.repeat(np.arange(m.n), lengths)
    assert np.all(np.isin(np.arange(m.n), A.indices[rows == A.indices]))                                # every locus has a diagonal
    assert _symmetric_cells(A)
    assert hubs[1] == 0 and np.array_equal(np.flatnonzero(A.indices == 0), [0])                        # column 0: row 0 alone
    assert np.all(A.data == np.floor(A.data)) and 1 <= A.data.min() and A.data.max() < 300             # packs
    span = np.array([A.indices[A.indptr[r + 1] - 1] - A.indices[A.indptr[r]] for r in range(m.n)])
    assert span.max() < 65536
    walks = {L: ks.chunk_walk(L) for L in ks.HUB_LENGTHS}
    assert {len(w[0]) for w in walks.values()} == {1, 2, 3}
    assert {L for L, w in walks.items() if w[1] == 0} == {256, 512, 768, 1024}                         # rows that end on a chunk edge
    assert {L for L, w in walks.items() if w[2] == 1} >= {1, 257, 513, 769, 1025}                      # one cell in the last chunk
    assert [walks[L][0][-1][1] for L in (256, 257, 768, 769, 1024, 1025)] == [False, True, False, True, True, False]
    assert {L % 4 for L in ks.HUB_LENGTHS} == {0, 1, 3}            # a lane's four cells cut after 1 and 3 (after 2: the 130 of case 7)
    vs = ks.vectors(m.n, 1)
    assert np.isinf(vs["inf at 0"][0]) and np.isnan(vs["nan at 0"][0])
    for name, v in vs.items():
        assert np.isfinite(v[1:]).all() and (v[1:] < 0).any() and (v[1:] > 0).any()
        assert np.isfinite(A.dot(v)[1:]).all(), name                                                    # no row but row 0 sees column 0


@pytest.mark.parametrize("last", ks.LAST_HUBS)
def test_row_lengths_balance_in_the_oracle(last):
    m, A = _built("row_lengths", last)
    x, i, k = ho.knight_ruiz(A)
    assert 1 <= i <= 30 and np.isfinite(x).all()
    assert np.max(np.abs(x * A.dot(x) - 1.0)) < 1e-5              # it is a balance


# ---- 3. few rows ---------------------------------------------------------------------------------------------------------------
def test_few_rows_reach_the_early_outs_of_the_remap_and_every_row_is_written_once():
    assert ks.FEW_ROWS == [1, 2, 3, 5, 29, 31, 32, 33, 37]
    seen = set()
    for n in ks.FEW_ROWS + [ks.row_lengths(513).n, ks.LIMIT_N, 900, 904]:
        writes, grid, idle = ks.row_writes(n)
        assert np.all(writes == 1), n
        n_blocks = (n + 3) // 4
        seen |= {("fewer than 8 blocks", n_blocks < 8), ("n % 4", n % 4), ("idle blocks", idle > 0), ("per", min(2, grid // 8))}
    assert seen >= {("fewer than 8 blocks", True), ("fewer than 8 blocks", False), ("n % 4", 0), ("n % 4", 1), ("n % 4", 2),
                    ("n % 4", 3), ("idle blocks", True), ("idle blocks", False), ("per", 1), ("per", 2)}
    assert ks.row_writes(1)[1:] == (8, 7) and ks.row_writes(33)[1:] == (16, 7)       # blk >= n_blocks in 7 workgroups each
    assert ks.row_writes(32)[1:] == (8, 0)
    for n in ks.FEW_ROWS:
        m, A = _built("few_rows", n)
        assert _symmetric_cells(A) and np.all(A.data == np.floor(A.data)) and _lengths(A).min() >= 1
        x, i, k = ho.knight_ruiz(A)
        assert np.isfinite(x).all() and np.max(np.abs(x * A.dot(x) - 1.0)) < 1e-5


# ---- 4. format limits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ks.LIMITS))
def test_format_limits_sit_on_the_last_accepted_and_first_refused_values(name):
    m, A = _built("format_limit", name)
    base = _built("format_limit", "band")[1]
    cell, count, value_bytes = ks.LIMITS[name]
    assert m.n == 65540 and _lengths(A).max() <= 4 and _symmetric_cells(A)
    assert ks.value_bytes(A) == value_bytes
    first = A.indices[A.indptr[:-1]]
    offs = A.indices - np.repeat(first, _lengths(A))
    if cell is None:
        assert offs.max() == 2 and A.data.max() < 400
        return
    r, c = cell
    assert _row(A, r)[1][_row(A, r)[0] == c][0] == count == _row(A, c)[1][_row(A, c)[0] == r][0]
    cells_of = lambda M: set(zip((np.repeat(np.arange(M.n), _lengths(M)) * M.n + M.indices).tolist(), M.data.tolist()))
    assert {key for key, _ in cells_of(A) - cells_of(base)} == {r * m.n + c, c * m.n + r}               # one cell and its mirror
    if name == "offset 65535 count 65535":
        assert offs.max() == 65535 == ks.FAR and A.data.max() == 65535.0
        assert _row(A, 0)[0].tolist() == [0, 1, 65535] and _row(A, 65535)[0].tolist() == [0, 65534, 65535]    # transposed: far one first
        assert np.sum(offs == 65535) == 2 and (65535 << 16 | 65535) == 0xFFFFFFFF
    elif name == "offset 65536":
        assert offs.max() == 65536 and np.sum(offs == 65536) == 2 and A.data.max() < 400                     # nothing else refuses it
        assert _row(A, 0)[0].tolist() == [0, 1, 65536] and _row(A, 65536)[0].tolist() == [0, 65536]
    else:
        assert offs.max() == 2
    f32 = np.float32(count)
    assert {"count 65536": count == 65536, "count 2^24": count == 16777216 and float(f32) == count,
            "count 2^24+2": count == 16777218 and float(f32) == count, "count 2^24+1": count == 16777217 and float(f32) != count,
            "count 0.5": float(f32) == 0.5, "count 0.1": float(f32) != 0.1}.get(name, True)


# ---- 5. removal ----------------------------------------------------------------------------------------------------------------
def test_removal_rows_lose_the_steps_they_are_named_for():
    m, A = _built("removal", False)
    removed, val, sums = ho.sparse_rows(A, 0.0)
    weak = np.sort(m.about["weak"])
    assert val == 1.0 and np.array_equal(removed, weak) and np.all(sums[weak] == 1.0) and np.all(np.delete(sums, weak) > 1.0)
    assert np.all(_lengths(A)[weak] == 1) and np.all(A.data[A.indptr[weak]] == 1.0)
    keep = np.ones(m.n, bool)
    keep[weak] = False
    steps = {}
    for L, hub in m.about["rows"].items():
        cols, _ = _row(A, hub)
        assert len(cols) == L
        steps[L] = ks.compact_steps(keep[cols])
    assert sorted(steps) == [63, 64, 65, 128, 129, 200]
    full = tuple(range(64))
    assert steps[64] == [(0,)] and steps[65] == [(63,), (0,)]                     # lane 0 alone; lane 63 alone, then a step of one cell
    assert steps[128] == [(), full] and steps[129] == [full, (), (0,)]            # a whole step removed; none removed
    assert steps[63] == [tuple(range(0, 63, 2))]                                  # alternate cells, 63 cells: the row ends inside a step
    assert steps[200] == [tuple(range(0, 64, 2)), tuple(range(1, 64, 2)), full, tuple(range(8))]
    # a lane that is dropped in one step and kept in a later one (a per-lane base would be stale there)
    assert any(l not in s0 and l in s1 for st in steps.values() for s0, s1 in zip(st, st[1:]) if s0 for l in range(64))
    assert {L % 64 for L in steps} >= {0, 1, 63}                                  # rows ending on, behind and before a step edge
    R = ho.drop(A, removed)
    assert R.n == m.n - len(weak) and _lengths(R).min() >= 1
    assert np.all(R.data == np.floor(R.data)) and R.data.max() < 65536           # packs
    x, i, k = ho.knight_ruiz(R)
    assert np.isfinite(x).all() and np.max(np.abs(x * R.dot(x) - 1.0)) < 1e-5


def test_removal_can_leave_an_empty_row_and_the_oracle_then_gives_nan_after_one_step():
    m, A = _built("removal", True)
    removed, val, sums = ho.sparse_rows(A, 0.0)
    lonely = m.about["lonely"]
    assert val == 1.0 and np.array_equal(removed, np.sort(m.about["weak"])) and sums[lonely] == 3.0
    assert set(_row(A, lonely)[0].tolist()) <= set(removed.tolist())
    R = ho.drop(A, removed)
    new = lonely - int(np.sum(removed < lonely))
    assert _lengths(R)[new] == 0 and np.sum(_lengths(R) == 0) == 1
    with np.errstate(all="ignore"):
        x, i, k = ho.knight_ruiz(R)
    assert (i, k) == (1, 1) and np.isnan(x).all()


# ---- 6. long reductions --------------------------------------------------------------------------------------------------------
def test_dot_sizes_sit_on_the_tile_and_buffer_seams():
    M = ks.M20
    assert ks.DOT_SIZES == [1, 255, 256, 257, 1023, 1024, 1025, 4097, M - 1, M, M + 1, 1024 * 1032 + 1, 1024 * 1033 + 5, 2 * M + 3]
    assert [ks.tiles_of(n) for n in (1023, 1024, 1025, M - 1, M, M + 1)] == [1, 1, 2, 1024, 1024, 1025]
    assert [ks.finish_buffers(n) for n in (M, M + 1, 2 * M, 2 * M + 3)] == [1, 2, 2, 3]
    second = {(ks.tiles_of(n) - 1024) for n in ks.DOT_SIZES if ks.finish_buffers(n) == 2}
    assert second == {1, 9, 10}                                   # the second buffer: one partial, a block of 8 and a tail
    assert ks.tiles_of(2 * M + 3) - 2048 == 1
    assert ks.finish_buffers(ks.LONG_N) == 2 and ks.tiles_of(ks.LONG_N) == 1026 and ks.LONG_N == M + 1033


def test_long_tridiagonal_is_an_integer_matrix_with_three_cells_a_row():
    m, A = _built("long_tridiagonal")
    L = _lengths(A)
    assert m.n == ks.LONG_N and L[0] == L[-1] == 2 and np.all(L[1:-1] == 3) and A.nnz <= 3_200_000
    assert np.all(A.data == np.floor(A.data)) and 1 <= A.data.min() and A.data.max() < 40


# ---- 7. loop exits -------------------------------------------------------------------------------------------------------------
def test_loop_exit_matrices_reach_every_exit_of_the_iteration():
    seen, per_case = set(), {}
    for name in ks.LOOP_CASES:
        m, A = _built("loop_exit", name)
        assert 890 <= m.n <= 910 and set(_lengths(A).tolist()) <= ks.LOOP_ROW_LENGTHS and _symmetric_cells(A)
        assert np.all(A.data == np.floor(A.data)) and A.data.min() >= 1
        assert ks.value_bytes(A) == (4 if A.data.max() > 65535 else 2)                 # 60 000 on a diagonal counts twice
        trace = []
        x, i, k = ho.knight_ruiz(A, trace=trace)
        plain = ho.knight_ruiz(A)
        assert np.array_equal(_bits(x), _bits(plain[0])) and (i, k) == plain[1:]       # the trace changes no value
        assert set(trace) <= {"accept", "delta", "Delta", "k>10", "i>30"} and np.isfinite(x).all()
        assert ("i>30" in trace) == (i == 31)
        per_case[name] = set(trace)
        seen |= set(trace)
    assert seen == {"accept", "delta", "Delta", "k>10", "i>30"}
    assert "i>30" in per_case["chain"] and {"delta", "Delta", "k>10"} <= per_case["band 1"]
    assert set().union(*[set(_lengths(_built("loop_exit", c)[1]).tolist()) for c in ks.LOOP_CASES]) == ks.LOOP_ROW_LENGTHS
    heavy = _built("loop_exit", "heavy 0")[0]
    assert set(heavy.z.tolist()) == {1.0, 60000.0} and 0.002 < np.mean(heavy.z == 60000.0) < 0.03


# ---- the oracle itself -----------------------------------------------------------------------------------------------------------
INTEGER_MATRICES = [("row_lengths", 513), ("row_lengths", 257), ("removal", False), ("removal", True), ("format_limit", "band"),
                    ("format_limit", "offset 65535 count 65535"), ("loop_exit", "heavy 0"), ("loop_exit", "chain")] + \
                   [("few_rows", n) for n in ks.FEW_ROWS]
REAL_MATRICES = [("row_lengths", 513), ("row_lengths", 257), ("assembly_empty_loci", None), ("removal", False),
                 ("format_limit", "count 0.1"), ("few_rows", 37), ("few_rows", 1)]


@pytest.mark.parametrize("kind,arg", INTEGER_MATRICES)
def test_oracle_spmv_is_exact_on_integers(kind, arg):
    m, A = _built(kind, arg)
    rng = np.random.default_rng(3)
    v = rng.integers(-8, 9, A.n)
    data = A.data.astype(np.int64)
    assert np.array_equal(data.astype(np.float64), A.data)
    prod = data * v[A.indices]
    want = np.zeros(A.n, np.int64)
    np.add.at(want, np.repeat(np.arange(A.n), _lengths(A)), prod)
    bound = np.zeros(A.n, np.int64)
    np.add.at(bound, np.repeat(np.arange(A.n), _lengths(A)), np.abs(prod))
    assert bound.max() < 2 ** 53                                  # no partial sum can round
    got = A.dot(v.astype(np.float64))
    assert np.array_equal(got, want.astype(np.float64)) and np.array_equal(got.astype(np.int64), want)


@pytest.mark.parametrize("n", ks.DOT_SIZES)
def test_oracle_dot_is_exact_on_integers_and_within_the_summation_bound_on_reals(n):
    rng = np.random.default_rng(n)
    a, b = rng.integers(-1000, 1001, n), rng.integers(-1000, 1001, n)
    assert int(np.abs(a * b).sum()) < 2 ** 53
    assert ho.dot(a.astype(np.float64), b.astype(np.float64)) == float(int((a * b).sum()))
    assert ho.dot(a.astype(np.float64)) == float(int(a.sum()))
    a, b = ks.dot_vectors(n)
    assert (a < 0).any() or n == 1
    prod = a * b                                                  # each product rounded once, as in the oracle: the bound is on the sum
    assert abs(ho.dot(a, b) - math.fsum(prod)) <= (n + 1) * U * math.fsum(np.abs(prod))
    assert abs(ho.dot(a) - math.fsum(a)) <= (n + 1) * U * math.fsum(np.abs(a))


@pytest.mark.parametrize("kind,arg", REAL_MATRICES)
def test_oracle_spmv_is_within_the_summation_bound_of_fsum(kind, arg):
    m, A = _built(kind, arg)
    v = ks.vectors(A.n, 2)["lognormal"]
    got = A.dot(v)
    rows = range(A.n) if A.n <= 10000 else np.random.default_rng(4).choice(A.n, 3000, replace=False).tolist() + [100, 101]
    differ = long_rows = 0
    for r in rows:
        cols, vals = _row(A, r)
        prod = vals * v[cols]                                     # rounded once, as in the oracle
        assert abs(got[r] - math.fsum(prod)) <= len(cols) * U * math.fsum(np.abs(prod)), (r, len(cols))
        if len(cols) >= 256:
            long_rows += 1
            differ += _bits([got[r]])[0] != _bits([np.dot(vals, v[cols])])[0]
    if kind == "row_lengths":                                     # the oracle's order is not numpy's: equal bits would say little
        assert long_rows == sum(L >= 256 for L in ks.HUB_LENGTHS) and 2 * differ >= long_rows, (differ, long_rows)
