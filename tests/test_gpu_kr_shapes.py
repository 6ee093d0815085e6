"""The Knight-Ruiz kernels (fithic_amd/csrc/fhx_kr.hip) on built matrices: chunk seams of kr_spmv / kr_spmv_packed, the XCD remap with
few rows, the last accepted and first refused values of kr_pack16 and kr_to_f32, kr_finish beyond one LDS buffer, the 64-cell steps
of kr_count_kept / kr_compact, the add order of kr_emit_cells, and every exit of the iteration in fhx_kr_balance.  Everything is
compared bit for bit with oracle/hickry_oracle.py (the same summation orders in plain C); nothing here has a tolerance.  The only
thing left uncompared is the payload of a NaN.

Matrices and the model of what each reaches: tests/kr_shapes.py, checked without a GPU by tests/test_kr_shape_inputs.py, which also
holds the oracle to exact integer arithmetic and to math.fsum.

Which SpMV kernel KrContext.spmv reaches depends on what ran before it, and every comparison below asserts info.value_bytes of the
preceding balance so that it names its kernel: before any balance kr_spmv<0, double>; after a balance of the same matrix
kr_spmv_packed<0> (value_bytes 2) or, in a context balanced under FHX_KR_NO_PACK=1, kr_spmv<0, float> (value_bytes 4).  The MODE 1
and MODE 2 epilogues (v = x * Ax, rk = 1 - v; w = x * A(x * p) + v * p) have no entry point of their own: they are covered through
balance, whose x, iteration counts and bias are compared on every matrix here."""
import functools

import numpy as np
import pytest

import kr_shapes as ks

pytestmark = pytest.mark.gpu

FORMATS = {"double": 8, "packed": 2, "float": 4}                  # name -> info.value_bytes of an integer matrix with narrow rows


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want, what):
    """equal bits; where the oracle has a NaN, a NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN mask")
    bad = np.flatnonzero(_bits(got)[~nan] != _bits(want)[~nan])
    assert len(bad) == 0, (what, "%d of %d differ, first at %d: got %r, want %r" % (
        len(bad), got.size, np.flatnonzero(~nan)[bad[0]], got[~nan][bad[0]], want[~nan][bad[0]]))


@functools.lru_cache(maxsize=None)
def _built(kind, arg=None):
    from oracle import hickry_oracle as ho
    m = getattr(ks, kind)() if arg is None else getattr(ks, kind)(arg)
    return m, ho.assemble(m.x, m.y, m.z, m.n)


@functools.lru_cache(maxsize=None)
def _balanced(kind, arg=None, perc=None):
    """the oracle's whole run -> (matrix that is balanced, removed, x, outer, inner, bias)"""
    from oracle import hickry_oracle as ho
    m, A = _built(kind, arg)
    removed = ho.sparse_rows(A, perc)[0] if perc is not None else np.zeros(0, np.int64)
    R = ho.drop(A, removed) if perc is not None else A
    with np.errstate(all="ignore"):
        x, i, k = ho.knight_ruiz(R)
        bias = ho.bias_vector(x, removed, A.n)
    return R, removed, x, i, k, bias


def _context(m, fmt, monkeypatch):
    from fithic_amd import _capi
    if fmt == "float":
        monkeypatch.setenv("FHX_KR_NO_PACK", "1")
    else:
        monkeypatch.delenv("FHX_KR_NO_PACK", raising=False)
    kr = _capi.KrContext(0)                                       # raises without a GPU or the library: no fallback
    m.load(kr)
    return kr


def _check_csr(kr, which, A, what):
    indptr, col, val = kr.get_csr(which)
    assert np.array_equal(indptr, A.indptr) and np.array_equal(col, A.indices), (what, "structure")
    _same(val, A.data, (what, "values"))


def _check_balance(kr, want, value_bytes, what):
    R, removed, x, i, k, bias = want
    gx, info = kr.balance(1e-6)
    assert info.value_bytes == value_bytes, (what, info.value_bytes)
    assert (info.n, info.nnz) == (R.n, R.nnz), what
    assert (info.outer_iterations, info.inner_iterations) == (i, k), what
    _same(gx, x, (what, "x"))
    _same(kr.bias(), bias, (what, "bias"))
    return info


def _check_spmv(kr, A, vectors, which, what, from_row=0):
    for name, v in vectors.items():
        got, _ = kr.spmv(v, which)
        want = A.dot(v)
        _same(got[from_row:], want[from_row:], (what, name))
        if from_row:                                              # the rows in front may hold inf or NaN: their class is compared
            assert np.isfinite(want[from_row:]).all(), (what, name)
            assert np.array_equal(np.isnan(got[:from_row]), np.isnan(want[:from_row])), (what, name)
            assert np.array_equal(np.isinf(got[:from_row]), np.isinf(want[:from_row])), (what, name)


# ---- 1. assembly order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["assembly_long_run", "assembly_both_ways", "assembly_diagonal"])
def test_duplicates_are_added_in_sort_order(kind, monkeypatch):
    """kr_emit_cells: the rows written (x, y) first, then those written (y, x), each in file order, one by one - also across the
    1024-key tiles of the sorted keys"""
    m, A = _built(kind)
    kr = _context(m, "double", monkeypatch)
    try:
        _check_csr(kr, 0, A, kind)
        plain = ks.assemble_plain(m)
        indptr, col, val = kr.get_csr(0)
        rows = np.repeat(np.arange(m.n), np.diff(indptr))
        assert list(zip(rows.tolist(), col.tolist())) == sorted(plain)
        _same(val, [plain[key] for key in sorted(plain)], (kind, "the Python loop"))
    finally:
        kr.close()


def test_loci_without_cells(monkeypatch):
    """kr_indptr flat over the empty first row, 70 empty rows and 9 empty last rows; their sums are +0.0; the 300-cell row in front
    of the empty tail reads its second chunk out of the padding"""
    m, A = _built("assembly_empty_loci")
    want = _balanced("assembly_empty_loci")
    kr = _context(m, "double", monkeypatch)
    try:
        _check_csr(kr, 0, A, "empty loci")
        sums = kr.row_sums()
        _same(sums, A.dot(np.ones(m.n)), "row sums")
        assert np.all(_bits(sums[m.about["empty"]]) == 0)
        vectors = {k: v for k, v in ks.vectors(m.n, 3).items() if k == "lognormal"}       # row 0 is empty here, column 0 a cell of others
        _check_spmv(kr, A, vectors, 0, "empty loci, double")
        assert np.isnan(want[2]).all() and want[3:5] == (1, 1)                                  # an empty row: NaN after one step
        _check_balance(kr, want, 4, "empty loci")                                               # eighths: binary32, not packed
        _check_spmv(kr, A, vectors, 0, "empty loci, float")
    finally:
        kr.close()


# ---- 2. row lengths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("last", ks.LAST_HUBS)
def test_rows_of_every_length_around_the_chunk_seams(last, fmt, monkeypatch):
    """hub rows of 1 to 1300 cells, the last row one that reads 255 cells of padding; a vector of the test's choice, and one with inf
    / nan at element 0, which every predicated lane gathers - and which is a cell of row 0 alone"""
    m, A = _built("row_lengths", last)
    kr = _context(m, fmt, monkeypatch)
    try:
        if fmt != "double":
            _check_balance(kr, _balanced("row_lengths", last), FORMATS[fmt], ("row lengths", last, fmt))
        else:
            _check_csr(kr, 0, A, ("row lengths", last))
        _check_spmv(kr, A, ks.vectors(m.n, last), 0, ("row lengths", last, fmt), from_row=1)
        _check_spmv(kr, A, {"lognormal": ks.vectors(m.n, last)["lognormal"]}, 0, ("row lengths", last, fmt, "row 0 too"))
    finally:
        kr.close()


# ---- 3. few rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ks.FEW_ROWS)
def test_few_rows(n, monkeypatch):
    """fewer than 8 row blocks, n % 4 != 0: the remap's early-outs; every row is written"""
    m, A = _built("few_rows", n)
    vectors = {"lognormal": ks.vectors(n, 50 + n)["lognormal"]}
    for fmt in FORMATS:
        kr = _context(m, fmt, monkeypatch)
        try:
            if fmt != "double":
                _check_balance(kr, _balanced("few_rows", n), FORMATS[fmt], ("few rows", n, fmt))
            _check_spmv(kr, A, vectors, 0, ("few rows", n, fmt))
            if fmt == "double":
                _same(kr.row_sums(), A.dot(np.ones(n)), ("few rows", n, "row sums"))
        finally:
            kr.close()


# ---- 4. format limits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ks.LIMITS))
def test_format_limits(name, monkeypatch):
    """kr_pack16 takes a column offset of 65 535 and a count of 65 535 and refuses 65 536 of either; kr_to_f32 takes 2^24, 2^24 + 2
    and 0.5 and refuses 2^24 + 1 and 0.1.  Whatever the format, nothing changes."""
    m, A = _built("format_limit", name)
    kr = _context(m, "packed", monkeypatch)
    try:
        _check_balance(kr, _balanced("format_limit", name), ks.LIMITS[name][2], name)
        _check_spmv(kr, A, {"lognormal": ks.vectors(m.n, 7)["lognormal"]}, 0, name)
    finally:
        kr.close()


# ---- 5. removal ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["packed", "float"])
def test_removal_of_whole_steps_single_lanes_and_alternate_cells(fmt, monkeypatch):
    """kr_count_kept / kr_compact on rows whose 64-cell steps lose everything, all but lane 0, all but lane 63, alternate cells and
    nothing, and that end on and off a step edge"""
    m, A = _built("removal", False)
    want = _balanced("removal", False, 0.0)
    kr = _context(m, fmt, monkeypatch)
    try:
        removed, val, rem = kr.remove_sparse(0.0)
        assert removed.tolist() == want[1].tolist() == np.sort(m.about["weak"]).tolist() and val == 1.0 and rem == 0
        _check_csr(kr, 1, want[0], "removal")
        _check_csr(kr, 0, A, "removal, the full matrix stays")
        _check_balance(kr, want, FORMATS[fmt], ("removal", fmt))
        _check_spmv(kr, want[0], {"lognormal": ks.vectors(want[0].n, 9)["lognormal"]}, 1, ("removal", fmt))
    finally:
        kr.close()


def test_removal_that_empties_a_kept_row(monkeypatch):
    """a kept locus whose neighbours are all removed: v = 0 there, the first step divides by it, NaN reaches nan_min / nan_max and
    the iteration ends after one outer and one inner step with x all NaN - as in the oracle"""
    m, A = _built("removal", True)
    want = _balanced("removal", True, 0.0)
    assert want[3:5] == (1, 1) and np.isnan(want[2]).all()
    kr = _context(m, "packed", monkeypatch)
    try:
        removed, val, _ = kr.remove_sparse(0.0)
        assert removed.tolist() == want[1].tolist() and val == 1.0
        _check_csr(kr, 1, want[0], "empty reduced row")
        _check_balance(kr, want, 2, "empty reduced row")
        _check_spmv(kr, want[0], {"lognormal": ks.vectors(want[0].n, 10)["lognormal"]}, 1, "empty reduced row")
    finally:
        kr.close()


# ---- 6. long reductions --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dot_context():
    from fithic_amd import _capi
    kr = _capi.KrContext(0)
    yield kr
    kr.close()


@pytest.mark.parametrize("n", ks.DOT_SIZES)
def test_dot_and_sum_around_the_tile_and_buffer_seams(dot_context, n):
    """kr_dot + kr_finish<0>: one tile, 1024 tiles (one LDS buffer), and a second and third buffer of 1, 9 and 10 partials"""
    from oracle import hickry_oracle as ho
    a, b = ks.dot_vectors(n)
    got, want = dot_context.dot(a, b), ho.dot(a, b)
    assert _bits([got])[0] == _bits([want])[0], (n, got, want)
    got, want = dot_context.dot(a), ho.dot(a)
    assert _bits([got])[0] == _bits([want])[0], (n, got, want)


def test_balance_beyond_one_buffer_of_tile_partials(monkeypatch):
    """2^20 + 1033 loci = 1026 tile partials: the sums, minima and maxima of a real iteration go through kr_finish's second buffer"""
    m, A = _built("long_tridiagonal")
    kr = _context(m, "packed", monkeypatch)
    try:
        _check_balance(kr, _balanced("long_tridiagonal"), 2, "long tridiagonal")
    finally:
        kr.close()


# ---- 7. loop exits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ks.LOOP_CASES)
def test_every_exit_of_the_iteration(name, monkeypatch):
    """both kr_gamma selections (delta, Delta), the 10-step and the 30-step cap: which matrix reaches which is asserted on the oracle's
    trace in tests/test_kr_shape_inputs.py"""
    m, A = _built("loop_exit", name)
    kr = _context(m, "packed", monkeypatch)
    try:
        _check_csr(kr, 0, A, name)
        _check_balance(kr, _balanced("loop_exit", name), ks.value_bytes(A), name)
    finally:
        kr.close()
