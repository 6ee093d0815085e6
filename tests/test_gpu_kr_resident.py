"""The Knight-Ruiz matrix assembled from an engine's resident contact rows (fhx_kr_load_pairs_resident, csrc/fhx_kr_resident.inc)
against the file route (hickry.loadfastfithicInteractions -> fhx_kr_load_pairs): the same CSR, row sums, removed rows, reduced
matrix, x, iteration counts and bias, bit for bit.  Contact counts are integers, so a cell's sum is exact in any order: there
is no tolerance anywhere in this file."""
import gzip
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
DATA = os.path.join(GOLDEN, "data")
# (case, the -r it is ingested at): fixed size at the data's resolution; the irregular set with -r 0; the combined-fragments set has
# no grid either: with -r 0, and with -r 40000 as loci off the grid (the engine slots those like -r 0, fhx_k1.hip)
KR_CASES = [("k1_kr_hESC", 40000), ("k1_kr_hESC_default", 40000), ("k2_kr_pfal", 10000), ("k3_kr_imr90", 1000000), ("k4_kr_irregular", 0),
            ("k5_kr_combine", 0), ("k5_kr_combine", 40000)]
TILE = 1024                                            # krd::TILE: keys per tile of the cell scan (2 per row)
KRR_CHUNK = 2048                                       # krd::KRR_CHUNK: rows per workgroup of krr_keys


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _meta(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def _ingest(contacts, frags, resolution):
    """the contacts file into an Engine as the command line does it (tables.load_contacts), the fragment lines in the run's ids"""
    from fithic_amd import tables
    from fithic_amd.engine import Engine
    chroms = tables.ChromIndex()
    eng = Engine(0)                                    # raises without a GPU or the built library: no fallback

    def engine_of():
        eng.configure(resolution)
        return eng
    try:
        con = tables.load_contacts(contacts, chroms, engine_of)
        fc, fm, eng.frag_hits = tables.read_fragments(frags, chroms)
        eng.chroms = chroms
    except BaseException:
        eng.close()
        raise
    return eng, con, fc, fm


def _everything(kr, perc):
    """what the issue compares, from a context whose matrix is loaded"""
    out = dict(shape=kr.shape()[:2], csr=kr.get_csr(0), sums=kr.row_sums())
    removed, val, rem = kr.remove_sparse(perc)
    out.update(removed=removed, val=val, rem=rem, reduced=kr.get_csr(1))
    x, info = kr.balance(1e-6)
    out.update(x=x, iters=(info.outer_iterations, info.inner_iterations, info.matvecs, info.value_bytes), bias=kr.bias())
    return out


def _same(a, b, what):
    assert a["shape"] == b["shape"], what
    for key in ("csr", "reduced"):
        (p1, c1, v1), (p2, c2, v2) = a[key], b[key]
        assert np.array_equal(p1, p2) and np.array_equal(c1, c2) and np.array_equal(_bits(v1), _bits(v2)), (what, key)
    assert np.array_equal(_bits(a["sums"]), _bits(b["sums"])), what
    assert np.array_equal(a["removed"], b["removed"]) and a["val"] == b["val"] and a["rem"] == b["rem"], what
    assert a["iters"] == b["iters"], (what, a["iters"], b["iters"])
    assert np.array_equal(_bits(a["x"]), _bits(b["x"])) and np.array_equal(_bits(a["bias"]), _bits(b["bias"])), what


def _dense(kr):
    n = kr.shape()[0]
    indptr, col, val = kr.get_csr(0)
    dense = np.zeros((n, n))
    for r in range(n):
        dense[r, col[indptr[r]:indptr[r + 1]]] = val[indptr[r]:indptr[r + 1]]
    return dense, indptr, col, val


@pytest.fixture(scope="module")
def file_route():
    """the file route's results per golden case, computed once"""
    from fithic_amd import hickry
    cache = {}

    def get(name):
        if name not in cache:
            meta = _meta(name)
            M, _ = hickry.loadfastfithicInteractions(os.path.join(DATA, meta["contacts"]), os.path.join(DATA, meta["frags"]))
            try:
                cache[name] = _everything(M.kr, meta["perc"])
            finally:
                M.kr.close()
        return cache[name]
    return get


# ---- 1. the golden cases -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,resolution", KR_CASES)
def test_golden_cases_equal_the_file_route(name, resolution, file_route, tmp_path, capsys):
    from fithic_amd import _capi
    meta = _meta(name)
    con_path, frg_path = os.path.join(DATA, meta["contacts"]), os.path.join(DATA, meta["frags"])
    with gzip.open(con_path, "rt") as f:
        fractional = any(float(ln.split()[4]) != int(float(ln.split()[4])) for ln in f)
    assert fractional == (name == "k3_kr_imr90")
    eng, con, fc, fm = _ingest(con_path, frg_path, resolution)
    kr = _capi.KrContext(0)
    try:
        assert hasattr(con, "rows"), "the device parser takes every golden contacts file"
        kr.load_loci(fc, fm)
        if fractional:                                 # 1.7 is not what the rows hold: the C entry refuses
            with pytest.raises(_capi.FhxError) as e:
                kr.load_pairs_resident(eng.ctx)
            assert e.value.code == _capi.FHX_ERR_UNSUPPORTED
            with pytest.raises(_capi.FhxError) as e:
                eng.kr_bias(fc, fm, meta["perc"])
            assert e.value.code == _capi.FHX_ERR_UNSUPPORTED
        else:
            kr.load_pairs_resident(eng.ctx)
            got = _everything(kr, meta["perc"])
            want = file_route(name)
            assert got["shape"] == (meta["n"], meta["nnz"])
            assert got["iters"][:2] == (meta["outer"], meta["inner"])
            _same(got, want, name)
            bias, info = eng.kr_bias(fc, fm, meta["perc"])
            assert np.array_equal(_bits(bias), _bits(want["bias"]))
            assert (info["outer_iterations"], info["inner_iterations"], info["n"]) == (meta["outer"], meta["inner"], meta["n"] - len(want["removed"]))
    finally:
        kr.close()
        eng.close()
    if fractional:                                     # the stage function takes the file route and gives its bias
        from fithic_amd import fithic as F, tables
        out = str(tmp_path / "bias.gz")
        F.reset_session()
        try:
            F.resolution, F.device, F.gpus, F.logfile = resolution, 0, 1, None
            F.read_Interactions(con_path, None)
            capsys.readouterr()
            dic = F.kr_biases(frg_path, meta["perc"], out)
            printed = capsys.readouterr().out
            assert "(contacts file)" in printed and "(resident rows)" not in printed
            assert printed.count("Creating sparse matrix...") == 1
            _, _, back = tables.read_bias(out, tables.ChromIndex())
            assert np.array_equal(_bits(back), _bits(file_route(name)["bias"]))
            assert sum(len(v) for v in dic.values()) == len(set(zip(fc.tolist(), fm.tolist())))
        finally:
            F.reset_session()


# ---- 2. twelve rows written out by hand --------------------------------------------------------------------------------------------
FRAG_LINES = [("chrA", 500), ("chrA", 1500), ("chrA", 2500), ("chrA", 500), ("chrA", 3500), ("chrA", 4500), ("chrB", 500), ("chrB", 1500),
              ("chrB", 2500), ("chrB", 9500)]          # line 3 repeats line 0's locus (the last line wins); no row touches lines 4 and 9
ROWS = [("chrA", 500, "chrA", 1500, 3), ("chrA", 500, "chrA", 1500, 4),            # a duplicated pair
        ("chrA", 1500, "chrA", 2500, 5), ("chrA", 2500, "chrA", 1500, 6),          # the same pair in both orders
        ("chrA", 2500, "chrA", 2500, 7),                                           # the diagonal
        ("chrA", 500, "chrB", 500, 2),                                             # inter-chromosomal
        ("chrA", 4500, "chrB", 1500, 0),                                           # a zero count: a stored zero
        ("chrA", 1500, "chrA", 4500, 70000),                                       # too large for the 4-byte cell
        ("chrB", 500, "chrB", 2500, (1 << 24) + 1),                                # not a binary32 number
        ("chrB", 1500, "chrB", 2500, 1), ("chrA", 500, "chrA", 2500, 9), ("chrB", 500, "chrB", 1500, 8)]


def _hand_matrix():
    want = np.zeros((10, 10))
    for (r, c), v in {(3, 1): 7, (1, 2): 11, (3, 6): 2, (1, 5): 70000, (6, 8): (1 << 24) + 1, (7, 8): 1, (3, 2): 9, (6, 7): 8}.items():
        want[r, c] = want[c, r] = float(v)
    want[2, 2] = 14.0                                  # coo + its transpose doubles the diagonal
    return want


@pytest.mark.parametrize("resolution", [1000, 0])
def test_twelve_rows_by_hand(resolution, tmp_path):
    from fithic_amd import _capi, hickry
    con_path, frg_path = str(tmp_path / "c.gz"), str(tmp_path / "f.gz")
    with gzip.open(con_path, "wt") as f:
        f.write("".join("%s\t%d\t%s\t%d\t%d\n" % r for r in ROWS))
    with gzip.open(frg_path, "wt") as f:
        f.write("".join("%s\t0\t%d\t1\t0\n" % ln for ln in FRAG_LINES))
    assert len(ROWS) == 12
    M, _ = hickry.loadfastfithicInteractions(con_path, frg_path)
    eng, con, fc, fm = _ingest(con_path, frg_path, resolution)
    kr = _capi.KrContext(0)
    try:
        kr.load_loci(fc, fm)
        kr.load_pairs_resident(eng.ctx)
        dense, indptr, col, val = _dense(kr)
        assert np.array_equal(dense, _hand_matrix())
        assert len(val) == 19 and np.count_nonzero(val == 0.0) == 2          # 9 pairs twice + the diagonal cell; the zero count is stored
        assert not dense[0].any() and not dense[4].any() and not dense[9].any()
        f_indptr, f_col, f_val = M.kr.get_csr(0)
        assert np.array_equal(indptr, f_indptr) and np.array_equal(col, f_col) and np.array_equal(_bits(val), _bits(f_val))
        assert np.array_equal(_bits(kr.row_sums()), _bits(M.kr.row_sums()))
    finally:
        kr.close()
        eng.close()
        M.kr.close()


# ---- 3. a locus that is no fragment line -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("resolution", [1000, 0])
def test_unknown_locus_names_the_first_row_of_the_file(reverse, resolution, tmp_path):
    from fithic_amd import _capi, hickry
    n_rows, n_loci, gone = 70_000, 400, (17, 233)      # rows 300 and 65 999 name a locus the fragments file lacks
    assert n_rows > 4 * KRR_CHUNK and 2 * n_rows > 4 * TILE
    rng = np.random.default_rng(3)
    ok = np.setdiff1d(np.arange(n_loci), gone)
    a, b = rng.choice(ok, n_rows), rng.choice(ok, n_rows)
    a[300], b[65_999] = gone[0], gone[1]
    cnt = rng.integers(1, 50, n_rows)
    order = np.arange(n_rows)[::-1] if reverse else np.arange(n_rows)
    first = int(np.flatnonzero(np.isin(a[order], gone) | np.isin(b[order], gone))[0])
    assert first == (n_rows - 1 - 65_999 if reverse else 300)
    con_path, frg_path = str(tmp_path / "c.gz"), str(tmp_path / "f.gz")
    with gzip.open(con_path, "wt", compresslevel=1) as f:
        f.write("".join("chr1\t%d\tchr1\t%d\t%d\n" % (a[i] * 1000 + 500, b[i] * 1000 + 500, cnt[i]) for i in order))
    with gzip.open(frg_path, "wt") as f:
        f.write("".join("chr1\t0\t%d\t1\t0\n" % (k * 1000 + 500) for k in ok))
    with pytest.raises(KeyError) as e:
        hickry.loadfastfithicInteractions(con_path, frg_path)
    assert e.value.args == (first,)
    eng, con, fc, fm = _ingest(con_path, frg_path, resolution)
    kr = _capi.KrContext(0)
    try:
        kr.load_loci(fc, fm)
        with pytest.raises(KeyError) as e:
            kr.load_pairs_resident(eng.ctx)
        assert e.value.args == (first,)
        with pytest.raises(KeyError) as e:
            eng.kr_bias(fc, fm)
        assert e.value.args == (first,)
    finally:
        kr.close()
        eng.close()


def test_unknown_locus_is_named_by_its_file_position():
    """rows loaded out of file order with their positions (set_global_rows): the KeyError names the file row, as the file route does"""
    from fithic_amd import _capi
    from fithic_amd.engine import Engine
    n = 5000
    rng = np.random.default_rng(4)
    a, b = rng.integers(0, 50, n), rng.integers(0, 50, n)
    a[[40, 4100]] = 60                                 # locus 60 is no fragment line; file rows 40 and 4100 name it
    order = rng.permutation(n)
    zeros = np.zeros(n, np.int32)
    eng, kr = Engine(0), _capi.KrContext(0)
    try:
        eng.configure(1000)
        eng.load_contacts(zeros, (a * 1000 + 500)[order], zeros, (b * 1000 + 500)[order], np.ones(n, np.int32))
        kr.load_loci(np.zeros(50, np.int32), np.arange(50) * 1000 + 500)
        with pytest.raises(KeyError) as e:
            kr.load_pairs_resident(eng.ctx)
        assert e.value.args == (int(np.flatnonzero(np.isin(order, [40, 4100]))[0]),)       # no positions: the loaded row
        eng.ctx.set_global_rows(order)
        with pytest.raises(KeyError) as e:
            kr.load_pairs_resident(eng.ctx)
        assert e.value.args == (40,)
    finally:
        kr.close()
        eng.close()


# ---- 4. sizes around the tiles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resolution", [1000, 0])
@pytest.mark.parametrize("n_rows", [1, TILE // 2 - 1, TILE // 2, TILE // 2 + 1, TILE + 1, KRR_CHUNK - 1, KRR_CHUNK, KRR_CHUNK + 1])
def test_sizes_around_the_tiles(n_rows, resolution):
    """int32 columns (fhx_load_pairs: integers by construction) over two chromosomes; the file route is given the same rows as doubles"""
    from fithic_amd import _capi
    from fithic_amd.engine import Engine
    rng = np.random.default_rng(n_rows)
    n_loci = 90
    c1, c2 = rng.integers(0, 2, n_rows).astype(np.int32), rng.integers(0, 2, n_rows).astype(np.int32)
    m1, m2 = (rng.integers(0, n_loci, n_rows) * 1000 + 500).astype(np.int32), (rng.integers(0, n_loci, n_rows) * 1000 + 500).astype(np.int32)
    cnt = rng.integers(0, 100_000, n_rows).astype(np.int32)
    fc = np.repeat(np.arange(2, dtype=np.int32), n_loci)
    fm = np.tile(np.arange(n_loci, dtype=np.int32) * 1000 + 500, 2)
    eng, kr, ref = Engine(0), _capi.KrContext(0), _capi.KrContext(0)
    try:
        eng.configure(resolution)
        eng.load_contacts(c1, m1, c2, m2, cnt)
        for k in (kr, ref):
            k.load_loci(fc, fm)
        kr.load_pairs_resident(eng.ctx)
        ref.load_pairs(c1, m1, c2, m2, cnt.astype(np.float64))
        assert kr.shape() == ref.shape()
        for got, want in zip(kr.get_csr(0), ref.get_csr(0)):
            assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
        assert np.array_equal(_bits(kr.row_sums()), _bits(ref.row_sums()))
    finally:
        ref.close()
        kr.close()
        eng.close()


def test_arguments_the_entry_refuses():
    from fithic_amd import _capi
    from fithic_amd.engine import Engine
    eng, kr, host = Engine(0), _capi.KrContext(0), _capi.Context(-1)
    try:
        eng.configure(1000)
        kr.load_loci([0, 0], [500, 1500])
        for ctx in (eng.ctx, host):                    # no rows loaded; a host-only context
            with pytest.raises(_capi.FhxError) as e:
                kr.load_pairs_resident(ctx)
            assert e.value.code == _capi.FHX_ERR_ARG
        eng.load_contacts([0], [500], [0], [1500], [3])
        fresh = _capi.KrContext(0)                     # load_loci has not run
        try:
            with pytest.raises(_capi.FhxError) as e:
                fresh.load_pairs_resident(eng.ctx)
            assert e.value.code == _capi.FHX_ERR_ARG
        finally:
            fresh.close()
        kr.load_pairs_resident(eng.ctx)
        assert kr.shape()[:2] == (2, 2)
    finally:
        host.close()
        kr.close()
        eng.close()


# ---- 5. after passes ---------------------------------------------------------------------------------------------------------------
def test_rows_the_passes_skip_still_count(file_route):
    """two passes on the hESC set under -x intraOnly with a p column that makes every 50th row an outlier: the skip mask hides those
    rows from the next pass, not from the matrix - and the pass state is what it was"""
    name = "k1_kr_hESC"
    meta = _meta(name)
    eng, con, fc, fm = _ingest(os.path.join(DATA, meta["contacts"]), os.path.join(DATA, meta["frags"]), 40000)
    try:
        eng.load_fragments(fc, fm, eng.frag_hits, eng.chroms.sort_rank())
        out = eng.run_pass()
        n = len(con)
        p = np.ones(n)
        p[::50] = 0.0                                  # below every 1/N threshold
        eng.ctx.copy(eng.ctx.device_ptr(0), p.ctypes.data, 8 * n, 0)
        assert eng.next_pass() == len(p[::50])
        skip = eng.ctx.fetch_flags(n, outlier=False, skip=True)[1]
        assert int(skip.sum()) == len(p[::50])
        second = eng.run_pass()
        assert second.stats["in_range_count"] < out.stats["in_range_count"]          # the second pass did skip them
        before = eng.fetch(p=True, q=True)
        bias, info = eng.kr_bias(fc, fm, meta["perc"])
        assert np.array_equal(_bits(bias), _bits(file_route(name)["bias"]))
        after = eng.fetch(p=True, q=True)
        assert np.array_equal(_bits(before["p"]), _bits(after["p"])) and np.array_equal(_bits(before["q"]), _bits(after["q"]))
        assert np.array_equal(eng.ctx.fetch_flags(n, outlier=False, skip=True)[1], skip)
        assert eng.ctx.stats().as_dict() == second.stats
    finally:
        eng.close()


# ---- 6. the fraction bit -----------------------------------------------------------------------------------------------------------
def _members(path, chunks):
    """a gzip file of one member per chunk of text"""
    with open(path, "wb") as f:
        for text in chunks:
            f.write(gzip.compress(text.encode(), 1))


def test_integers_as_written_are_accepted_and_one_fraction_refuses(tmp_path):
    from fithic_amd import _capi
    rng = np.random.default_rng(6)
    n_rows, n_loci = 3000, 60
    a, b = rng.integers(0, n_loci, n_rows), rng.integers(0, n_loci, n_rows)
    cnt = rng.integers(0, 500, n_rows)
    frg_path = str(tmp_path / "f.gz")
    with gzip.open(frg_path, "wt") as f:
        f.write("".join("chr1\t0\t%d\t1\t0\n" % (k * 1000 + 500) for k in range(n_loci)))

    def lines(fmt, special=None):
        out = ["chr1\t%d\tchr1\t%d\t%s\n" % (a[i] * 1000 + 500, b[i] * 1000 + 500, fmt % cnt[i]) for i in range(n_rows)]
        if special is not None:
            i, text = special
            out[i] = "chr1\t%d\tchr1\t%d\t%s\n" % (a[i] * 1000 + 500, b[i] * 1000 + 500, text)
        return out

    def load(name, rows, cuts=(1000, 2000)):
        path = str(tmp_path / name)
        _members(path, ["".join(rows[lo:hi]) for lo, hi in zip((0,) + cuts, cuts + (len(rows),))])
        eng, con, fc, fm = _ingest(path, frg_path, 1000)
        kr = _capi.KrContext(0)
        try:
            assert hasattr(con, "rows") and len(con) == n_rows
            assert np.array_equal(con.count, cnt if name.startswith("int") else np.where(np.arange(n_rows) == special_row, cnt_special, cnt))
            kr.load_loci(fc, fm)
            kr.load_pairs_resident(eng.ctx)
            return kr.get_csr(0)
        finally:
            kr.close()
            eng.close()

    special_row, cnt_special = None, None
    want = None
    for k, fmt in enumerate(["%d", "%d.0", "%d.", "0%d.000"]):
        got = load("int%d.gz" % k, lines(fmt))
        if want is None:
            want = got
        for g, w in zip(got, want):
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), fmt
    assert len(want[2]) > 0
    # one count with a non-zero fractional digit: in the first line, in the middle, in the last line of the last member (with and
    # without its newline), and behind zeros
    for special_row, text, cnt_special in [(0, "3.5", 3), (1500, "7.25", 7), (n_rows - 1, "3.5", 3), (n_rows - 1, "0.001", 0), (17, "12.0000000000001", 12)]:
        rows = lines("%d", (special_row, text))
        for strip in (False, True):
            if strip:
                if special_row != n_rows - 1:
                    continue
                rows[-1] = rows[-1].rstrip("\n")
            with pytest.raises(_capi.FhxError) as e:
                load("frac.gz", rows)
            assert e.value.code == _capi.FHX_ERR_UNSUPPORTED, (special_row, text, strip)
    # and the refusal does not stick to the context's successors: int32 columns are integers again
    from fithic_amd.engine import Engine
    eng, kr = Engine(0), _capi.KrContext(0)
    try:
        eng.configure(1000)
        eng.load_contacts([0], [500], [0], [1500], [3])
        kr.load_loci([0, 0], [500, 1500])
        kr.load_pairs_resident(eng.ctx)
    finally:
        kr.close()
        eng.close()
