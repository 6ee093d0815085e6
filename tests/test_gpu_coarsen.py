"""GPU tests of the coarsening (fithic_amd.coarsen, csrc/fhx_coarsen.hip): the fetched columns, the counts and the decompressed
bytes of both written files equal the model's (tests/coarsen_model.py, pinned by hand in test_coarsen_model.py) - on row counts
around the 256-row blocks and the 1024-key scan tiles, for every factor in both modes with the diagonal kept and dropped, on one
cell that holds every row and on rows that share no cell; sums at the int32 edge; every refusal names the smallest row and leaves
the handle empty; a path, host columns and a resident producer give the same cells; and three chains hold the step to what the
tree already computes: the HiC-Pro model on a summed matrix, the fragment binning on every N-th cut, validPairs at N*R.  Then the
cells go into an Engine, and the command line writes the same files."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import coarsen_model as cm
import fragpairs_model as fm
import hicpro_model as hm
import validpairs_model as vm
from conftest import DATA, ROOT, bits_equal
from test_gpu_fragpairs import _pairs_over, bed_of

pytestmark = pytest.mark.gpu

INT32_MAX = (1 << 31) - 1
NAMES = ["chrB", "chrA", "chrC"]
FACTORS = [1, 2, 3, 10, 64]


def _gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def _chroms(names=NAMES):
    from fithic_amd import tables
    chroms = tables.ChromIndex()
    for n in names:
        chroms.intern(n)
    return chroms


def grid_table(sizes, resolution):
    """chromosome c has sizes[c] bins from 0 on, every 7th bin of the grid missing when there are more than 7; hits = the bin number % 5"""
    c, m, h = [], [], []
    for ch, n in enumerate(sizes):
        bins = [k for k in range(2 * n) if n <= 7 or k % 7 != 6][:n]
        c += [ch] * n
        m += [k * resolution + resolution // 2 for k in bins]
        h += [k % 5 for k in bins]
    return np.array(c, np.int32), np.array(m, np.int32), np.array(h, np.int32)


def meta_table(sizes, seed=1):
    """chromosome c has sizes[c] fragment ends at irregular distances"""
    rng = np.random.default_rng(seed)
    c = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    m = np.concatenate([np.cumsum(rng.integers(1, 900, n)) for n in sizes]).astype(np.int32)
    return c, m, rng.integers(0, 4, len(m)).astype(np.int32)


def random_rows(table, n, seed, top=1000):
    """n rows over the loci of a table, either end first; a fifth of the counts are zero"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, len(table[1]), n), rng.integers(0, len(table[1]), n)
    near = rng.random(n) < 0.5                                        # half of the rows near the diagonal: cells that are hit often
    b = np.where(near, np.clip(a + rng.integers(-3, 4, n), 0, len(table[1]) - 1), b)
    count = np.where(rng.random(n) < 0.2, 0, rng.integers(0, top, n))
    return [table[0][a], table[1][a], table[0][b], table[1][b], count.astype(np.int32)]


def check(table, rows, factor, resolution, diagonal, tmp_path, names=NAMES):
    """the device path against the model: columns, counts, the coarse table and both written files -> the cells"""
    from fithic_amd import coarsen
    coarse, want, counts = cm.coarsen(table, rows, factor, resolution, diagonal)
    con, frag = str(tmp_path / "c.gz"), str(tmp_path / "f.gz")
    with coarsen.read(tuple(rows), table, factor, resolution, _chroms(names), diagonal=diagonal) as got:
        assert got.names == names and got.resolution == factor * resolution and len(got) == len(want)
        for k, g in enumerate(got.contacts()):
            assert g.dtype == np.int32 and np.array_equal(g, np.array([c[k] for c in want], np.int32)), (k, factor, resolution, diagonal)
        assert got.counts() == counts
        assert [v.tolist() for v in got.fragments()] == [[t[k] for t in coarse] for k in range(3)]
        assert set(got.stage_seconds()) == {"upload", "keys", "sort", "heads_sums", "cells", "plan"}
        got.write(con)
        got.write_fragments(frag)
    assert _gunzip(con) == cm.contacts_text(names, want)
    assert _gunzip(frag) == cm.fragments_text(names, coarse, factor * resolution)
    return want


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resolution", [10, 0])
@pytest.mark.parametrize("n", [0, 1, 2, 1023, 1024, 1025, 4097])
def test_cells_equal_the_model_for_every_factor_and_both_diagonal_settings(n, resolution, tmp_path):
    table = grid_table([40, 40, 40], resolution) if resolution else meta_table([40, 40, 40])
    assert len(table[0]) == 120
    rows = random_rows(table, n, 100 + n)
    sizes = set()
    for factor in FACTORS:
        kept = check(table, rows, factor, resolution, True, tmp_path)
        dropped = check(table, rows, factor, resolution, False, tmp_path)
        assert len(dropped) <= len(kept) <= n
        sizes.add(len(kept))
    assert n < 1000 or len(sizes) == len(FACTORS)                     # every factor gave another number of cells


def test_70000_rows_in_one_cell_sum_exactly(tmp_path):
    table = meta_table([50, 70])
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, 50, 70000), rng.integers(50, 120, 70000)
    a, b = np.where(np.arange(70000) % 3 == 0, b, a), np.where(np.arange(70000) % 3 == 0, a, b)      # either end first
    count = rng.integers(0, 30000, 70000).astype(np.int32)
    rows = [table[0][a], table[1][a], table[0][b], table[1][b], count]
    got = check(table, rows, 128, 0, True, tmp_path, NAMES[:2])       # one locus per chromosome: the trans cell holds every row
    assert got == [(0, int(table[1][49]), 1, int(table[1][119]), int(count.astype(np.int64).sum()))] and got[0][4] > 10**9
    assert check(table, rows, 128, 0, False, tmp_path, NAMES[:2]) == got
    same = [table[0][a], table[1][a], table[0][a], table[1][a], count]          # ... and the diagonal cell does, kept or dropped
    assert len(check(table, same, 128, 0, True, tmp_path, NAMES[:2])) == 2
    assert check(table, same, 128, 0, False, tmp_path, NAMES[:2]) == []


def test_70000_rows_with_a_cell_each(tmp_path):
    table = grid_table([5, 400], 100)
    n_loci = len(table[1])
    i, j = np.triu_indices(n_loci)
    pick = np.random.default_rng(4).permutation(len(i))[:70000]
    flip = pick % 2 == 0
    a, b = np.where(flip, j[pick], i[pick]), np.where(flip, i[pick], j[pick])
    rows = [table[0][a], table[1][a], table[0][b], table[1][b], (pick % 1000).astype(np.int32)]
    assert len(check(table, rows, 1, 100, True, tmp_path, NAMES[:2])) == 70000
    assert len(check(table, rows, 3, 100, False, tmp_path, NAMES[:2])) < 70000


@pytest.mark.parametrize("resolution", [6, 0])
def test_chromosomes_of_1_and_4097_loci(resolution, tmp_path):
    if resolution:
        table = (np.r_[0, np.ones(4097)].astype(np.int32), np.r_[3, np.arange(4097) * 6 + 3].astype(np.int32), np.ones(4098, np.int32))
    else:
        table = meta_table([1, 4097])
    rows = random_rows(table, 3000, 5)
    rows = [np.r_[v, w] for v, w in zip(rows, [[0, 1], [table[1][0], table[1][4097]], [1, 0], [table[1][1], table[1][0]], [7, 9]])]
    for factor in (3, 4097, 4098):
        check(table, rows, factor, resolution, True, tmp_path, NAMES[:2])


# ---- 2. sums -----------------------------------------------------------------------------------------------------------------
def _context(table, factor, resolution):
    from fithic_amd import _capi, coarsen
    p = coarsen.plan(*table, factor, resolution)
    cz = _capi.CzContext(0)
    cz.load_plan(*p.device_tables(), p.chr, p.mid)
    return cz


SUM_TABLE = ([0, 0, 0, 0, 1], [5, 15, 25, 35, 5], [1] * 5)            # with N = 2, R = 10: loci 0 = (0, 10), 1 = (0, 30), 2 = (1, 10)


def test_a_cell_of_exactly_int32_max_is_taken_and_one_more_is_refused(tmp_path):
    from fithic_amd import _capi, coarsen
    rows = [(0, 5, 0, 25, INT32_MAX - 10), (0, 35, 0, 15, 3), (0, 5, 1, 5, 1), (0, 15, 0, 35, 7)]
    cols = [np.array(v, np.int32) for v in zip(*rows)]
    got = check(SUM_TABLE, cols, 2, 10, True, tmp_path, NAMES[:2])
    assert got == [(0, 10, 0, 30, INT32_MAX), (0, 10, 1, 10, 1)]
    cols[4][1] += 1                                                   # 2^31
    with pytest.raises(cm.Refused) as want:
        cm.coarsen(SUM_TABLE, cols, 2, 10)
    cz = _context(SUM_TABLE, 2, 10)
    try:
        with pytest.raises(_capi.CzRefused) as e:
            cz.coarsen_host(*cols)
        assert (e.value.why, e.value.row) == (cm.SUM, (0 << 32) | 1) == (want.value.why, want.value.row)
        assert e.value.code == _capi.FHX_ERR_UNSUPPORTED and "2147483648" in str(e.value)
        assert cz.n_cells == 0 and cz.device_ptrs() == [0] * 5 and cz.counts() == dict(rows=0, diagonal=0, cells=0)
    finally:
        cz.close()
    with pytest.raises(ValueError, match=r"the cell chrB:10 x chrB:30 sum to more than 2\^31 - 1"):
        coarsen.read(tuple(cols), SUM_TABLE, 2, 10, _chroms())


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------
def _refused(cz, cols, diagonal=True):
    from fithic_amd import _capi
    with pytest.raises(_capi.CzRefused) as e:
        cz.coarsen_host(*cols, diagonal=diagonal)
    assert e.value.code == _capi.FHX_ERR_UNSUPPORTED
    assert cz.n_cells == 0 and cz.device_ptrs() == [0] * 5 and cz.counts() == dict(rows=0, diagonal=0, cells=0)
    return e.value.why, e.value.row


def test_refusals_name_the_smallest_row_and_leave_the_handle_empty(tmp_path):
    from fithic_amd import coarsen
    table = grid_table([40, 40, 40], 10)
    good = random_rows(table, 4097, 6)
    want, counts = cm.coarsen(table, good, 3, 10)[1:]
    cz = _context(table, 3, 10)
    try:
        for row in (0, 1023, 4096):
            for column, value in ((1, 7), (3, 10 * 1000 + 5), (0, 3), (2, -1)):          # off the grid, beyond the last bin, no such chromosome
                bad = [v.copy() for v in good]
                bad[column][row] = value
                assert _refused(cz, bad) == (cm.LOCUS, row)
        bad = [v.copy() for v in good]
        bad[4][1023] = -1
        assert _refused(cz, bad) == (cm.COUNT, 1023)
        bad[1][1024] = 7                                              # an unknown locus behind the negative count, then in front of it
        assert _refused(cz, bad) == (cm.COUNT, 1023)
        bad[1][1022] = 7
        assert _refused(cz, bad) == (cm.LOCUS, 1022)
        bad[4][3] = -5
        assert _refused(cz, bad, diagonal=False) == (cm.COUNT, 3)
        with pytest.raises(cm.Refused) as e:
            cm.coarsen(table, bad, 3, 10, False)
        assert (e.value.why, e.value.row) == (cm.COUNT, 3)
        assert cz.coarsen_host(*good) == len(want)                    # a good call on the same handle
        for k, g in enumerate(cz.fetch_cells()):
            assert np.array_equal(g, np.array([c[k] for c in want], np.int32))
        assert cz.counts() == counts
        cz.reset()
        assert cz.device_ptrs() == [0] * 5 and cz.counts() == dict(rows=0, diagonal=0, cells=0)
        assert cz.coarsen_host(*good, diagonal=False) == cm.coarsen(table, good, 3, 10, False)[2]["cells"]     # the plan stayed
    finally:
        cz.close()
    bad = [v.copy() for v in good]
    bad[0][1023], bad[1][1023], bad[2][1023], bad[3][1023], bad[4][1023] = 1, 7, 2, 15, 3
    with pytest.raises(ValueError, match=r"row 1023 \(chrA:7 chrC:15 count 3\): an end that is no locus of the fragments table"):
        coarsen.read(tuple(bad), table, 3, 10, _chroms())


def test_two_runs_give_the_same_bytes(tmp_path):
    from fithic_amd import coarsen
    table = meta_table([40, 40, 40])
    rows = random_rows(table, 20000, 7)
    files = []
    for k in range(2):
        with coarsen.read(tuple(rows), table, 3, 0, _chroms(), diagonal=False) as got:
            got.write(str(tmp_path / ("%d.gz" % k)))
        with open(str(tmp_path / ("%d.gz" % k)), "rb") as f:
            files.append(f.read())
    assert files[0] == files[1] and len(gzip.decompress(files[0])) > 10000


# ---- 4, 5, 9. the HiC-Pro chain: sources, bytes, the command line ----------------------------------------------------------------
def coarse_hicpro(bed, matrix, factor):
    """a bed and a raw matrix summed onto the factor-fold grid with numpy, in (i, j) order with i <= j -> (bed bytes, matrix bytes, R')"""
    lines = [l.split() for l in hm.text_lines(bed)]
    res = int(lines[0][2]) - int(lines[0][1])
    big = res * factor
    index_of, coarse_of, out_bed = {}, {}, []
    for name, start, _, index in sorted(lines, key=lambda t: int(t[3])):
        key = (name, int(start) // big * big)
        if key not in index_of:
            index_of[key] = len(index_of) + 1
            out_bed.append("%s\t%d\t%d\t%d\n" % (name, key[1], key[1] + big, index_of[key]))
        coarse_of[int(index)] = index_of[key]
    assert [k for k in index_of] == sorted(index_of, key=lambda k: ([n for n, *_ in lines].index(k[0]), k[1]))     # the bed is in table order
    t = np.array([l.split() for l in hm.text_lines(matrix)])
    i, j = (np.array([coarse_of[int(v)] for v in t[:, k]], np.int64) for k in (0, 1))
    i, j = np.minimum(i, j), np.maximum(i, j)
    count = np.array([int(float(v)) for v in t[:, 2]], np.int64)
    order = np.lexsort((j, i))
    heads = np.flatnonzero(np.r_[True, (i[order][1:] != i[order][:-1]) | (j[order][1:] != j[order][:-1])])
    sums = np.add.reduceat(count[order], heads)
    out_matrix = "".join("%d\t%d\t%d\n" % (a, b, s) for a, b, s in zip(i[order][heads].tolist(), j[order][heads].tolist(), sums.tolist()))
    return "".join(out_bed).encode(), out_matrix.encode(), big


@pytest.fixture(scope="module")
def hp2(tmp_path_factory):
    """hp2's bed and matrix as files, the fine files the converter writes for them, and the bytes of the inputs"""
    from fithic_amd import hicpro
    tmp = tmp_path_factory.mktemp("hp2")
    case = hm.CASES["hp2_r0"]
    bed, matrix, _ = hm.case_inputs(case, tmp)
    con, frag = str(tmp / "fine.contacts.gz"), str(tmp / "fine.fragments.gz")
    hicpro.outputfithicform(bed, matrix, con, frag, None, None, 0)
    return dict(bed=bed, matrix=matrix, contacts=con, fragments=frag, bed_bytes=hm.fixture_bytes(case["bed"]),
                matrix_bytes=hm.fixture_bytes(case["matrix"]))


def hp2_model(hp2, factor):
    bed, matrix, big = coarse_hicpro(hp2["bed_bytes"], hp2["matrix_bytes"], factor)
    model = hm.Model(bed, matrix, None, big)
    return model.contacts_text().encode(), model.fragments_text().encode(), big


@pytest.mark.parametrize("factor", [2, 7])                            # chromosomes of 120, 100 and 80 bins: 7 leaves short last groups
def test_hicpro_rows_coarsened_are_the_model_s_files_of_the_summed_matrix(factor, hp2, tmp_path):
    from fithic_amd import coarsen, hicpro
    want_contacts, want_fragments, big = hp2_model(hp2, factor)
    assert want_fragments.count(b"\n") == sum(-(-n // factor) for n in (120, 100, 80))
    con, frag = str(tmp_path / "c.gz"), str(tmp_path / "f.gz")
    with hicpro.read(hp2["bed"], hp2["matrix"]) as fine:
        with coarsen.read(fine, fine.fragments, factor, 10000) as got:          # HBM to HBM
            assert got.resolution == big and got.names == ["chrA", "chrB", "chrC"] and got.counts()["rows"] == 40000
            got.write(con)
            got.write_fragments(frag)
    assert _gunzip(con) == want_contacts and _gunzip(frag) == want_fragments


def test_a_path_host_columns_and_a_resident_producer_give_the_same_cells(hp2, tmp_path):
    from fithic_amd import coarsen, hicpro, tables
    want_contacts, want_fragments, _ = hp2_model(hp2, 3)
    with hicpro.read(hp2["bed"], hp2["matrix"]) as fine:
        chroms = tables.ChromIndex()
        triple = tables.read_fragments(hp2["fragments"], chroms)
        sources = {"path": (hp2["contacts"], hp2["fragments"], None), "columns": (tuple(fine.contacts()), triple, chroms),
                   "resident": (fine, hp2["fragments"], None), "resident, triple": (fine, fine.fragments, None)}
        for kind, (source, fragments, index) in sources.items():
            con, frag = str(tmp_path / "c.gz"), str(tmp_path / "f.gz")
            with coarsen.read(source, fragments, 3, 10000, index) as got:
                got.write(con)
                got.write_fragments(frag)
            assert _gunzip(con) == want_contacts and _gunzip(frag) == want_fragments, kind


def test_command_line_writes_the_same_files_and_a_refused_input_leaves_none(hp2, tmp_path):
    from fithic_amd import coarsen
    want_contacts, want_fragments, _ = hp2_model(hp2, 2)
    r = subprocess.run([sys.executable, "-m", "fithic_amd.coarsen", "-i", hp2["contacts"], "-f", hp2["fragments"], "-r", "10000", "-n", "2",
                        "-o", str(tmp_path), "-l", "lib"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines()[0] == "The new resolution is 20000"
    assert _gunzip(str(tmp_path / "lib_x2.contactCounts.gz")) == want_contacts
    assert _gunzip(str(tmp_path / "lib_x2.fragments.gz")) == want_fragments
    bad = str(tmp_path / "bad.contacts.gz")
    with gzip.open(bad, "wb") as f:
        f.write(_gunzip(hp2["contacts"]) + b"chrA\t5000\tchrB\t5001\t4\n")
    out = tmp_path / "out"
    out.mkdir()
    with pytest.raises(ValueError, match=r"row 40000 \(chrA:5000 chrB:5001 count 4\)"):
        coarsen.main(["-i", bad, "-f", hp2["fragments"], "-r", "10000", "-n", "2", "-o", str(out)])
    with pytest.raises(ValueError, match="resolution 0"):
        coarsen.main(["-i", hp2["contacts"], "-f", hp2["fragments"], "-r", "3000", "-n", "2", "-o", str(out)])
    assert os.listdir(str(out)) == []


# ---- 6. meta-fragments against the fragment binning on every N-th cut ---------------------------------------------------------------
def _digest_table(sizes, seed=8):
    rng = np.random.default_rng(seed)
    return [(b"ctg%d" % k, np.cumsum(rng.integers(150, 700, n)).tolist()) for k, n in enumerate(sizes)]


def _every_nth(table, factor):
    """the ends of every factor-th fragment and of every contig's last"""
    return [(name, ends[factor - 1::factor] + ([ends[-1]] if len(ends) % factor else [])) for name, ends in table]


@pytest.fixture(scope="module")
def meta_files(tmp_path_factory):
    """contigs of 1, 9, 10, 11 and 25 fragments (and two long ones, for the pass of test 8) binned to single fragments, then taken to
    meta-fragments of 10: the coarse files, and what fragpairs gives on every 10th cut"""
    from fithic_amd import coarsen, fragpairs
    tmp = tmp_path_factory.mktemp("meta")
    table = _digest_table([1, 9, 10, 11, 25, 400, 300])
    coarse_table = _every_nth(table, 10)
    assert [len(e) for _, e in coarse_table] == [1, 1, 1, 2, 3, 40, 30]
    pairs = _pairs_over(table, 40000, 9)
    src, bed, coarse_bed = str(tmp / "s.allValidPairs"), str(tmp / "fine.bed"), str(tmp / "coarse.bed")
    for path, data in ((src, pairs), (bed, bed_of(table)), (coarse_bed, bed_of(coarse_table))):
        with open(path, "wb") as f:
            f.write(data)
    triple = (np.repeat(np.arange(len(table)), [len(e) for _, e in table]).astype(np.int32),
              np.array([e for _, ends in table for e in ends], np.int32), np.ones(sum(len(e) for _, e in table), np.int32))
    con, frag = str(tmp / "meta.contacts.gz"), str(tmp / "meta.fragments.gz")
    with fragpairs.read(src, bed) as fine:
        fine_cols = fine.contacts()
        with coarsen.read(fine, triple, 10, 0, diagonal=False) as got:
            cols, counts, names = got.contacts(), got.counts(), got.names
            got.write(con)
            got.write_fragments(frag)
    with fragpairs.read(src, coarse_bed) as direct:
        want, want_counts = direct.contacts(), direct.counts()
    return dict(table=table, coarse_table=coarse_table, pairs=pairs, triple=triple, fine_cols=fine_cols, cols=cols, counts=counts, names=names,
                want=want, want_counts=want_counts, contacts=con, fragments=frag, src=src, bed=bed)


def test_meta_fragments_of_ten_are_the_fragment_binning_on_every_tenth_cut(meta_files):
    m = meta_files
    assert m["names"] == ["chr%d" % (k + 1) for k in range(7)]
    assert m["counts"]["cells"] == m["want_counts"]["cells"] > 1000
    for got, want in zip(m["cols"], m["want"]):
        assert got.dtype == np.int32 and np.array_equal(got, want)
    assert int(m["cols"][4].astype(np.int64).sum()) == m["want_counts"]["pairs"]
    assert m["counts"]["rows"] == len(m["fine_cols"][0])
    # the model says the same on the CPU side
    coarse, cells, _ = cm.coarsen(m["triple"], fm.columns(m["pairs"], m["table"]), 10, 0, diagonal=False)
    assert cells == fm.cells(m["pairs"], m["coarse_table"])[0]
    assert [(c, mid) for c, mid, _ in coarse] == [(c, e) for c, (_, ends) in enumerate(m["coarse_table"]) for e in ends]
    assert _gunzip(m["contacts"]) == fm.text(m["pairs"], m["coarse_table"])
    assert _gunzip(m["fragments"]) == b"".join(b"chr%d\t0\t%d\t%d\t1\n" % (c + 1, e, min(10, len(m["table"][c][1]) - 10 * k))
                                               for c, (_, ends) in enumerate(m["coarse_table"]) for k, e in enumerate(ends))


# ---- 7. the grid against validPairs at N * R -----------------------------------------------------------------------------------------
def test_validpairs_at_r_coarsened_are_validpairs_at_n_r(tmp_path):
    from fithic_amd import coarsen, validpairs
    res, factor = 10, 3
    rng = np.random.default_rng(10)
    lines = []
    for k in range(6000):
        a, b = rng.integers(1, 4, 2) if rng.random() < 0.3 else [rng.integers(1, 4)] * 2
        p = int(rng.integers(0, 900))
        # the script keeps a cis pair when distance^2 > 2 * resolution, in front of the binning: closer than that at R, or kept at N * R too
        d = int(rng.integers(0, 5)) if rng.random() < 0.2 else int(rng.integers(8, 300))
        q = int(rng.integers(0, 900)) if a != b else p + d
        if rng.random() < 0.5:
            a, p, b, q = b, q, a, p
        lines.append(b"r%d\tchr%d\t%d\t+\tchr%d\t%d\t-\n" % (k, a, p, b, q))
    data = b"".join(lines)
    fine_pairs, coarse_pairs = vm.pairs(data, res), vm.pairs(data, res * factor)
    assert len(fine_pairs) == len(coarse_pairs) and 4000 < len(fine_pairs) < 6000          # the filter dropped the same lines, and some
    src = str(tmp_path / "in.allValidPairs")
    with open(src, "wb") as f:
        f.write(data)

    def oriented(names, cols):
        rows = []
        for c1, m1, c2, m2, n in zip(*[np.asarray(v).tolist() for v in cols]):
            a, b = sorted([(names[c1], m1), (names[c2], m2)])
            rows.append(a + b + (n,))
        return sorted(rows)

    with validpairs.read(src, res * factor) as direct:
        want = oriented(direct.names, direct.contacts())
    with validpairs.read(src, res) as fine:
        n_bins = 1300 // res
        table = (np.repeat(np.arange(len(fine.names)), n_bins).astype(np.int32),
                 np.tile(np.arange(n_bins) * res + res // 2, len(fine.names)).astype(np.int32), np.ones(n_bins * len(fine.names), np.int32))
        with coarsen.read(fine, table, factor, res) as got:
            assert got.resolution == res * factor and got.counts()["rows"] == len(fine)
            assert oriented(got.names, got.contacts()) == want
    names, *cols = vm.columns(data, res * factor)
    assert want == oriented(names, cols)
    assert sum(r[4] for r in want) == len(coarse_pairs)


# ---- 8. into the engine ----------------------------------------------------------------------------------------------------------
def _pass(configure, load):
    from fithic_amd import tables
    from fithic_amd.engine import Engine
    eng = Engine(0)
    try:
        configure(eng)
        load(eng, tables.ChromIndex())
        eng.run_pass()
        v = eng.fetch()
        return v["p"].copy(), v["q"].copy()
    finally:
        eng.close()


def _from_files(contacts, fragments):
    from fithic_amd import tables

    def load(eng, chroms):
        con = tables.read_contacts(contacts, chroms)
        eng.load_fragments(*tables.read_fragments(fragments, chroms), chroms.sort_rank())
        eng.load_contacts(con.chr1, con.mid1, con.chr2, con.mid2, con.count)
    return load


def test_grid_cells_loaded_directly_give_the_pass_of_the_written_files(tmp_path):
    from fithic_amd import coarsen
    contacts, fragments = os.path.join(DATA, "hESC_chr1_w40000.contacts.gz"), os.path.join(DATA, "hESC_chr1_w40000.frags.gz")
    con, frag = str(tmp_path / "c.gz"), str(tmp_path / "f.gz")
    cells = []

    def direct(eng, chroms):
        with coarsen.read(contacts, fragments, 2, 40000) as data:
            data.write(con)
            data.write_fragments(frag)
            cells.append(len(data))
            data.load_into(eng, chroms)

    def configure(eng):
        eng.configure(80000, 100000, 5000000, 50, 1, "All")
    gp, gq = _pass(configure, direct)
    wp, wq = _pass(configure, _from_files(con, frag))
    assert len(wp) == cells[0] > 100000 and np.isfinite(wp).any() and (wp < 1).any()
    assert bits_equal(gp, wp) and bits_equal(gq, wq)


def test_meta_fragment_cells_loaded_directly_give_the_r_0_pass_of_the_written_files(meta_files):
    from fithic_amd import coarsen, fragpairs
    m = meta_files

    def direct(eng, chroms):
        with fragpairs.read(m["src"], m["bed"]) as fine, coarsen.read(fine, m["triple"], 10, 0, diagonal=False) as data:
            assert len(data) == m["counts"]["cells"]
            data.load_into(eng, chroms)

    def configure(eng):
        eng.configure(0, 0, float("inf"), n_bins=10, mapp_thres=1, mode="All", bias_low=0.5, bias_up=2.0)
    gp, gq = _pass(configure, direct)
    wp, wq = _pass(configure, _from_files(m["contacts"], m["fragments"]))
    assert len(wp) == m["counts"]["cells"] and np.isfinite(wp).any() and (wp < 1).any()
    assert bits_equal(gp, wp) and bits_equal(gq, wq)
