"""GPU tests of the validPairs path (fithic_amd.validpairs, csrc/fhx_validpairs.hip): the written file equals the real script's
after decompression (tests/golden/validpairs), the cells equal the model's (tests/validpairs_model.py) on texts built around
the 16 KB scan blocks and around batch edges, on one long run and on all-different lines, every refusal names the right line,
two runs give the same bytes, and the direct path feeds an Engine the same rows as the written files do."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import tile_edge
import validpairs_model as vm
from batch_env import batch_bytes
from conftest import ROOT, bits_equal
from test_validpairs_host import RUNS, VP, _gunzip, run_input

pytestmark = pytest.mark.gpu

BLOCK = 16384
GOOD = b"r\tchr1\t5\t+\tchr2\t9\t-\n"


def gpu_bytes(data, res, tmp_path, batch=None):
    """the decompressed bytes the device path writes for `data`, after checking the fetched columns against the model"""
    from fithic_amd import validpairs
    src, out = str(tmp_path / "in.validPairs"), str(tmp_path / "out.gz")
    with open(src, "wb") as f:
        f.write(data)
    with batch_bytes("FHX_VP_BATCH_BYTES", batch), validpairs.read(src, res) as got:
        names, *cols = vm.columns(data, res)
        assert got.names == names and len(got) == len(cols[0])
        for g, w in zip(got.contacts(), cols):
            assert g.dtype == np.int32 and np.array_equal(g, np.asarray(w, np.int32))
        counts = got.counts()
        assert counts["lines"] == len(vm.lines_of(gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data))
        assert counts["pairs"] == sum(cols[4]) and counts["cells"] == len(cols[0])
        got.write(out)
    return _gunzip(out)


# ---- 1. goldens -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RUNS))
def test_device_path_writes_the_script_s_file(name, tmp_path):
    run = RUNS[name]
    assert gpu_bytes(run_input(run), run["res"], tmp_path) == _gunzip(os.path.join(VP, run["output"]))


@pytest.mark.parametrize("name", ["vpa_r10000", "vpb_r50", "vpa_r10000_gz"])
def test_command_line_writes_the_script_s_file(name, tmp_path):
    run = RUNS[name]
    src = str(tmp_path / "lib.allValidPairs")
    with open(src, "wb") as f:
        f.write(run_input(run))
    r = subprocess.run([sys.executable, "-m", "fithic_amd.validpairs", str(run["res"]), "lib", src, str(tmp_path)], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == run["stdout"]
    assert _gunzip(str(tmp_path / "lib_fithic.contactCounts.gz")) == _gunzip(os.path.join(VP, run["output"]))


# ---- 2. block and batch edges -----------------------------------------------------------------------------------------------
def _filler(n):
    """a kept line of exactly n bytes (the read name takes up the slack)"""
    rest = b"\tchr1\t100\t+\tchr2\t200\t-\n"
    assert n > len(rest)
    return b"F" * (n - len(rest)) + rest


def edge_text(kind, n_edges=4):
    """a text in which, at every 16 KB edge, `kind` straddles the edge: a position token, a chrM occurrence, or a line start that
    is the first / the last byte of a block"""
    rng = np.random.default_rng(5)
    buf = b""
    for k in range(1, n_edges + 1):
        edge = k * BLOCK
        while len(buf) < edge - 400:                                  # ordinary lines, some of them duplicates
            a, b = rng.integers(1, 4, 2)
            p, q = rng.integers(0, 40, 2) * 10000 + rng.integers(0, 10000, 2)
            buf += b"read%d\tchr%d\t%d\t+\tchr%d\t%d\t-\t%d\n" % (len(buf), a, p, b, q, abs(p - q))
        if kind == "token":                                           # the edge falls inside pos1
            line, at = b"e\tchr3\t123456789\t-\tchr3\t55\t+\n", 7 + 4
        elif kind == "chrM_name":                                     # ... inside the chrM of a chromosome column
            line, at = b"e\tchrM\t1234\t-\tchr3\t55\t+\n", 2 + 2
        elif kind == "chrM_tail":                                     # ... inside a chrM of a trailing column
            line, at = b"e\tchr3\t1234\t-\tchr3\t99955\t+\txchrMx\n", 28 + 2
        elif kind == "line_start_first":                              # the line starts on the first byte of the next block
            line, at = b"e\tchr3\t1234\t-\tchr3\t99955\t+\n", 0
        else:                                                         # the newline before the line is the first byte of the next block
            line, at = b"e\tchr3\t1234\t-\tchr3\t99955\t+\n", -1
        buf += _filler(edge - at - len(buf)) + line
        assert buf[edge - at:] == line                                # byte `at` of the line is the first byte of the block
    return buf + GOOD * 3


EDGE_KINDS = ["token", "chrM_name", "chrM_tail", "line_start_first", "newline_first"]


@pytest.mark.parametrize("kind", EDGE_KINDS)
def test_cells_equal_the_model_at_block_edges(kind, tmp_path):
    data = edge_text(kind)
    assert gpu_bytes(data, 10000, tmp_path) == vm.text(data, 10000)


@pytest.mark.parametrize("kind", EDGE_KINDS)
@pytest.mark.parametrize("batch", [8192, 2 * BLOCK - 100])
def test_cells_equal_the_model_when_batch_edges_fall_inside_the_file(kind, batch, tmp_path):
    data = edge_text(kind)                                            # the filler lines are one cell: its run spans every batch
    assert len(data) > 2 * batch
    assert gpu_bytes(data, 10000, tmp_path, batch) == vm.text(data, 10000)


def test_no_lines_at_all(tmp_path):
    assert gpu_bytes(b"", 10000, tmp_path) == b""
    assert gpu_bytes(b"r chr1 5 + chr1 9\n", 10000, tmp_path) == b""     # every pair dropped


# ---- 3. one long run, and no run at all -------------------------------------------------------------------------------------
def test_one_cell_hit_by_70000_lines(tmp_path):
    data = b"".join(b"r%d\tchr7\t%d\t+\tchr7\t%d\t-\n" % (k, 30000 + k % 9000, 990000 + k % 7000) for k in range(70000))
    assert gpu_bytes(data, 10000, tmp_path) == b"chr7\t35000\tchr7\t995000\t  70000\n"


def test_4096_lines_that_are_all_different(tmp_path):
    data = b"".join(b"r\tchr%d\t%d\t+\t%d\t%d\t-\n" % (k % 3, (k // 64) * 50, k % 5, (k % 64) * 50 + 10000) for k in range(4096))
    want = vm.text(data, 50)
    assert want.count(b"\n") == 4096
    assert gpu_bytes(data, 50, tmp_path) == want


@pytest.mark.parametrize("n", tile_edge.SIZES)
def test_runs_that_end_and_start_at_a_1024_key_tile_edge(n, tmp_path):
    # cell c is chr1:3 x chr2:10000 + 2 * c: five digits at resolution 2, so the script's text order is the order of c
    pairs = [c for c, k in enumerate(tile_edge.hits(n)) for _ in range(k)]
    data = b"".join(b"r\tchr1\t3\t+\tchr2\t%d\t-\n" % (10000 + 2 * pairs[i] + i % 2) for i in tile_edge.file_order(n))
    tile_edge.assert_runs_meet_the_edge(vm.columns(data, 2)[5], n)   # from the model's own cells, in the order of its sorted keys
    assert gpu_bytes(data, 2, tmp_path) == vm.text(data, 2)


def test_every_line_kept_over_three_batches_and_more(tmp_path):
    # the record array grows from batch to batch with the earlier batches' records in it (DeviceScratch::grow_keep)
    data = b"".join(b"read%06d\tchr%d\t%d\t+\tchr%d\t%d\t-\n" % (k, 1 + k % 3, 100 + 37 * k, 4 + k % 2, 900000 - 91 * k) for k in range(900))
    assert len(data) > 3 * 8192 and sum(vm.columns(data, 10000)[5]) == 900
    assert gpu_bytes(data, 10000, tmp_path, 8192) == vm.text(data, 10000)


def test_two_runs_give_the_same_bytes(tmp_path):
    data = edge_text("token") + run_input(RUNS["vpa_r10000"])
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    assert gpu_bytes(data, 10000, tmp_path / "a") == gpu_bytes(data, 10000, tmp_path / "b", 8192)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
BAD_LINES = {"five tokens": (b"r chr1 5 + chr2", vm.TOKENS), "empty line": (b"", vm.TOKENS), "blank line": (b" \t ", vm.TOKENS),
             "name with a sign": (b"r +x 5 + chr2 9", vm.NAME), "name with a point": (b"r chr1 5 + .5 9", vm.NAME),
             "digit then letter": (b"r 1x 5 + chr2 9", vm.NAME), "leading zero": (b"r 02 5 + chr2 9", vm.NAME),
             "inf": (b"r Inf 5 + chr2 9", vm.NAME), "nan": (b"r chr1 5 + nAn1 9", vm.NAME), "signed position": (b"r chr1 -5 + chr2 9", vm.POSITION),
             "point in a position": (b"r chr1 5.0 + chr2 9", vm.POSITION), "exponent": (b"r chr1 5 + chr2 1e3", vm.POSITION),
             "11 digits": (b"r chr1 12345678901 + chr2 9", vm.POSITION), "midpoint beyond int32": (b"r chr1 5 + chr2 2147480000", vm.RANGE),
             "NUL": (b"r chr1 5 + chr2 9 \x00", vm.BYTES), "non-ASCII": (b"r chr1 5 + ch\xe9 9", vm.BYTES),
             "lone CR": (b"r chr1 5\r + chr2 9", vm.BYTES), "long line": (b"r" * 4097 + b" chr1 5 + chr2 9", vm.LONG_LINE)}


def _refusal_of(data, res, tmp_path, batch=None):
    from fithic_amd import _capi
    src = str(tmp_path / "bad.validPairs")
    with open(src, "wb") as f:
        f.write(data)
    vp = _capi.VpContext(0)
    try:
        with batch_bytes("FHX_VP_BATCH_BYTES", batch), pytest.raises(_capi.VpRefused) as e:
            vp.bin_file(src, res)
        assert vp.n_cells == 0 and vp.device_ptrs() == [0] * 5
        return e.value.why, e.value.line
    finally:
        vp.close()


@pytest.mark.parametrize("kind", sorted(BAD_LINES))
def test_a_bad_line_is_refused_with_its_line_number(kind, tmp_path):
    bad, why = BAD_LINES[kind]
    data = GOOD * 900 + bad + b"\n" + GOOD * 50                       # line 901 lies in the second 16 KB block
    with pytest.raises(vm.Refused) as e:
        vm.pairs(data, 10000)
    assert (e.value.why, e.value.line) == (why, 901)
    assert _refusal_of(data, 10000, tmp_path) == (why, 901)


def test_the_smaller_of_two_bad_lines_is_reported_in_a_later_batch_too(tmp_path):
    data = GOOD * 1000 + b"r chr1 5 + chr2\n" + GOOD * 700 + b"r 02 5 + chr2 9\n" + GOOD * 10
    assert _refusal_of(data, 10000, tmp_path) == (vm.TOKENS, 1001)
    assert _refusal_of(data, 10000, tmp_path, 8192) == (vm.TOKENS, 1001)
    assert _refusal_of(GOOD * 5 + b"r chr1 5 + chr2 9\r", 10000, tmp_path) == (vm.BYTES, 6)       # a \r that ends the text


def test_a_good_call_after_a_refused_one_gives_the_model_s_cells(tmp_path):
    from fithic_amd import _capi
    rows = [b"r\tchr%d\t%d\t+\tchr%d\t%d\t-\n" % (1 + k % 3, 1000 * k, 1 + k % 2, 700 * k + 5) for k in range(900)]
    good, bad = b"".join(rows), b"".join(rows[:700]) + b"r chr1 5 + chr2\n" + b"".join(rows[700:])
    assert 2 * 8192 < len(b"".join(rows[:700])) and len(bad) < 4 * 8192      # line 701 lies in the third batch at the earliest
    for name, data in (("bad.validPairs", bad), ("good.validPairs", good)):
        with open(str(tmp_path / name), "wb") as f:
            f.write(data)
    vp = _capi.VpContext(0)
    try:
        with batch_bytes("FHX_VP_BATCH_BYTES", 8192):
            with pytest.raises(_capi.VpRefused) as e:
                vp.bin_file(str(tmp_path / "bad.validPairs"), 10000)
            assert (e.value.why, e.value.line) == (vm.TOKENS, 701)
            assert vp.counts() == dict(lines=0, pairs=0, cells=0, names=0) and vp.device_ptrs() == [0] * 5
            names, *cols = vm.columns(good, 10000)
            assert vp.bin_file(str(tmp_path / "good.validPairs"), 10000) == len(cols[0])
        assert vp.names() == names
        for g, w in zip(vp.fetch_cells(), cols):
            assert np.array_equal(g, np.asarray(w, np.int32))
        assert vp.counts() == dict(lines=900, pairs=sum(cols[4]), cells=len(cols[0]), names=len(names))
    finally:
        vp.close()


def test_lines_the_first_filters_drop_are_not_read_further(tmp_path):
    data = GOOD + b"r chr100 x + 1x -9\nr 02 1e3 + chr1 9 chrM\n" + GOOD
    assert gpu_bytes(data, 10000, tmp_path) == b"chr1\t5000\tchr2\t5000\t      2\n"


def test_resolution_and_name_table_refusals(tmp_path):
    from fithic_amd import validpairs
    for res in (0, 1, 9999):
        assert _refusal_of(GOOD, res, tmp_path) == (vm.RES, 0)
    many = b"".join(b"r\tn%04d\t5\t+\tn%04d\t900000\t-\n" % (k, k) for k in range(vm.MAX_NAMES + 1))
    with pytest.raises(vm.Refused) as e:
        vm.pairs(many, 10000)
    assert e.value.why == vm.NAMES
    assert _refusal_of(many, 10000, tmp_path) == (vm.NAMES, 0)
    fits = many[:many.rindex(b"r\t")]                                 # 1024 names are taken
    assert gpu_bytes(fits, 10000, tmp_path).count(b"\n") == vm.MAX_NAMES
    src = str(tmp_path / "bad.validPairs")
    with open(src, "wb") as f:
        f.write(GOOD * 2 + b"r 1x 5 + chr2 9\n")
    with pytest.raises(ValueError, match="line 3.*The reference accepts this"):
        validpairs.read(src, 10000)


# ---- 5. the direct path -----------------------------------------------------------------------------------------------------
def _two_passes(load):
    from fithic_amd import tables
    from fithic_amd.engine import Engine
    eng = Engine(0)
    try:
        eng.configure(10000, 20000, 2000000, 20, 1, "intraOnly")
        load(eng, tables.ChromIndex())
        out = []
        for _ in range(2):
            eng.run_pass()
            v = eng.fetch()
            out.append((v["p"].copy(), v["q"].copy()))
            eng.next_pass()
        return out
    finally:
        eng.close()


def test_direct_path_equals_the_run_on_the_written_files(tmp_path):
    from fithic_amd import fragments, tables, validpairs
    rng = np.random.default_rng(11)
    n = 40000
    chrom = rng.integers(1, 4, n)
    left = rng.integers(0, 2900000, n)
    gap = (rng.pareto(1.2, n) * 30000).astype(np.int64) % 2500000 + 150
    right = np.minimum(left + gap, 2999999)
    src, sizes = str(tmp_path / "s.allValidPairs"), str(tmp_path / "chrom.sizes")
    with open(src, "wb") as f:
        f.write(b"".join(b"r%d\tchr%d\t%d\t+\tchr%d\t%d\t-\n" % (k, chrom[k], left[k], chrom[k], right[k]) for k in range(n)))
    with open(sizes, "w") as f:
        f.write("chr1\t3000000\nchr2\t3000000\nchr3\t2999999\n")
    con_path, frag_path = str(tmp_path / "lib_fithic.contactCounts.gz"), str(tmp_path / "frags.gz")
    validpairs.main(["10000", "lib", src, str(tmp_path)])
    fragments.main(["--chrLens", sizes, "--outFile", frag_path, "--resolution", "10000"])
    n_cells = _gunzip(con_path).count(b"\n")
    assert n_cells > 5000

    def from_files(eng, chroms):
        con = tables.read_contacts(con_path, chroms)
        fc, fm, fh = tables.read_fragments(frag_path, chroms)
        eng.load_fragments(fc, fm, fh, chroms.sort_rank())
        eng.load_contacts(con.chr1, con.mid1, con.chr2, con.mid2, con.count)

    def direct(eng, chroms):
        with validpairs.read(src, 10000) as data:
            assert len(data) == n_cells
            data.intern(chroms)
            eng.load_fragments(*fragments.bins(sizes, 10000, chroms), chroms.sort_rank())
            data.load_into(eng, chroms)

    want, got = _two_passes(from_files), _two_passes(direct)
    for (wp, wq), (gp, gq) in zip(want, got):
        assert len(wp) == n_cells and np.isfinite(wp).any()
        assert bits_equal(gp, wp) and bits_equal(gq, wq)
