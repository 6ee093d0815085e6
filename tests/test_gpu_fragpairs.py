"""GPU tests of the fragment binning (fithic_amd.fragpairs, csrc/fhx_fragpairs.hip): the fetched columns and the decompressed file
equal the model's (tests/fragpairs_model.py, pinned by hand in test_fragpairs_model.py) byte for byte - on contigs of every size at
which a bisection changes its depth, on empty fragments, on the longest names and the most contigs, on texts built around the
16 KB scan blocks and around batch edges, on one long run and on all-different lines; every refusal names the right line; two runs
give the same bytes; the bed route equals the Digest route; the command line writes the model's file; and a `-r 0` pass fed
directly equals the one run on the written files."""
import glob
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import digest_model as dm
import fragpairs_model as fm
import tile_edge
from batch_env import batch_bytes
from conftest import ROOT, bits_equal
from test_digest_host import _gunzip
from test_fragpairs_model import BAD, TABLE

pytestmark = pytest.mark.gpu

BLOCK = 16384
ENV = "FHX_FP_BATCH_BYTES"


def bed_of(table):
    """the bed file of a model table [(name, E_c)]"""
    return b"".join(b"%s\t%d\t%d\tHIC_%s_%d\t0\t+\n" % (name, start, end, name, k + 1)
                    for name, ends in table for k, (start, end) in enumerate(zip([0] + ends[:-1], ends)))


def line(n1, p1, n2, p2):
    return b"r\t%s\t%d\t+\t%s\t%d\t-\t77\n" % (n1, p1, n2, p2)


def gpu_bytes(data, table, tmp_path, drop=(), batch=None, source=None):
    """the decompressed bytes the device path writes for `data`, after checking the fetched columns and the counts against the
    model; the table goes in as its bed file, or as `source`"""
    from fithic_amd import fragpairs
    src, bed, out = str(tmp_path / "in.validPairs"), str(tmp_path / "table.bed"), str(tmp_path / "out.gz")
    with open(src, "wb") as f:
        f.write(data)
    with open(bed, "wb") as f:
        f.write(bed_of(table))
    want, counts = fm.cells(data, table, [d.encode() for d in drop])
    with batch_bytes(ENV, batch), fragpairs.read(src, bed if source is None else source, drop=drop) as got:
        assert got.names == ["chr%d" % (k + 1) for k in range(len(table))] and len(got) == len(want)
        for k, g in enumerate(got.contacts()):
            assert g.dtype == np.int32 and np.array_equal(g, np.array([c[k] for c in want], np.int32))
        assert got.counts() == counts
        assert set(got.stage_seconds()) == {"read_upload", "newline_scan", "parse", "sort", "cells", "table"}
        got.write(out)
    text = _gunzip(out)
    assert text == fm.text(data, table, [d.encode() for d in drop])
    return text


# ---- 1. where a bisection changes its depth ---------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 63, 64, 65, 4097]
TABLE_OF_SIZES = [(b"s%d" % n, [3 * (k + 1) + (k % 2) for k in range(n)]) for n in SIZES]


def test_contigs_of_1_2_3_63_64_65_and_4097_fragments(tmp_path):
    rng = np.random.default_rng(2)
    rows = []
    for name, ends in TABLE_OF_SIZES:
        if len(ends) <= 65:                                          # every end and every end + 1, and position 1
            ps = sorted(set([1] + ends + [e + 1 for e in ends if e + 1 <= ends[-1]]))
        else:
            picked = rng.choice(len(ends), 300, replace=False).tolist() + [0, 1, len(ends) - 2, len(ends) - 1]
            ps = sorted(set([1] + [ends[k] for k in picked] + [ends[k] + 1 for k in picked if ends[k] + 1 <= ends[-1]]))
        partner = TABLE_OF_SIZES[(SIZES.index(len(ends)) + 3) % len(SIZES)]
        for k, p in enumerate(ps):
            rows.append(line(name, p, partner[0], 1 + (7 * k) % partner[1][-1]))
            rows.append(line(name, ps[-1 - k], name, p))
    data = b"".join(rows)
    text = gpu_bytes(data, TABLE_OF_SIZES, tmp_path)
    assert text.count(b"\n") > 1000


def test_empty_fragments_are_never_hit(tmp_path):
    table = [(b"a", [0, 7, 7, 14, 14]), (b"b", [0, 0, 2, 8, 8])]      # a site at 0, a repeated site, a site at the length; twice at 0
    data = b"".join(line(b"a", p, b"b", q) + line(b"b", q, b"b", 9 - q) + line(b"a", 15 - p, b"a", p) for p in range(1, 15) for q in range(1, 9))
    text = gpu_bytes(data, table, tmp_path)
    assert set(l.split(b"\t")[1] for l in text.splitlines() if l.startswith(b"chr1")) == {b"7", b"14"}
    assert set(l.split(b"\t")[3] for l in text.splitlines() if l.split(b"\t")[2] == b"chr2") == {b"2", b"8"}
    assert gpu_bytes(b"".join(line(b"a", p, b"b", 1 + p % 8) for p in range(1, 15)), TABLE, tmp_path)      # the hand-written table


def test_names_of_1_and_63_bytes_and_4096_contigs(tmp_path):
    names = [b"x", b"y" * 63] + [b"n%d" % k for k in range(2, 4096)]
    table = [(n, [5, 11][:1 + k % 2]) for k, n in enumerate(names)]
    data = b"".join(line(names[k], 1 + k % 5, names[(k * 7 + 1) % 4096], 5) for k in range(4096))
    text = gpu_bytes(data, table, tmp_path, drop=["n5", "q" * 63])
    assert b"chr4096\t" in text and b"chr2\t" in text and b"chr6\t" not in text


# ---- 2. block and batch edges -----------------------------------------------------------------------------------------------
EDGE_TABLE = [(b"chr1", [10000 * (k + 1) for k in range(50)]), (b"chr2", [7000 * (k + 1) for k in range(50)]),
              (b"chromosome_3", [10000 * (k + 1) for k in range(40)] + [2000000000])]


def _filler(n):
    """a kept line of exactly n bytes (the read name takes up the slack)"""
    rest = b"\tchr1\t100\t+\tchr2\t200\t-\n"
    assert n > len(rest)
    return b"F" * (n - len(rest)) + rest


def edge_text(kind, n_edges=4):
    """a text in which, at every 16 KB edge, `kind` straddles the edge: a position token, a name, or a line start that is the
    first / the last byte of a block"""
    rng = np.random.default_rng(5)
    buf = b""
    for k in range(1, n_edges + 1):
        edge = k * BLOCK
        while len(buf) < edge - 400:                                  # ordinary lines, some of them duplicates
            a, b = rng.integers(1, 3, 2)
            p, q = rng.integers(0, 35, 2) * 10000 + rng.integers(1, 10000, 2)
            buf += b"read%d\tchr%d\t%d\t+\tchr%d\t%d\t-\t%d\n" % (len(buf), a, p, b, q, abs(p - q))
        if kind == "token":                                           # the edge falls inside pos1
            text, at = b"e\tchromosome_3\t123456789\t-\tchromosome_3\t55\t+\n", 15 + 4
        elif kind == "name":                                          # ... inside name2
            text, at = b"e\tchr2\t1234\t-\tchromosome_3\t55\t+\n", 14 + 6
        elif kind == "line_start_first":                              # the line starts on the first byte of the next block
            text, at = b"e\tchromosome_3\t1234\t-\tchromosome_3\t99955\t+\n", 0
        else:                                                         # the newline before the line is the first byte of the next block
            text, at = b"e\tchromosome_3\t1234\t-\tchromosome_3\t99955\t+\n", -1
        buf += _filler(edge - at - len(buf)) + text
        assert buf[edge - at:] == text                                # byte `at` of the line is the first byte of the block
    return buf + line(b"chr1", 5, b"chr2", 9) * 3


EDGE_KINDS = ["token", "name", "line_start_first", "newline_first"]


@pytest.mark.parametrize("kind", EDGE_KINDS)
def test_cells_equal_the_model_at_block_edges(kind, tmp_path):
    gpu_bytes(edge_text(kind), EDGE_TABLE, tmp_path)


@pytest.mark.parametrize("kind", EDGE_KINDS)
@pytest.mark.parametrize("batch", [8192, 2 * BLOCK - 100])
def test_cells_equal_the_model_when_batch_edges_fall_inside_the_file(kind, batch, tmp_path):
    data = edge_text(kind)                                            # the filler lines are one cell: its run spans every batch
    assert len(data) > 2 * batch
    gpu_bytes(data, EDGE_TABLE, tmp_path, batch=batch)


def test_no_lines_at_all(tmp_path):
    assert gpu_bytes(b"", TABLE, tmp_path) == b""
    assert gpu_bytes(line(b"a", 1, b"a", 7) + line(b"chrM", 1, b"a", 7), TABLE, tmp_path, drop=["chrM"]) == b""     # every pair dropped


# ---- 3. one long run, and no run at all -------------------------------------------------------------------------------------
def test_one_cell_hit_by_70000_lines(tmp_path):
    data = b"".join(b"r%d\tchr1\t%d\t+\tchr2\t%d\t-\n" % (k, 30001 + k % 9000, 14001 + k % 7000) for k in range(70000))
    assert gpu_bytes(data, EDGE_TABLE, tmp_path) == b"chr1\t40000\tchr2\t21000\t70000\n"


def test_4096_lines_on_4096_different_cells(tmp_path):
    table = [(b"A", [50 * (k + 1) for k in range(64)]), (b"B", [50 * (k + 1) for k in range(64)])]
    order = np.random.default_rng(6).permutation(4096).tolist()
    data = b"".join(line(b"B", 50 * (k % 64) + 1 + k % 50, b"A", 50 * (k // 64) + 50 - k % 50) for k in order)
    assert gpu_bytes(data, table, tmp_path).count(b"\n") == 4096


TILE_TABLE = [(b"a", [10 * (k + 1) for k in range(1002)]), (b"b", [10])]


@pytest.mark.parametrize("n", tile_edge.SIZES)
def test_runs_that_end_and_start_at_a_1024_key_tile_edge(n, tmp_path):
    # cell c is fragment c of `a` x the one fragment of `b`: the sort key is row c << 32 | row 1002
    pairs = [c for c, k in enumerate(tile_edge.hits(n)) for _ in range(k)]
    data = b"".join(line(b"b", 1 + i % 10, b"a", 10 * pairs[i] + 1 + i % 10) for i in tile_edge.file_order(n))
    want, counts = fm.cells(data, TILE_TABLE, [])
    assert counts["pairs"] == n
    tile_edge.assert_runs_meet_the_edge([c[4] for c in want], n)      # from the model's own cells, in the order of its sorted keys
    gpu_bytes(data, TILE_TABLE, tmp_path)


def test_every_line_kept_over_three_batches_and_more(tmp_path):
    # the record array grows from batch to batch with the earlier batches' records in it (DeviceScratch::grow_keep)
    data = b"".join(line(b"chr1", 1 + 523 * k, b"chr2", 349999 - 377 * k) for k in range(900))
    assert len(data) > 3 * 8192 and fm.cells(data, EDGE_TABLE, [])[1]["pairs"] == 900
    gpu_bytes(data, EDGE_TABLE, tmp_path, batch=8192)


def test_gzipped_input(tmp_path):
    data = edge_text("token", 2)
    assert gpu_bytes(gzip.compress(data), EDGE_TABLE, tmp_path) == fm.text(data, EDGE_TABLE)


def test_two_runs_give_the_same_bytes(tmp_path):
    data = edge_text("name") + edge_text("token")
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    assert gpu_bytes(data, EDGE_TABLE, tmp_path / "a") == gpu_bytes(data, EDGE_TABLE, tmp_path / "b", batch=8192)
    with open(str(tmp_path / "a" / "out.gz"), "rb") as f, open(str(tmp_path / "b" / "out.gz"), "rb") as g:
        assert f.read() == g.read()                                   # the compressed bytes too


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
GOOD = line(b"a", 1, b"b", 1)


def _context(table, drop=()):
    from fithic_amd import _capi
    fp = _capi.FpContext(0)
    names = [n for n, _ in table] + list(drop)
    first = np.cumsum([0] + [len(e) for _, e in table])
    fp.load_table(names, list(range(len(table))) + [-1] * len(drop), first, np.array([e for _, ends in table for e in ends], np.int32))
    return fp


def _refusal_of(data, tmp_path, batch=None):
    from fithic_amd import _capi
    src = str(tmp_path / "bad.validPairs")
    with open(src, "wb") as f:
        f.write(data)
    fp = _context(TABLE)
    try:
        with batch_bytes(ENV, batch), pytest.raises(_capi.FpRefused) as e:
            fp.bin_file(src)
        assert fp.n_cells == 0 and fp.device_ptrs() == [0] * 5
        assert fp.counts() == dict(lines=0, pairs=0, dropped_name=0, same_fragment=0, cells=0)
        return e.value.why, e.value.line
    finally:
        fp.close()


@pytest.mark.parametrize("kind", sorted(BAD))
def test_a_bad_line_is_refused_with_its_line_number(kind, tmp_path):
    from fithic_amd import fragpairs
    bad, why = BAD[kind]
    data = GOOD * 1000 + bad + b"\n" + GOOD * 50                      # line 1001 lies in the second 16 KB block
    assert BLOCK < len(GOOD) * 1000 < 2 * BLOCK
    with pytest.raises(fm.Refused) as e:
        fm.pairs(data, TABLE)
    assert (e.value.why, e.value.line) == (why, 1001)
    assert _refusal_of(data, tmp_path) == (why, 1001)
    bed, out = str(tmp_path / "t.bed"), str(tmp_path / "out.gz")
    with open(bed, "wb") as f:
        f.write(bed_of(TABLE))
    with pytest.raises(ValueError, match=r"bad\.validPairs, line 1001: "):
        fragpairs.main([str(tmp_path / "bad.validPairs"), out, "--bed", bed])
    assert not os.path.exists(out)                                    # nothing is written


def test_the_smaller_of_two_bad_lines_is_reported_whatever_batch_it_falls_in(tmp_path):
    data = GOOD * 1000 + b"r a 1 + b\n" + GOOD * 700 + b"r a 0 + b 1\n" + GOOD * 10
    assert _refusal_of(data, tmp_path) == (fm.TOKENS, 1001)          # two blocks of one batch
    assert _refusal_of(data, tmp_path, 8192) == (fm.TOKENS, 1001)    # the other one lies in a later batch
    data = GOOD * 1000 + b"r a 99 + b 1\n" + GOOD * 700 + b"r a 1 + b\n" + GOOD * 10
    assert _refusal_of(data, tmp_path) == (fm.RANGE, 1001)
    assert _refusal_of(data, tmp_path, 8192) == (fm.RANGE, 1001)
    assert _refusal_of(GOOD * 5 + b"r a 1 + b 1\r", tmp_path) == (fm.BYTES, 6)       # a \r that ends the text


def test_a_good_call_after_a_refused_one_gives_the_model_s_cells(tmp_path):
    from fithic_amd import _capi
    rows = [line(b"a", 1 + k % 14, b"b", 1 + k % 8) if k % 3 else line(b"b", 1 + k % 8, b"a", 14 - k % 14) for k in range(1300)]
    good, bad = b"".join(rows), b"".join(rows[:1100]) + b"r a 1 + c 1\n" + b"".join(rows[1100:])
    assert 2 * 8192 < len(b"".join(rows[:1100])) and len(bad) < 4 * 8192     # line 1101 lies in the third batch at the earliest
    for name, data in (("bad.validPairs", bad), ("good.validPairs", good)):
        with open(str(tmp_path / name), "wb") as f:
            f.write(data)
    fp = _context(TABLE)
    try:
        with batch_bytes(ENV, 8192):
            with pytest.raises(_capi.FpRefused) as e:
                fp.bin_file(str(tmp_path / "bad.validPairs"))
            assert (e.value.why, e.value.line) == (fm.NAME, 1101)
            assert fp.counts()["lines"] == 0 and fp.device_ptrs() == [0] * 5
            want, counts = fm.cells(good, TABLE)
            assert fp.bin_file(str(tmp_path / "good.validPairs")) == len(want)
        for k, g in enumerate(fp.fetch_cells()):
            assert np.array_equal(g, np.array([c[k] for c in want], np.int32))
        assert fp.counts() == counts
    finally:
        fp.close()


def test_table_limits_are_refused_before_the_file_is_opened(tmp_path):
    from fithic_amd import fragpairs
    missing = str(tmp_path / "no.such.validPairs")
    for table in ([(b"n%d" % k, [4]) for k in range(4097)], [(b"a", [4]), (b"z" * 64, [4])]):
        bed = str(tmp_path / "limit.bed")
        with open(bed, "wb") as f:
            f.write(bed_of(table))
        with pytest.raises(ValueError, match="at most"):
            fragpairs.read(missing, bed)
    many = fragpairs.Table([b"a"], [0, 1 << 31], np.broadcast_to(np.int32(9), (1 << 31,)))     # no memory behind it
    with pytest.raises(ValueError, match="fewer than 2\\^31"):
        fragpairs.read(missing, many)
    with pytest.raises(ValueError, match="to drop"):
        fragpairs.read(missing, fragpairs.Table([b"a"], [0, 1], [9]), drop=["d" * 64])


# ---- 5. the two table sources, the command line ---------------------------------------------------------------------------------
def _pairs_over(table, n, seed, extra=()):
    """n lines over a model table: a position anywhere, its partner near it, far from it or on another contig"""
    rng = np.random.default_rng(seed)
    names = [name for name, ends in table if ends[-1] > 0]
    length = {name: ends[-1] for name, ends in table}
    rows = []
    for k in range(n):
        n1 = names[rng.integers(len(names))]
        n2 = n1 if rng.random() < 0.8 else names[rng.integers(len(names))]
        p1 = int(rng.integers(1, length[n1] + 1))
        p2 = int(rng.integers(1, length[n2] + 1)) if n2 != n1 or rng.random() < 0.3 else min(length[n1], p1 + int(rng.pareto(1.2) * 300))
        rows.append(b"r%d\t%s\t%d\t+\t%s\t%d\t-\t%d\tHIC_%s_1\tHIC_%s_2\t42\t42\n" % (k, n1, p1, n2, p2, abs(p1 - p2), n1, n2))
    return b"".join(rows + list(extra))


def _wrap(seq, width=60):
    return b"".join(seq[k:k + width] + b"\n" for k in range(0, len(seq), width))


def _genome(seed=12):
    """three contigs of random bases whose names are not chr1, chr2, chr3"""
    rng = np.random.default_rng(seed)
    return b"".join(b">%s\n" % n + _wrap(bytes(b"ACGT"[k] for k in rng.integers(0, 4, size))) for n, size in ((b"II", 90000), (b"I", 60000), (b"X", 75000)))


TWO_ENZYMES = ["^GATC", "bglii"]                                      # every AGATCT is cut twice at one place: empty fragments


def test_bed_and_digest_of_the_same_fasta_give_the_same_file(tmp_path):
    from fithic_amd import digest
    fasta = str(tmp_path / "g.fa")
    with open(fasta, "wb") as f:
        f.write(_genome())
    table = fm.table_of_fasta(_genome(), TWO_ENZYMES)
    assert any(a == b for _, e in table for a, b in zip(e, e[1:]))
    data = _pairs_over(table, 3000, 3)
    d = digest.read(fasta, TWO_ENZYMES)
    d.write_bed(str(tmp_path / "d.bed"))
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    one = gpu_bytes(data, table, tmp_path / "a", source=d)
    two = gpu_bytes(data, table, tmp_path / "b", source=str(tmp_path / "d.bed"))
    assert one == two and one.count(b"\n") > 1000
    with open(str(tmp_path / "a" / "out.gz"), "rb") as f, open(str(tmp_path / "b" / "out.gz"), "rb") as g:
        assert f.read() == g.read()


@pytest.mark.parametrize("source", ["fasta", "bed"])
def test_command_line_writes_the_model_s_file_and_prints_the_model_s_counts(source, tmp_path):
    fasta, bed, src, out = str(tmp_path / "g.fa"), str(tmp_path / "g.bed"), str(tmp_path / "lib.allValidPairs.gz"), str(tmp_path / "contacts.gz")
    with open(fasta, "wb") as f:
        f.write(_genome())
    with open(bed, "wb") as f:
        f.write(dm.bed(_genome(), TWO_ENZYMES))
    table = fm.table_of_fasta(_genome(), TWO_ENZYMES)
    data = _pairs_over(table, 2000, 4, extra=[b"m\tchrM\t5\t+\t%s\t1\t-\n" % table[0][0]] * 7)
    with open(src, "wb") as f:
        f.write(gzip.compress(data))
    where = ["--fasta", fasta, "--re", TWO_ENZYMES[0], "--also", TWO_ENZYMES[1]] if source == "fasta" else ["--bed", bed]
    r = subprocess.run([sys.executable, "-m", "fithic_amd.fragpairs", src, out] + where + ["--drop", "chrM"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    want, counts = fm.cells(data, table, [b"chrM"])
    assert counts["dropped_name"] == 7 and counts["same_fragment"] > 0 and counts["cells"] > 1000
    assert r.stdout == "".join("%s\t%d\n" % (k, counts[k]) for k in ("lines", "pairs", "dropped_name", "same_fragment", "cells"))
    assert _gunzip(out) == fm.text(data, table, [b"chrM"])


# ---- 6. end to end: digest -> fragpairs -> a -r 0 pass ----------------------------------------------------------------------------
def _one_pass(load, out=None):
    from fithic_amd import tables
    from fithic_amd.engine import Engine
    eng = Engine(0)
    try:
        eng.configure(0, 0, float("inf"), n_bins=10, mapp_thres=1, mode="All", bias_low=0.5, bias_up=2.0)
        chroms = tables.ChromIndex()
        load(eng, chroms)
        eng.run_pass()
        v = eng.fetch()
        if out:
            eng.ctx.write_significances_device(out, chroms.names)
        return v["p"].copy(), v["q"].copy()
    finally:
        eng.close()


def test_direct_route_equals_the_run_on_the_written_files(tmp_path):
    from fithic_amd import digest, fragpairs, tables
    genome = _genome()
    table = fm.table_of_fasta(genome, ["^GATC"])
    assert all(e[0] > 0 and all(a < b for a, b in zip(e, e[1:])) for _, e in table)      # no empty fragment: one locus per row
    fasta, src = str(tmp_path / "g.fa"), str(tmp_path / "s.allValidPairs")
    with open(fasta, "wb") as f:
        f.write(genome)
    pairs = _pairs_over(table, 40000, 13)
    with open(src, "wb") as f:
        f.write(pairs)
    frag_path, con_path, bed = str(tmp_path / "frags"), str(tmp_path / "contacts.gz"), str(tmp_path / "g.bed")
    # the file route: three command lines
    digest.main([frag_path, "^GATC", fasta, "--bed", bed])
    fragpairs.main([src, con_path, "--bed", bed])
    r = subprocess.run([sys.executable, "-m", "fithic_amd", "-i", con_path, "-f", frag_path + ".gz", "-o", str(tmp_path / "out"), "-r", "0",
                        "-b", "10", "-x", "All"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    written = glob.glob(str(tmp_path / "out" / "*spline_pass1*significances.txt.gz"))
    assert len(written) == 1
    contacts = _gunzip(con_path)
    n_cells = contacts.count(b"\n")
    assert n_cells > 5000 and contacts == fm.text(pairs, table)
    loci = set(tuple(l.split(b"\t")[::2][:2]) for l in _gunzip(frag_path + ".gz").splitlines())
    for l in contacts.splitlines():
        t = l.split(b"\t")
        assert (t[0], t[1]) in loci and (t[2], t[3]) in loci          # every locus of the contacts is a line of the fragments file

    def from_files(eng, chroms):
        con = tables.read_contacts(con_path, chroms)
        eng.load_fragments(*tables.read_fragments(frag_path + ".gz", chroms), chroms.sort_rank())
        eng.load_contacts(con.chr1, con.mid1, con.chr2, con.mid2, con.count)

    def direct(eng, chroms):
        d = digest.read(fasta, ["^GATC"])
        eng.load_fragments(*d.fragments(chroms), chroms.sort_rank())
        with fragpairs.read(src, d) as data:
            assert len(data) == n_cells
            data.load_into(eng, chroms)

    direct_out = str(tmp_path / "direct.significances.txt.gz")
    (wp, wq), (gp, gq) = _one_pass(from_files), _one_pass(direct, direct_out)
    assert len(wp) == n_cells and np.isfinite(wp).any() and (wp < 1).any()
    assert bits_equal(gp, wp) and bits_equal(gq, wq)
    with open(direct_out, "rb") as f, open(written[0], "rb") as g:
        assert f.read() == g.read()                                   # the writer's file, compressed bytes included
