"""GPU tests of the HiC-Pro converter (fithic_amd.hicpro, csrc/fhx_hicpro.hip): the three output files equal the real
reference's after decompression (tests/golden/hicpro), the kernels' columns and totals equal the model's on matrices built
around the 16 KB scan blocks and under same-address pressure, every refusal names the right line, and the direct path feeds an
Engine the same rows as the written files do."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import hicpro_model as hm
from conftest import ROOT, bits_equal

pytestmark = pytest.mark.gpu

CASE_NAMES = ["hp1", "hp2_r0", "hp2_r10000", "hp3"]
BLOCK = 16384
OUT_NAMES = ("fithic.interactionCounts.gz", "fithic.fragmentMappability.gz", "fithic.biases.gz")


def _gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


# ---- 1. goldens ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_function_writes_the_reference_s_files(name, tmp_path, capsys):
    from fithic_amd import hicpro
    case = hm.CASES[name]
    bed, matrix, bias = hm.case_inputs(case, tmp_path)
    outs = [str(tmp_path / n) for n in OUT_NAMES]
    hicpro.outputfithicform(bed, matrix, outs[0], outs[1], bias, outs[2] if bias else None, case["res"])
    assert capsys.readouterr().out == case["stdout"]
    want = hm.case_outputs(case)
    assert _gunzip(outs[0]) == want[0]
    assert _gunzip(outs[1]) == want[1]
    if bias:
        assert _gunzip(outs[2]) == want[2]
    else:
        assert not os.path.exists(outs[2])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_command_line_writes_the_reference_s_files(name, tmp_path):
    case = hm.CASES[name]
    bed, matrix, bias = hm.case_inputs(case, tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    cmd = [sys.executable, "-m", "fithic_amd.hicpro", "-i", matrix, "-b", bed, "-o", str(out), "-r", str(case["res"])]
    if bias:
        cmd += ["-s", bias]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == case["stdout"]
    want = hm.case_outputs(case)
    assert _gunzip(str(out / OUT_NAMES[0])) == want[0]
    assert _gunzip(str(out / OUT_NAMES[1])) == want[1]
    if bias:
        assert _gunzip(str(out / OUT_NAMES[2])) == want[2]
    else:
        assert not (out / OUT_NAMES[2]).exists()


# ---- generated matrices -------------------------------------------------------------------------------------------------
N_BINS = 300
HOLE = 150                                                           # an index the bed of the refusal tests does not list


@pytest.fixture(scope="module")
def bed_bytes():
    return hm.fixture_bytes("hp2.bed.gz")


def _line(rng, bins):
    i, j = (int(v) for v in rng.choice(bins, 2))
    c = int(rng.integers(1, 100000))
    count = ("%d", "%d.0", "%d.000000")[int(rng.integers(0, 3))] % c
    sep = ("\t", " ", " \t ")[int(rng.integers(0, 3))]
    return ("%d%s%d%s%s\n" % (i, sep, j, sep, count)).encode()


def fill(rng, nbytes, bins=None):
    """exactly nbytes of whole lines (each ends in \\n); the last one is padded with blanks to fit"""
    bins = np.arange(1, N_BINS + 1) if bins is None else bins
    out, left = [], nbytes
    while left > 64:
        ln = _line(rng, bins)
        out.append(ln)
        left -= len(ln)
    ln = _line(rng, bins)
    while len(ln) > left:
        ln = b"7 9 1\n"
    assert left >= 6
    out.append(b" " * (left - len(ln)) + ln)
    data = b"".join(out)
    assert len(data) == nbytes and data.endswith(b"\n")
    return data


def _edge_texts():
    rng = np.random.default_rng(7)
    texts = {"one_line": b"3\t4\t5\n", "16383": fill(rng, BLOCK - 1), "16384": fill(rng, BLOCK), "16385": fill(rng, BLOCK + 1)}
    texts["line_begins_at_last_byte_of_block"] = fill(rng, BLOCK - 1) + fill(rng, 5000)
    texts["newline_is_first_byte_of_block"] = fill(rng, BLOCK + 1) + fill(rng, 3000)
    texts["3_blocks_and_1_byte_no_final_newline"] = fill(rng, 3 * BLOCK + 2)[:-1]
    assert texts["line_begins_at_last_byte_of_block"][BLOCK - 2:BLOCK - 1] == b"\n"
    assert texts["newline_is_first_byte_of_block"][BLOCK:BLOCK + 1] == b"\n"
    t = texts["3_blocks_and_1_byte_no_final_newline"]
    assert len(t) == 3 * BLOCK + 1 and not t.endswith(b"\n")
    return texts


EDGE_TEXTS = _edge_texts()


def _device(bed, matrix_bytes, tmp_path, name="m.matrix"):
    """-> (columns, totals) of the native unit for these bed bytes and matrix bytes"""
    from fithic_amd import _capi, hicpro
    bed_path, matrix_path = str(tmp_path / "b.bed"), str(tmp_path / name)
    with open(bed_path, "wb") as f:
        f.write(bed)
    with open(matrix_path, "wb") as f:
        f.write(matrix_bytes)
    b = hicpro.read_bed(bed_path)
    hp = _capi.HpContext(0)
    try:
        hp.load_bins(b.index_base, b.chr_id, b.mid)
        n = hp.parse_matrix(matrix_path)
        cols, totals = hp.fetch_rows(), hp.totals()
        assert all(len(c) == n for c in cols)
        return cols, totals
    finally:
        hp.close()


def _assert_equals_model(bed, text, tmp_path):
    m = hm.Model(bed, text)
    cols, totals = _device(bed, text, tmp_path)
    for got, want in zip(cols, m.cols):
        assert got.dtype == np.int32 and np.array_equal(got, want)
    assert totals.dtype == np.int64 and np.array_equal(totals, m.totals)
    return totals


# ---- 2. columns and totals at block edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(EDGE_TEXTS))
def test_columns_and_totals_equal_the_model_at_block_edges(shape, bed_bytes, tmp_path):
    _assert_equals_model(bed_bytes, EDGE_TEXTS[shape], tmp_path)


def test_no_lines_at_all(bed_bytes, tmp_path):
    cols, totals = _device(bed_bytes, b"", tmp_path)
    assert all(len(c) == 0 for c in cols) and len(totals) == N_BINS and not totals.any()


# ---- 3. same-address pressure --------------------------------------------------------------------------------------------
def _pressure_text(kind):
    rng = np.random.default_rng(11)
    c = rng.integers(1, 2**31, 20000) if kind != "random" else rng.integers(1, 5000, 20000)
    if kind == "diagonal":
        i, j = np.ones(20000, np.int64), np.ones(20000, np.int64)
    elif kind == "cycle64":
        i, j = np.ones(20000, np.int64), 1 + np.arange(20000) % 64
    else:
        i, j = rng.integers(1, N_BINS + 1, 20000), rng.integers(1, N_BINS + 1, 20000)
    return "".join("%d\t%d\t%d\n" % (a, b, n) for a, b, n in zip(i, j, c)).encode()


@pytest.mark.parametrize("kind", ["diagonal", "cycle64", "random"])
def test_totals_are_exact_and_repeatable_under_same_address_pressure(kind, bed_bytes, tmp_path):
    text = _pressure_text(kind)
    first = _assert_equals_model(bed_bytes, text, tmp_path)
    second = _assert_equals_model(bed_bytes, text, tmp_path)
    assert np.array_equal(first, second)
    if kind == "diagonal":
        assert first[0] > 2**44 and not first[1:].any()               # 2 x 20 000 counts of up to 2^31: far beyond 32 bits


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def holed_bed(bed_bytes):
    lines = [ln for ln in bed_bytes.split(b"\n") if ln and int(ln.split()[3]) != HOLE]
    return b"\n".join(lines) + b"\n"


def _good_lines():
    bins = np.array([k for k in range(1, N_BINS + 1) if k != HOLE])
    return fill(np.random.default_rng(3), 2 * BLOCK, bins).split(b"\n")[:-1]


GOOD_LINES = _good_lines()
# bad line -> (exception, reason code name, the KeyError's index)
BAD_LINES = {
    "2.5": (b"4 5 2.5", ValueError, "HP_FRACTION", None),
    "1e2": (b"4 5 1e2", ValueError, "HP_COUNT", None),
    "-3": (b"4 5 -3", ValueError, "HP_COUNT", None),
    "1_0": (b"4 5 1_0", ValueError, "HP_COUNT", None),
    "four_tokens": (b"4 5 6 7", ValueError, "HP_TOKENS", None),
    "two_tokens": (b"4 5", ValueError, "HP_TOKENS", None),
    "empty_line": (b"", ValueError, "HP_TOKENS", None),
    "absent_index": (b"4 %d 6" % HOLE, KeyError, "HP_ABSENT", HOLE),
    "index_outside_the_table": (b"5000 4 6", KeyError, "HP_ABSENT", 5000),
    "11_digit_index": (b"12345678901 5 6", ValueError, "HP_INDEX", None),
    "nul_byte": (b"4 5\x00 6", ValueError, "HP_BYTES", None),
}


def _refused(holed_bed, lines, tmp_path):
    """-> (HpRefused of the native call, exception of outputfithicform); no output file may exist afterwards"""
    from fithic_amd import _capi, hicpro
    bed_path, matrix_path = str(tmp_path / "b.bed"), str(tmp_path / "bad.matrix")
    with open(bed_path, "wb") as f:
        f.write(holed_bed)
    with open(matrix_path, "wb") as f:
        f.write(b"\n".join(lines) + b"\n")
    b = hicpro.read_bed(bed_path)
    hp = _capi.HpContext(0)
    try:
        hp.load_bins(b.index_base, b.chr_id, b.mid)
        with pytest.raises(_capi.HpRefused) as low:
            hp.parse_matrix(matrix_path)
        assert hp.n_rows == 0 and not hp.totals().any() and hp.device_ptrs() == [0] * 5        # nothing stays loaded
    finally:
        hp.close()
    outs = [str(tmp_path / n) for n in OUT_NAMES]
    with pytest.raises((ValueError, KeyError)) as high:
        hicpro.outputfithicform(bed_path, matrix_path, outs[0], outs[1])
    assert not any(os.path.exists(p) for p in outs)
    return low.value, high.value


@pytest.mark.parametrize("kind", sorted(BAD_LINES))
@pytest.mark.parametrize("where", ["first_block", "second_block"])
def test_a_bad_line_is_refused_with_its_line_number(kind, where, holed_bed, tmp_path):
    from fithic_amd import _capi
    text, exc, why, index = BAD_LINES[kind]
    at = 17 if where == "first_block" else len(GOOD_LINES) - 9
    lines = list(GOOD_LINES)
    lines[at] = text
    assert (sum(len(ln) + 1 for ln in lines[:at]) >= BLOCK) == (where == "second_block")
    low, high = _refused(holed_bed, lines, tmp_path)
    assert (low.why, low.line) == (getattr(_capi, why), at + 1)
    assert type(high) is exc
    if exc is KeyError:
        assert low.index == index and high.args == (index,)
    else:
        assert "line %d" % (at + 1) in str(high)
        accepted_by_the_reference = kind in ("2.5", "1e2", "-3", "1_0", "11_digit_index", "four_tokens")
        assert ("raw (integer) HiC-Pro matrix" in str(high)) == accepted_by_the_reference


def test_the_smaller_of_two_bad_lines_is_reported(holed_bed, tmp_path):
    from fithic_amd import _capi
    lines = list(GOOD_LINES)
    late, early = len(GOOD_LINES) - 5, len(GOOD_LINES) // 2 + 3
    lines[late] = b"4 5"                                             # reason code 1 at the larger line number ...
    lines[early] = b"4 %d 6" % HOLE                                  # ... must not win over reason code 5 at the smaller one
    low, high = _refused(holed_bed, lines, tmp_path)
    assert (low.why, low.line, low.index) == (_capi.HP_ABSENT, early + 1, HOLE)
    assert type(high) is KeyError and high.args == (HOLE,)


def test_a_total_of_2_to_the_53_is_refused(bed_bytes, tmp_path):
    """2^21 diagonal lines of 2^31 - 1 give bin 1 the total 2^53 - 2^22; eight lines more pass 2^53.  (32 MB of text: the upload
    takes both pinned buffers.)"""
    from fithic_amd import _capi
    line = b"1\t1\t2147483647\r\n"
    with pytest.raises(_capi.HpRefused) as e:
        _device(bed_bytes, line * (2**21 + 8), tmp_path)
    assert (e.value.why, e.value.line) == (_capi.HP_TOTAL, 0)
    cols, totals = _device(bed_bytes, line * 2**21, tmp_path, "ok.matrix")
    assert totals[0] == 2**22 * (2**31 - 1) < 2**53 and not totals[1:].any()
    assert len(cols[4]) == 2**21 and (cols[4] == 2**31 - 1).all() and (cols[1] == 5000).all()


# ---- 5. the direct path --------------------------------------------------------------------------------------------------
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
    from fithic_amd import hicpro, tables
    case = hm.CASES["hp2_r0"]
    bed, matrix, bias = hm.case_inputs(case, tmp_path)
    outs = [str(tmp_path / n) for n in OUT_NAMES]
    hicpro.outputfithicform(bed, matrix, outs[0], outs[1], bias, outs[2], 0)

    def from_files(eng, chroms):
        con = tables.read_contacts(outs[0], chroms)
        fc, fm, fh = tables.read_fragments(outs[1], chroms)
        eng.load_fragments(fc, fm, fh, chroms.sort_rank())
        eng.load_bias(*tables.read_bias(outs[2], chroms))
        eng.load_contacts(con.chr1, con.mid1, con.chr2, con.mid2, con.count)

    def direct(eng, chroms):
        with hicpro.read(bed, matrix, bias, 0) as data:
            assert len(data) == 40000
            data.load_into(eng, chroms)

    want, got = _two_passes(from_files), _two_passes(direct)
    for (wp, wq), (gp, gq) in zip(want, got):
        assert len(wp) == 40000 and np.isfinite(wp).any()
        assert bits_equal(gp, wp) and bits_equal(gq, wq)
