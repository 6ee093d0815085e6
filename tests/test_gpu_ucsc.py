"""GPU tests of the interact-track path (fithic_amd.ucsc, csrc/fhx_sigtrack.inc, csrc/fhx_score.hpp): the track equals the real
script's file (tests/golden/ucsc) and the model's (tests/ucsc_model.py) on the fields whose score lies next to a boundary, on
texts built round the 16 KB scan blocks and round batch edges, at 0 % and 100 % kept, on the shortest lines (the expansion
case), on files whose every kept row is deferred; every refusal names the right line, the header rule holds on line 1 only,
two runs give the same bytes, and the kernel certifies all but 1 in 1000 of the scores of a random file."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import ucsc_model as um
from batch_env import batch_bytes
from conftest import ROOT
from test_gpu_mergefilter import BLOCK, DROPPED, EDGE_KINDS, HEADER, KEPT, edge_text, row, third_batch_texts
from test_ucsc_host import RUNS, random_fields, run_input, run_track

pytestmark = pytest.mark.gpu


def gpu_track(data, qval, tmp_path, batch=None):
    """the Track the device path makes for `data`, after checking its counts against the model"""
    from fithic_amd import ucsc
    src = str(tmp_path / "sig.txt")
    with open(src, "wb") as f:
        f.write(data)
    with batch_bytes("FHX_MS_BATCH_BYTES", batch):
        got = ucsc.track(src, qval)
    text = got.text()
    assert isinstance(text, bytes) and text.startswith(um.HEAD) and got.n_kept == text.count(b"\n") - 2
    assert got.n_lines == len(um.mm.lines_of(gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data))
    assert 0 <= got.n_deferred <= got.n_kept
    assert list(got.stage_seconds()) == ["read_upload", "newline_scan", "select", "deferred_round_trip", "format", "copy_out"]
    return got


def model(data, qval):
    return um.track(data, qval)[0]


# ---- 1. goldens -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RUNS))
def test_device_path_writes_the_script_s_file(name, tmp_path):
    run = RUNS[name]
    got = gpu_track(run_input(run), run["qval"], tmp_path)
    assert got.text() == run_track(run)
    got.write(str(tmp_path / "track.txt"))
    with open(str(tmp_path / "track.txt"), "rb") as f:
        assert f.read() == run_track(run)


@pytest.mark.parametrize("name, gzipped", [("uca", True), ("ucq_5", False)])
def test_command_line_writes_the_script_s_file(name, gzipped, tmp_path):
    run = RUNS[name]
    src, out = str(tmp_path / ("sig.gz" if gzipped else "sig.txt")), str(tmp_path / "track.txt")
    with open(src, "wb") as f:
        f.write(gzip.compress(run_input(run)) if gzipped else run_input(run))
    r = subprocess.run([sys.executable, "-m", "fithic_amd.ucsc", src, out, run["qval"]], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out, "rb") as f:
        assert f.read() == run_track(run)


# ---- 2. the score -----------------------------------------------------------------------------------------------------------
def test_scores_next_to_an_integer_or_a_rounding_boundary(tmp_path):
    data = um.rows_of(um.near_boundary_fields())
    got = gpu_track(data, "5", tmp_path)
    assert got.n_kept == 800 and got.text() == model(data, "5")


def test_a_file_whose_every_kept_row_is_deferred(tmp_path):
    fields = [b"1.000000e-%02d" % k for k in range(1, 308)] + [b"1.000000e+00", b"1.000000e-320", b"1.000000e+309", b"1.000000e-310"]
    fields = fields * 3 + [b"9.000000e+00"] * 5                       # 9 is dropped at 5: the deferred slots skip dropped lines
    fields = [fields[(11 * k) % len(fields)] for k in range(len(fields))]
    assert sorted(fields).count(b"9.000000e+00") == 5 and len(fields) == 311 * 3 + 5
    data = um.rows_of(fields)
    for batch in (None, 8192):
        got = gpu_track(data, "5", tmp_path, batch)
        assert got.n_deferred == got.n_kept == 311 * 3 and got.text() == model(data, "5")


def test_the_kernel_certifies_all_but_1_in_1000_scores_of_a_random_file(tmp_path):
    """2 * 10^5 numeric rows, mantissas uniform, exponents -307..0, no power of ten: the geometry defers about 2 eps / 1e-6 of them"""
    rng = np.random.default_rng(21)
    mant, ex = rng.integers(1000001, 10000000, 200000), rng.integers(-307, 1, 200000)
    data = um.rows_of([b"%d.%06de%s%02d" % (m // 1000000, m % 1000000, b"-" if x < 0 else b"+", abs(x)) for m, x in zip(mant.tolist(), ex.tolist())],
                      seps=(b" ",))
    got = gpu_track(data, "5", tmp_path)
    print("kept %d, deferred %d" % (got.n_kept, got.n_deferred))
    assert got.n_kept > 199000 and got.n_deferred * 1000 <= got.n_kept
    assert got.text() == model(data, "5")


# ---- 3. block and batch edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", EDGE_KINDS)
def test_track_equals_the_model_at_block_edges(kind, tmp_path):
    data = edge_text(kind)
    want = model(data, "0.05")
    assert 2 < want.count(b"\n") < data.count(b"\n")
    assert gpu_track(data, "0.05", tmp_path).text() == want


@pytest.mark.parametrize("kind", EDGE_KINDS)
@pytest.mark.parametrize("batch", [8192, 2 * BLOCK - 100])
def test_nr_goes_on_across_the_batches(kind, batch, tmp_path):
    data = row(0, KEPT) + edge_text(kind)[len(HEADER):]               # line 1 is a data row that passes: the track keeps it
    want = model(data, "0.05")
    assert len(data) > 2 * batch and want.splitlines()[2].split()[3] == b"1"
    got = gpu_track(data, "0.05", tmp_path, batch)
    assert got.text() == want
    assert int(got.text().splitlines()[-1].split()[3]) == got.n_kept > 100


# ---- 4. keep patterns -------------------------------------------------------------------------------------------------------
def test_nothing_kept_everything_kept_only_a_header_and_no_text(tmp_path):
    fields = [b"%d.%06de-%02d" % (1 + k % 9, 7919 * k % 1000000, 1 + k % 5) for k in range(700)]
    body = b"".join(row(k, f) for k, f in enumerate(fields))         # three blocks
    assert gpu_track(HEADER + body, "0", tmp_path).text() == um.HEAD
    for data in (HEADER + body, body, body[:-1]):
        got = gpu_track(data, "5", tmp_path)
        assert got.n_kept == 700 and got.text() == model(data, "5")
    assert gpu_track(HEADER + body[:-1], "5", tmp_path, 8192).text() == model(HEADER + body, "5")
    assert gpu_track(HEADER, "0.05", tmp_path).text() == um.HEAD
    assert gpu_track(HEADER[:-1], "0.05", tmp_path).text() == um.HEAD
    empty = gpu_track(b"", "0.05", tmp_path)
    assert empty.text() == um.HEAD and (empty.n_lines, empty.n_kept, empty.n_deferred) == (0, 0, 0)


def test_the_shortest_lines_all_kept_grow_to_three_times_their_bytes(tmp_path):
    data = b"a 1 a 1 1 1 0.000000e+00\n" * 4000 + b"b 0 b 0 1 1 2.500000e-01\n" * 3000                # 650 lines a block
    got = gpu_track(data, "5", tmp_path)
    assert got.n_kept == 7000 and got.n_deferred == 0 and len(got.text()) - len(um.HEAD) > 2.5 * len(data)
    assert got.text() == model(data, "5")
    assert gpu_track(data, "5", tmp_path, 8192).text() == got.text()


def test_the_longest_track_lines(tmp_path):
    """names of 63 bytes and midpoints of 9 digits: a round of 256 such lines is several 16 KB windows of the formatter"""
    a, b = b"A" * 63, b"chrB" + b"b" * 59
    lines = [b"%s 999999999 %s 99999999%d 1 1 %s\n" % (a, b, k % 10, [b"1.234567e-100", b"1.000000e-200", b"9.000000e+00"][k % 3]) for k in range(900)]
    data = b"".join(lines)
    got = gpu_track(data, "5", tmp_path)
    assert got.n_kept == 600 and got.n_deferred == 300 and got.text() == model(data, "5")
    assert max(len(line) for line in got.text().splitlines()) > 300


def test_runs_of_kept_lines_that_cross_wave_and_round_boundaries(tmp_path):
    rng = np.random.default_rng(9)
    lines, keep = [], True
    while len(lines) < 2000:
        n = int(rng.integers(1, 150))
        lines += [b"a %d c %d e f %s\n" % (len(lines) + k, 7 * k, (KEPT if k % 5 else b"3.141593e-02") if keep else DROPPED) for k in range(n)]
        keep = not keep
    data = HEADER + b"".join(lines)
    want = model(data, "0.05")
    assert want.count(b"\n") > 64 * 8 and max(map(len, lines)) * 300 < BLOCK
    got = gpu_track(data, "0.05", tmp_path)
    assert got.text() == want and 0 < got.n_deferred < got.n_kept       # 1.000000e-03 is a power of ten


def test_two_runs_give_the_same_bytes(tmp_path):
    data = edge_text("field_straddles") + run_input(RUNS["ucq_5"])
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    first = gpu_track(data, "0.05", tmp_path / "a").text()
    assert first == gpu_track(data, "0.05", tmp_path / "b").text() == gpu_track(data, "0.05", tmp_path / "b", 8192).text()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
GOOD = row(1, KEPT)
BAD_LINES = {"six tokens": (b"chr1 1 chr1 2 3 1.000000e-09", um.TOKENS), "empty line": (b"", um.TOKENS),
             "a sign in field 7": (b"c 1 c 2 3 4 -1.000000e-03", um.FIELD), "nan": (b"c 1 c 2 3 4 nan", um.FIELD),
             "a header on a later line": (b"c 1 c 2 3 4 q-value", um.FIELD), "plain decimal": (b"c 1 c 2 3 4 0.05", um.FIELD),
             "exponent 308": (b"c 1 c 2 3 4 1.000000e+308", um.FIELD), "NUL": (b"c 1 c 2 3 4 1.000000e-03 \x00", um.BYTES),
             "CR": (b"c 1 c 2 3 4 1.000000e-03\r", um.BYTES), "long line": (b"c 1 c 2 3 4 1.000000e-03 " + b"x" * 4072, um.LONG_LINE),
             "a sign in token 2": (b"c -1 c 2 3 4 1.000000e-03", um.MIDPOINT), "a plus in token 4": (b"c 1 c +2 3 4 1.000000e-03", um.MIDPOINT),
             "ten digits": (b"c 1 c 2147483647 3 4 1.000000e-03", um.MIDPOINT), "a fraction": (b"c 1.5 c 2 3 4 1.000000e-03", um.MIDPOINT),
             "a name as midpoint": (b"c mid c 2 3 4 9.000000e-01", um.MIDPOINT), "token 1 of 64 bytes": (b"c" * 64 + b" 1 c 2 3 4 1.000000e-03", um.NAME),
             "token 3 of 64 bytes": (b"c 1 " + b"d" * 64 + b" 2 3 4 9.000000e-01", um.NAME)}


def _refusal_of(data, tmp_path, batch=None):
    from fithic_amd import _capi, mergefilter as mf
    src = str(tmp_path / "bad.txt")
    with open(src, "wb") as f:
        f.write(data)
    ms = _capi.MsContext(0)
    try:
        with batch_bytes("FHX_MS_BATCH_BYTES", batch), pytest.raises(_capi.MsRefused) as e:
            ms.track_file(src, b"0.05", mf.key_bound("0.05", True), True)
        assert ms.track_counts() == dict(lines=0, kept=0, deferred=0, bytes=0) and ms.track() == b""
        return e.value.why, e.value.line
    finally:
        ms.close()


@pytest.mark.parametrize("kind", sorted(BAD_LINES))
def test_a_bad_line_is_refused_with_its_line_number(kind, tmp_path):
    bad, why = BAD_LINES[kind]
    data = HEADER + GOOD * 400 + bad + b"\n" + GOOD * 50                # line 402 lies in the second 16 KB block
    assert len(HEADER + GOOD * 400) > BLOCK
    with pytest.raises(um.Refused) as e:
        um.track(data, "0.05")
    assert (e.value.why, e.value.line) == (why, 402)
    assert _refusal_of(data, tmp_path) == (why, 402)


def test_names_of_63_bytes_and_midpoints_of_9_digits_are_taken(tmp_path):
    data = b"c" * 63 + b" 000000000 " + b"d" * 63 + b" 999999999 3 4 1.000000e-03\n" + GOOD
    assert gpu_track(data, "0.05", tmp_path).text() == model(data, "0.05")


def test_the_header_rule_holds_on_line_1_only(tmp_path):
    assert gpu_track(HEADER + GOOD, "0.05", tmp_path).text() == model(GOOD, "0.05")
    assert gpu_track(b"c mid c mid n p Q-value\n" + GOOD, "0.05", tmp_path).text() == model(GOOD, "0.05")      # nothing else of it is parsed
    assert gpu_track(GOOD + GOOD, "0.05", tmp_path).text() == model(GOOD + GOOD, "0.05")                      # a data row on line 1 is kept
    assert _refusal_of(GOOD + HEADER + GOOD, tmp_path) == (um.FIELD, 2)
    assert _refusal_of(b"chr1 fragmentMid1 chr2 fragmentMid2 contactCount p-value\n" + GOOD, tmp_path) == (um.TOKENS, 1)
    assert _refusal_of(b"\n" + GOOD, tmp_path) == (um.TOKENS, 1)
    assert _refusal_of(b"c 1 c 2 3 4 -1.000000e-03\n" + GOOD, tmp_path) == (um.FIELD, 1)               # no letter: parsed as a row
    assert _refusal_of(b"head\x00er a b c d e q-value\n" + GOOD, tmp_path) == (um.BYTES, 1)
    assert _refusal_of(GOOD * 300 + HEADER + GOOD * 300, tmp_path, 8192) == (um.FIELD, 301)           # the first line of a later batch


def test_the_smaller_of_two_bad_lines_is_reported_from_a_later_block_and_a_later_batch(tmp_path):
    data = HEADER + GOOD * 450 + b"c x c 2 3 4 1.000000e-03\n" + GOOD * 400 + b"c 1 c 2 3 4 nan\n" + GOOD * 10
    assert len(HEADER + GOOD * 450) > BLOCK and len(GOOD * 400) > BLOCK
    for batch in (None, 8192, 2 * BLOCK - 100):
        assert _refusal_of(data, tmp_path, batch) == (um.MIDPOINT, 452)


def test_a_refusal_in_the_third_batch_leaves_nothing(tmp_path):
    _, bad = third_batch_texts()
    assert model(bad[:bad.rindex(b"\n", 0, 8192) + 1], "0.05") != um.HEAD       # the first batch alone keeps lines
    assert _refusal_of(bad, tmp_path, 8192) == (um.TOKENS, 252)         # counts all 0 and an empty track: _refusal_of


def test_a_good_call_after_a_refused_one_gives_the_model_s_bytes(tmp_path):
    from fithic_amd import _capi, mergefilter as mf
    good, bad = third_batch_texts()
    for name, data in (("bad.txt", bad), ("good.txt", good)):
        with open(str(tmp_path / name), "wb") as f:
            f.write(data)
    ms = _capi.MsContext(0)
    try:
        with batch_bytes("FHX_MS_BATCH_BYTES", 8192):
            with pytest.raises(_capi.MsRefused) as e:
                ms.track_file(str(tmp_path / "bad.txt"), b"0.05", mf.key_bound("0.05", True), True)
            assert (e.value.why, e.value.line) == (um.TOKENS, 252)
            want = model(good, "0.05")
            assert ms.track_file(str(tmp_path / "good.txt"), b"0.05", mf.key_bound("0.05", True), True) == len(want)
        assert ms.track() == want
        counts = ms.track_counts()
        assert (counts["lines"], counts["kept"], counts["bytes"]) == (301, 200, len(want))
    finally:
        ms.close()


def test_a_refused_file_leaves_no_output_file(tmp_path):
    from fithic_amd import ucsc
    src, out = str(tmp_path / "bad.txt"), tmp_path / "track.txt"
    with open(src, "wb") as f:
        f.write(HEADER + GOOD * 2 + b"c 1 c 2.5 3 4 1.000000e-03\n")
    with pytest.raises(ValueError, match="line 4.*tokens 2 and 4.*The reference accepts this"):
        ucsc.main([src, str(out), "0.05"])
    with pytest.raises(ValueError, match="fdr"):
        ucsc.main([src, str(out), "5%"])
    assert not out.exists()
