"""GPU tests of the merge-filter path (fithic_amd.mergefilter, csrc/fhx_sigselect.hip): the subset and the merged file equal the
real script's after decompression (tests/golden/mergefilter), the subset equals the model's (tests/mergefilter_model.py) on
texts built round the 16 KB scan blocks and round batch edges, at 0 % and 100 % kept, for every threshold and class, every
refusal names the right line, two runs give the same bytes, and combine() equals the combine module on the written subset."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mergefilter_model as mm
from batch_env import batch_bytes
from conftest import ROOT
from test_mergefilter_host import MF, RUNS, THRESHOLDS, _gunzip, run_input

pytestmark = pytest.mark.gpu

BLOCK = 16384
HEADER = b"chr1\tfragmentMid1\tchr2\tfragmentMid2\tcontactCount\tp-value\tq-value\tbias1\tbias2\tExpCC\n"


def gpu_subset(data, fdr, tmp_path, batch=None, **kw):
    """the subset the device path makes for `data`, after checking its counts against the model"""
    from fithic_amd import mergefilter
    src = str(tmp_path / "sig.txt")
    with open(src, "wb") as f:
        f.write(data)
    with batch_bytes("FHX_MS_BATCH_BYTES", batch):
        got = mergefilter.select(src, fdr, **kw)
    text = got.subset_text()
    assert isinstance(text, bytes) and got.n_kept == text.count(b"\n")
    assert got.n_lines == len(mm.lines_of(gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data))
    assert set(got.stage_seconds()) == {"read_upload", "newline_scan", "select", "gather", "copy_out"}
    return text


def row(k, q, pad=0, sep=b"\t"):
    """one row of a significances file whose field 7 is q; `pad` more bytes in the trailing column"""
    return sep.join([b"chr%d" % (1 + k % 3), b"%d" % (5000 * (k % 900) + 2500), b"chr%d" % (1 + k % 3), b"%d" % (5000 * (k % 900 + k % 7 + 3) + 2500),
                     b"%d" % (5 + k % 90), b"1.000000e-09", q, b"1.000000", b"1.000000", b"2.5" + b"0" * pad]) + b"\n"


KEPT, DROPPED = b"1.000000e-03", b"9.000000e-01"                      # at fdr = 0.05


# ---- 1. goldens -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RUNS))
def test_device_path_writes_the_script_s_files(name, tmp_path):
    from fithic_amd import combine, mergefilter
    run = RUNS[name]
    src, sub, out = str(tmp_path / "sig.txt"), str(tmp_path / "fithic_subset.gz"), str(tmp_path / "merged.gz")
    with open(src, "wb") as f:
        f.write(run_input(run))
    got = mergefilter.select(src, run["fdr"])
    assert got.subset_text() == _gunzip(os.path.join(MF, run["subset"]))
    got.write_subset(sub)
    assert _gunzip(sub) == got.subset_text()
    combine.write_merged(out, *got.merged(run["res"]), run["res"])
    assert _gunzip(out) == _gunzip(os.path.join(MF, run["merged"]))


@pytest.mark.parametrize("name, gzipped", [("mfa", True), ("mfq_5", False), ("mfe", False)])
def test_command_line_writes_the_script_s_files(name, gzipped, tmp_path):
    run = RUNS[name]
    src = str(tmp_path / ("sig.gz" if gzipped else "sig.txt"))
    with open(src, "wb") as f:
        f.write(gzip.compress(run_input(run)) if gzipped else run_input(run))
    out = str(tmp_path / "made" / "here" / "merged.gz")
    r = subprocess.run([sys.executable, "-m", "fithic_amd.mergefilter", src, str(run["res"]), out, run["fdr"], "ignored/"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _gunzip(str(tmp_path / "made" / "here" / "fithic_subset.gz")) == _gunzip(os.path.join(MF, run["subset"]))
    assert _gunzip(out) == _gunzip(os.path.join(MF, run["merged"]))


# ---- 2. block and batch edges -----------------------------------------------------------------------------------------------
def edge_text(kind, n_edges=4):
    """a text in which, at every 16 KB edge, a line ends at the edge, starts at it, straddles it, or has its field 7 across it;
    the line at the edge is kept at the odd edges and dropped at the even ones, between a dropped and a kept neighbour"""
    rng = np.random.default_rng(5)
    buf = HEADER
    for k in range(1, n_edges + 1):
        edge = k * BLOCK
        while len(buf) < edge - 600:
            buf += row(len(buf), b"%d.%06de-%02d" % (rng.integers(1, 10), rng.integers(0, 1000000), rng.integers(0, 4)), sep=[b"\t", b" "][len(buf) % 2])
        line = row(k, KEPT if k % 2 else DROPPED)
        field_at = line.index(b"e-0") - 4                             # the edge falls inside the digits of field 7
        at = {"ends_at_edge": len(line), "starts_at_edge": 0, "newline_first": -1, "straddles": 9, "field_straddles": field_at}[kind]
        before = row(k + 1, DROPPED if k % 2 else KEPT)
        slack = edge - at - len(buf) - len(before)
        assert slack > 0
        buf += row(k + 1, DROPPED if k % 2 else KEPT, pad=slack) + line + row(k + 2, DROPPED if k % 2 else KEPT)
        assert buf[edge - at:].startswith(line)                       # byte `at` of the line is the first byte of the block
    return buf + row(7, KEPT) * 3


EDGE_KINDS = ["ends_at_edge", "starts_at_edge", "newline_first", "straddles", "field_straddles"]


@pytest.mark.parametrize("kind", EDGE_KINDS)
def test_subset_equals_the_model_at_block_edges(kind, tmp_path):
    data = edge_text(kind)
    want = mm.select(data, "0.05")
    assert 0 < want.count(b"\n") < data.count(b"\n") - 1
    assert gpu_subset(data, "0.05", tmp_path) == want


@pytest.mark.parametrize("kind", EDGE_KINDS)
@pytest.mark.parametrize("batch", [8192, 2 * BLOCK - 100])
def test_subset_equals_the_model_when_batch_edges_fall_inside_the_file(kind, batch, tmp_path):
    data = row(0, KEPT) + edge_text(kind)[len(HEADER):]               # line 1 is a data row that passes: it is dropped, and only
    assert len(data) > 2 * batch and mm.keeps(data.split()[6], b"0.05")       # it - the first line of a later batch stays
    want = mm.select(data, "0.05")
    assert gpu_subset(data, "0.05", tmp_path, batch) == want
    assert gpu_subset(data, "0.05", tmp_path, batch, skip_first_line=False) == data[:data.index(b"\n") + 1] + want


# ---- 3. keep patterns -------------------------------------------------------------------------------------------------------
def test_nothing_kept_everything_kept_only_a_header_and_no_text(tmp_path):
    body = b"".join(row(k, b"%d.000000e-%02d" % (1 + k % 9, 1 + k % 5)) for k in range(700))     # three blocks
    assert gpu_subset(HEADER + body, "0", tmp_path) == b""
    assert gpu_subset(HEADER + body, "5", tmp_path) == body
    assert gpu_subset(body, "5", tmp_path, skip_first_line=False) == body
    assert gpu_subset(body[:-1], "5", tmp_path, skip_first_line=False) == body              # the newline the last line lacked
    assert gpu_subset(HEADER + body[:-1], "5", tmp_path, 8192) == body
    assert gpu_subset(HEADER, "0.05", tmp_path) == b""
    assert gpu_subset(HEADER[:-1], "0.05", tmp_path) == b""
    assert gpu_subset(b"any\x7eheader | at all", "0.05", tmp_path) == b""
    assert gpu_subset(b"", "0.05", tmp_path) == b""
    assert gpu_subset(b"", "0.05", tmp_path, skip_first_line=False) == b""


def test_runs_of_kept_lines_that_cross_wave_boundaries(tmp_path):
    """short lines, 300 and more per block: kept in runs of 1 to 150, so that runs start and end inside, and span, the waves of a
    block and the 256-line rounds of the gather"""
    rng = np.random.default_rng(9)
    lines, keep = [], True
    while len(lines) < 2000:
        lines += [b"a b c d e f %s\n" % (KEPT if keep else DROPPED)] * int(rng.integers(1, 150))
        keep = not keep
    data = HEADER + b"".join(lines)
    want = mm.select(data, "0.05")
    assert want.count(b"\n") > 64 * 8 and len(lines[0]) * 300 < BLOCK
    assert gpu_subset(data, "0.05", tmp_path) == want


def test_70000_lines_with_every_997th_kept(tmp_path):
    data = HEADER + b"".join(row(k, KEPT if k % 997 == 0 else DROPPED) for k in range(70000))
    want = mm.select(data, "0.05")
    assert want.count(b"\n") == 71
    assert gpu_subset(data, "0.05", tmp_path) == want


def test_a_text_of_three_upload_chunks_refills_the_first_pinned_buffer(tmp_path):
    """The uploader fills two pinned 32 MiB buffers in turn: a text just over 64 MiB + 16 KB, one batch at the default batch size,
    is three chunks, so buffer 0 is filled again - after the copy engine has drained it.  Two lines alternate, A kept and B
    dropped as the model classifies them; the subset is then A repeated."""
    a, b = row(1, KEPT), row(2, DROPPED)
    assert mm.select(HEADER + a + b, "0.05") == a
    pairs = ((64 << 20) + BLOCK - len(HEADER)) // len(a + b) + 1
    data = HEADER + (a + b) * pairs
    assert (64 << 20) + BLOCK < len(data) <= (64 << 20) + BLOCK + len(a + b) and "FHX_MS_BATCH_BYTES" not in os.environ
    src, out = str(tmp_path / "sig.txt"), str(tmp_path / "subset.txt")
    with open(src, "wb") as f:
        f.write(data)
    # in a process of its own: a wait on an event that never fires ends at the time limit, as one failed test
    code = ("import json, sys\n"
            "from fithic_amd import _capi, mergefilter as mf\n"
            "ms = _capi.MsContext(0)\n"
            "n = ms.select_file(sys.argv[1], b'0.05', mf.key_bound('0.05'), True)\n"
            "open(sys.argv[2], 'wb').write(ms.subset())\n"
            "print(json.dumps(dict(ms.counts(), returned=n)))\n"
            "ms.close()\n")
    r = subprocess.run([sys.executable, "-c", code, src, out], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout) == dict(lines=1 + 2 * pairs, kept=pairs, bytes=pairs * len(a), returned=pairs * len(a))
    with open(out, "rb") as f:
        assert f.read() == a * pairs


# ---- 4. thresholds and classes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("fdr", THRESHOLDS)
def test_rows_at_the_key_bound_and_in_every_class(fdr, strict, tmp_path):
    from fithic_amd import mergefilter as mf
    bound = mf.key_bound(fdr, strict)
    fields = ["0.000000e+00", "0.000000e-07", "1.000000e-320", "2.225073e-308", "9.000000e-315", "4.940656e-324", "1.000000e+309", "4.000000e+310",
              "9.999999e+999", "2.225074e-308", "9.999999e+307", "1.000000e-03", "5.000000e-001"]
    if bound:
        e, m = divmod(bound, 10000000)
        at = e * mf._MANTISSAS + m - 1000000
        fields += [mf._field(i) for i in range(max(mf._LOWEST, at - 2), min(mf._HIGHEST, at + 2) + 1)]
    data = b"".join(row(k, f.encode(), sep=[b"\t", b" ", b" \t"][k % 3]) for k, f in enumerate(fields * 3))
    want = mm.select(data, fdr, strict=strict, skip_first_line=False)
    assert gpu_subset(data, fdr, tmp_path, strict=strict, skip_first_line=False) == want
    kept = set(line.split()[6] for line in want.splitlines())
    assert (b"0.000000e+00" in kept) == (not strict or float(fdr) > 0)
    if fdr == "5":
        assert {b"1.000000e-320", b"2.225073e-308", b"1.000000e+309", b"4.000000e+310", b"4.940656e-324"} <= kept
        assert not {b"9.000000e-315", b"9.999999e+999"} & kept
    if fdr == "0.05":
        assert not {b"1.000000e-320", b"2.225073e-308", b"1.000000e+309"} & kept and b"2.225074e-308" in kept


def test_two_runs_give_the_same_bytes(tmp_path):
    data = edge_text("field_straddles") + run_input(RUNS["mfq_5"])
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    first = gpu_subset(data, "0.05", tmp_path / "a")
    assert first == gpu_subset(data, "0.05", tmp_path / "b") == gpu_subset(data, "0.05", tmp_path / "b", 8192)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
GOOD = row(1, KEPT)
BAD_LINES = {"six tokens": (b"chr1 1 chr1 2 3 1.000000e-09", mm.TOKENS), "empty line": (b"", mm.TOKENS), "blank line": (b" \t ", mm.TOKENS),
             "a sign": (b"c 1 c 2 3 4 -1.000000e-03", mm.FIELD), "a plus": (b"c 1 c 2 3 4 +1.000000e-03", mm.FIELD),
             "nan": (b"c 1 c 2 3 4 nan", mm.FIELD), "-nan": (b"c 1 c 2 3 4 -nan", mm.FIELD), "inf": (b"c 1 c 2 3 4 inf", mm.FIELD),
             "first digit 0": (b"c 1 c 2 3 4 0.100000e-03", mm.FIELD), "five digits": (b"c 1 c 2 3 4 1.00000e-03", mm.FIELD),
             "seven digits": (b"c 1 c 2 3 4 1.0000000e-03", mm.FIELD), "one exponent digit": (b"c 1 c 2 3 4 1.000000e-3", mm.FIELD),
             "four exponent digits": (b"c 1 c 2 3 4 1.000000e-0003", mm.FIELD), "capital E": (b"c 1 c 2 3 4 1.000000E-03", mm.FIELD),
             "plain decimal": (b"c 1 c 2 3 4 0.05", mm.FIELD), "exponent 308": (b"c 1 c 2 3 4 1.000000e+308", mm.FIELD),
             "no exponent sign": (b"c 1 c 2 3 4 1.000000e0003", mm.FIELD), "comma": (b"c 1 c 2 3 4 1,000000e-03", mm.FIELD),
             "NUL": (b"c 1 c 2 3 4 1.000000e-03 \x00", mm.BYTES), "non-ASCII": (b"c\xe9 1 c 2 3 4 1.000000e-03", mm.BYTES),
             "CR": (b"c 1 c 2 3 4 1.000000e-03\r", mm.BYTES), "DEL": (b"c 1 c 2 3 4 1.000000e-03 \x7f", mm.BYTES),
             "long line": (b"c 1 c 2 3 4 1.000000e-03 " + b"x" * 4072, mm.LONG_LINE)}


def _refusal_of(data, tmp_path, batch=None, **kw):
    from fithic_amd import _capi, mergefilter as mf
    src = str(tmp_path / "bad.txt")
    with open(src, "wb") as f:
        f.write(data)
    ms = _capi.MsContext(0)
    try:
        with batch_bytes("FHX_MS_BATCH_BYTES", batch), pytest.raises(_capi.MsRefused) as e:
            ms.select_file(src, b"0.05", mf.key_bound("0.05"), True, False, kw.get("skip_first_line", True))
        assert ms.counts() == dict(lines=0, kept=0, bytes=0) and ms.subset() == b""
        return e.value.why, e.value.line
    finally:
        ms.close()


@pytest.mark.parametrize("kind", sorted(BAD_LINES))
def test_a_bad_line_is_refused_with_its_line_number(kind, tmp_path):
    bad, why = BAD_LINES[kind]
    data = HEADER + GOOD * 400 + bad + b"\n" + GOOD * 50                # line 402 lies in the second 16 KB block
    assert len(HEADER + GOOD * 400) > BLOCK
    with pytest.raises(mm.Refused) as e:
        mm.select(data, "0.05")
    assert (e.value.why, e.value.line) == (why, 402)
    assert _refusal_of(data, tmp_path) == (why, 402)


def test_a_line_of_4096_bytes_is_taken_and_the_header_is_not_parsed(tmp_path):
    longest = b"c 1 c 2 3 4 1.000000e-03 " + b"x" * 4071
    assert len(longest) == 4096
    assert gpu_subset(HEADER + longest + b"\n" + GOOD, "0.05", tmp_path) == longest + b"\n" + GOOD
    assert gpu_subset(b"\n" + GOOD, "0.05", tmp_path) == GOOD          # an empty first line is only dropped
    assert _refusal_of(b"head\x00er\n" + GOOD, tmp_path) == (mm.BYTES, 1)      # the byte rules hold for it
    assert _refusal_of(b"h" * 4097 + b"\n" + GOOD, tmp_path) == (mm.LONG_LINE, 1)
    assert _refusal_of(b"header\n" + GOOD, tmp_path, skip_first_line=False) == (mm.TOKENS, 1)


def test_the_smaller_of_two_bad_lines_is_reported_from_a_later_block_and_a_later_batch(tmp_path):
    data = HEADER + GOOD * 450 + b"c 1 c 2 3 4\n" + GOOD * 400 + b"c 1 c 2 3 4 nan\n" + GOOD * 10
    assert len(HEADER + GOOD * 450) > BLOCK and len(GOOD * 400) > BLOCK
    assert _refusal_of(data, tmp_path) == (mm.TOKENS, 452)
    assert _refusal_of(data, tmp_path, 8192) == (mm.TOKENS, 452)
    assert _refusal_of(data, tmp_path, 2 * BLOCK - 100) == (mm.TOKENS, 452)
    assert _refusal_of(HEADER + GOOD * 5 + b"c 1 c 2 3 4 1.000000e-03\r", tmp_path) == (mm.BYTES, 7)       # a \r that ends the text


SIX_TOKENS = b"chr1 1 chr1 2 3 1.000000e-09\n"


def third_batch_texts():
    """300 ordinary rows, two in three of them kept, that take three or four batches of 8192 bytes; and the same text with a line
    of six tokens as line 252, which lies in the third batch at the earliest: 250 rows before it are more than two batches"""
    rows = [row(k, KEPT if k % 3 else DROPPED) for k in range(300)]
    good, bad = HEADER + b"".join(rows), HEADER + b"".join(rows[:250]) + SIX_TOKENS + b"".join(rows[250:])
    assert 2 * 8192 < len(HEADER + b"".join(rows[:250])) and len(bad) < 4 * 8192
    assert mm.select(HEADER + b"".join(rows[:100]), "0.05")             # the first batch alone keeps lines
    return good, bad


def test_a_refusal_in_the_third_batch_leaves_nothing(tmp_path):
    _, bad = third_batch_texts()
    assert _refusal_of(bad, tmp_path, 8192) == (mm.TOKENS, 252)         # counts all 0 and an empty subset: _refusal_of


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
                ms.select_file(str(tmp_path / "bad.txt"), b"0.05", mf.key_bound("0.05"), True)
            assert (e.value.why, e.value.line) == (mm.TOKENS, 252)
            want = mm.select(good, "0.05")
            assert ms.select_file(str(tmp_path / "good.txt"), b"0.05", mf.key_bound("0.05"), True) == len(want)
        assert ms.subset() == want and ms.counts() == dict(lines=301, kept=200, bytes=len(want))
    finally:
        ms.close()


def test_a_refused_file_leaves_no_output_file(tmp_path):
    from fithic_amd import mergefilter
    src = str(tmp_path / "bad.txt")
    with open(src, "wb") as f:
        f.write(HEADER + GOOD * 2 + b"c 1 c 2 3 4 0.05\n")
    with pytest.raises(ValueError, match="line 4.*The reference accepts this"):
        mergefilter.select(src, "0.05")
    out = tmp_path / "out" / "merged.gz"
    with pytest.raises(ValueError, match="line 4"):
        mergefilter.main([src, "5000", str(out), "0.05"])
    with pytest.raises(ValueError, match="fdr"):
        mergefilter.main([src, "5000", str(out), "5%"])
    assert not (tmp_path / "out").exists()


# ---- 6. combine() -----------------------------------------------------------------------------------------------------------
def test_combine_equals_the_combine_module_on_the_written_subset(tmp_path):
    from fithic_amd import combine, mergefilter
    run = RUNS["mfa"]
    src, sub = str(tmp_path / "sig.txt"), str(tmp_path / "fithic_subset.gz")
    with open(src, "wb") as f:
        f.write(run_input(run))
    got = mergefilter.select(src, run["fdr"])
    got.write_subset(sub)
    names, rec, info = got.combine(run["res"])
    want_names, want_rec, want_info = combine.combine_records(combine.read_significances(sub, 0), run["res"])
    assert names == want_names and rec.dtype == want_rec.dtype and rec.tobytes() == want_rec.tobytes()
    assert info.as_dict() == want_info.as_dict() and info.selected == len(rec) > 10
    assert combine.format_lines(names, rec, run["res"]) == combine.format_lines(want_names, want_rec, run["res"])
