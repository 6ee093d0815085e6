"""GPU tests of the Juicer dump path (fithic_amd.juicer, csrc/fhx_juicer.hip): the written files equal the real reference's
(tests/golden/juicer) through convert() and through both command lines, the bytes equal the model's (tests/juicer_model.py) on
texts built around the 16 KB scan blocks, around batch edges, around the 256-line rounds of the format kernel and at the largest
amplification, every refusal names the right line and leaves nothing written, two runs give the same bytes, and read() feeds an
Engine the same rows as the written file does."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import juicer_model as jm
from batch_env import batch_bytes
from conftest import ROOT, bits_equal
from test_juicer_host import BAD_BOTH, BAD_MIDPOINT, GOOD, RUNS, _gunzip, run_input, run_output

pytestmark = pytest.mark.gpu

BLOCK = 16384


def gpu_bytes(data, res, tmp_path, batch=None, chr1="1", chr2="X", out="out.gz"):
    """the (decompressed) bytes convert() writes for the dump text `data`"""
    from fithic_amd import juicer
    src, dst = str(tmp_path / "dump.txt"), str(tmp_path / out)
    with open(src, "wb") as f:
        f.write(data)
    with batch_bytes("FHX_JC_BATCH_BYTES", batch):
        n = juicer.convert(src, chr1, chr2, dst, res)
    with open(dst, "rb") as f:
        raw = f.read()
    made = gzip.decompress(raw) if dst.endswith(".gz") else raw
    assert made.count(b"\n") == n
    return made


def model_bytes(data, res, chr1="1", chr2="X"):
    return jm.convert(data, chr1.encode(), chr2.encode(), res)


# ---- 1. goldens -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RUNS))
def test_convert_writes_the_reference_s_file(name, tmp_path):
    run = RUNS[name]
    want = run_output(run)
    for out in (["out.gz"] if run["mode"] == "verbatim" else ["out.txt", "out.gz"]):                # .gz in midpoint mode: the extension
        assert gpu_bytes(run_input(run), run["resolution"], tmp_path, None, run["chr1"], run["chr2"], out) == want
    if run["mode"] == "verbatim":
        with open(str(tmp_path / "out.gz"), "rb") as f:
            assert f.read(2) == b"\x1f\x8b"                                                        # the old script always gzips


def _echo(stdout):
    return [line for line in stdout.splitlines() if line.split(":")[0] in ("CHR1", "CHR2", "resolution", "datatype", "Norm")]


@pytest.mark.parametrize("name,out", [("jvq_01_1e3", "o.gz"), ("jvn", "o.gz"), ("jmx_r5000", "o.txt"), ("jmo_r10001", "o.txt.gz")])
def test_command_lines_write_the_reference_s_file(name, out, tmp_path):
    run = RUNS[name]
    src, dst = str(tmp_path / "dump.txt"), str(tmp_path / out)
    with open(src, "wb") as f:
        f.write(run_input(run))
    if run["mode"] == "verbatim":
        argv = [src, run["chr1"], run["chr2"], dst]
    else:
        argv = ["--dump", src, "--CHR1", run["chr1"], "--CHR2", run["chr2"], "--resolution", str(run["resolution"]), "--datatype", "observed",
                "--Norm", "NONE", "--outFile", dst]
    r = subprocess.run([sys.executable, "-m", "fithic_amd.juicer"] + argv, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    if run["mode"] == "verbatim":
        assert r.stdout == ""
    else:
        assert _echo(r.stdout) == _echo(run["stdout"]) and len(_echo(r.stdout)) == 5
        assert "OutFile: %s" % os.path.realpath(dst) in r.stdout.splitlines()
    with open(dst, "rb") as f:
        raw = f.read()
    assert (gzip.decompress(raw) if out.endswith(".gz") else raw) == run_output(run)


# ---- 2. block, batch and round edges ----------------------------------------------------------------------------------------------
def _line(k, n=None):
    """a line both modes take (bins on the 5000 grid); n: its exact length with the newline, the slack being blanks"""
    x, y, c = b"%d" % (k % 4000 * 5000), b"%d" % ((k % 4000 + k % 37) * 5000), b"%d" % (k % 977)
    if n is None:
        return x + b"\t" + y + b"\t" + c + b"\n"
    pad = n - len(x) - len(y) - len(c) - 2
    assert 1 <= pad <= 4090
    return x + b" " * pad + y + b"\t" + c + b"\n"


def edge_text(kind, edge_every=BLOCK, n_edges=3):
    """a text in which, at every multiple of edge_every, a line ends exactly at the edge (its newline is the last byte before it),
    lies across it, or starts one byte behind it (the newline before it is the first byte behind the edge)"""
    at = {"ends": None, "across": 9, "behind": -1}[kind]
    buf, k = b"", 0
    for e in range(1, n_edges + 1):
        edge = e * edge_every
        while len(buf) < edge - 300:
            buf += _line(k)
            k += 1
        special = _line(k + 1)
        start = edge - len(special) if at is None else edge - at       # where the special line starts
        buf += _line(k, start - len(buf)) + special
        k += 2
        assert buf.endswith(special) and len(buf) - len(special) == start
    return buf + _line(k) * 3


EDGE_KINDS = ["ends", "across", "behind"]


@pytest.mark.parametrize("res", [None, 5000])
@pytest.mark.parametrize("kind", EDGE_KINDS)
def test_bytes_equal_the_model_at_block_edges(kind, res, tmp_path):
    data = edge_text(kind)
    where = {"ends": data[BLOCK - 1:BLOCK] == b"\n", "across": b"\n" not in data[BLOCK - 9:BLOCK + 1], "behind": data[BLOCK:BLOCK + 1] == b"\n"}
    assert where[kind]
    assert gpu_bytes(data, res, tmp_path) == model_bytes(data, res)


@pytest.mark.parametrize("res", [None, 5000])
@pytest.mark.parametrize("kind", EDGE_KINDS)
def test_bytes_equal_the_model_when_batch_edges_fall_inside_the_file(kind, res, tmp_path):
    data = edge_text(kind, 8192, 5)                                    # "ends": the first batch is full to its last byte
    assert len(data) > 5 * 8192 and (kind != "ends" or data[8191:8192] == b"\n")
    assert gpu_bytes(data, res, tmp_path, 8192) == model_bytes(data, res)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 511])
def test_bytes_equal_the_model_round_the_rounds_of_256_lines(n, tmp_path):
    data = b"".join(_line(k) for k in range(n))
    assert len(data) < BLOCK                                           # one block: its lines take n / 256 rounds
    for res in (None, 5000):
        assert gpu_bytes(data, res, tmp_path) == model_bytes(data, res)
    assert gpu_bytes(data[:-1], 5000, tmp_path) == model_bytes(data, 5000)      # a last line without a newline gets one


def test_a_block_of_empty_lines_between_two_63_byte_names_gives_131_times_the_input(tmp_path):
    data, a, b = b"\n" * BLOCK, "A" * 63, "b" * 63
    made = gpu_bytes(data, None, tmp_path, None, a, b)
    assert len(made) == 131 * BLOCK and made == model_bytes(data, None, a, b)
    two = b"\n" * (BLOCK + 700) + _line(3) + b"\n" * 300                # the same across a block edge, a batch edge and an odd line
    assert gpu_bytes(two, None, tmp_path, 8192, a, b) == model_bytes(two, None, a, b)


def test_a_4096_byte_line_beside_8_byte_lines(tmp_path):
    short = b"0\t0\t123\n"
    assert len(short) == 8 and len(_line(7, 4097)) == 4097
    data = short * 40 + _line(7, 4097) + short * 300 + _line(8, 4097) + short * 5
    for res in (None, 5000):
        for batch in (None, 8192):
            assert gpu_bytes(data, res, tmp_path, batch) == model_bytes(data, res)
    wide = short * 3 + b"x" * 4096 + b"\n" + b"y" * 2000 + b" " + b"z" * 2095 + b"\n" + short        # verbatim: one field of 4096 bytes
    assert gpu_bytes(wide, None, tmp_path) == model_bytes(wide, None)


def test_two_runs_give_the_same_bytes(tmp_path):
    data = edge_text("across") + run_input(RUNS["jma_r5000"])
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    for res in (None, 5000):
        assert gpu_bytes(data, res, tmp_path / "a") == gpu_bytes(data, res, tmp_path / "b", 8192)


def test_a_gzipped_dump(tmp_path):
    data = edge_text("behind")
    for res in (None, 5000):
        assert gpu_bytes(gzip.compress(data), res, tmp_path) == model_bytes(data, res)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------
def _refusal_of(data, res, tmp_path, batch=None):
    from fithic_amd import _capi
    src = str(tmp_path / "bad.txt")
    with open(src, "wb") as f:
        f.write(data)
    jc = _capi.JcContext(0)
    try:
        with batch_bytes("FHX_JC_BATCH_BYTES", batch), pytest.raises(_capi.JcRefused) as e:
            jc.convert_file(src, "chr1", "chrX", res or 0, keep_rows=bool(res))
        assert jc.counts() == dict(lines=0, rows=0, bytes=0) and jc.device_ptrs() == [0] * 5 and jc.text() == b""
        return e.value.why, e.value.line
    finally:
        jc.close()


@pytest.mark.parametrize("kind", sorted(BAD_BOTH) + sorted(BAD_MIDPOINT))
def test_a_bad_line_is_refused_with_its_line_number(kind, tmp_path):
    bad, why = (BAD_BOTH.get(kind) or BAD_MIDPOINT[kind])
    data = GOOD * 1300 + bad + b"\n" + GOOD * 50                      # line 1301 lies in the second 16 KB block
    assert len(GOOD) * 1300 > BLOCK
    for res in ([None, 5000] if kind in BAD_BOTH else [5000]):
        with pytest.raises(jm.Refused) as e:
            jm.records(data, res)
        assert (e.value.why, e.value.line) == (why, 1301)
        assert _refusal_of(data, res, tmp_path) == (why, 1301)
    if kind in BAD_MIDPOINT:                                          # verbatim mode copies the line
        assert gpu_bytes(data, None, tmp_path) == model_bytes(data, None)


def test_a_4097_byte_line_is_refused(tmp_path):
    data = GOOD * 5 + b"5000" + b" " * 4083 + b"10000\t3   \n" + GOOD
    assert len(data.split(b"\n")[5]) == 4097
    for res in (None, 5000):
        assert _refusal_of(data, res, tmp_path) == (jm.LONG_LINE, 6)
    fits = data.replace(b"3   \n", b"3  \n")                           # 4096 bytes are a line
    assert gpu_bytes(fits, 5000, tmp_path) == model_bytes(fits, 5000)


def test_the_smaller_of_two_bad_lines_is_reported_and_line_numbers_run_across_batches(tmp_path):
    data = GOOD * 1000 + b"5000 10000\n" + GOOD * 700 + b"5000 10001 3\n" + GOOD * 10
    assert _refusal_of(data, 5000, tmp_path) == (jm.TOKENS, 1001)
    assert _refusal_of(data, 5000, tmp_path, 8192) == (jm.TOKENS, 1001)                   # 8192 // 13 = 630 lines a batch: batch 2
    late = GOOD * 1701 + b"5000 10001 3\n" + GOOD * 10
    assert _refusal_of(late, 5000, tmp_path, 8192) == (jm.GRID, 1702)                    # batch 3
    assert _refusal_of(GOOD * 5 + b"5000\t10000\t3\r", None, tmp_path) == (jm.BYTES, 6)    # a \r that ends the text


def test_a_refusal_in_the_second_batch_leaves_nothing_written(tmp_path):
    from fithic_amd import juicer
    src = str(tmp_path / "dump.txt")
    with open(src, "wb") as f:
        f.write(GOOD * 900 + b"5000\t10000\t0.5\n" + GOOD * 3)
    for out, res in (("o.gz", None), ("o.txt", 5000), ("o.txt.gz", 5000)):
        dst = str(tmp_path / out)
        with batch_bytes("FHX_JC_BATCH_BYTES", 8192):
            if res is None:
                assert juicer.convert(src, "1", "1", dst) == 904
                os.remove(dst)
                continue
            with pytest.raises(ValueError, match=r"dump\.txt, line 901: .*raw \(`NONE`\) dump is expected.*0\.5"):
                juicer.convert(src, "1", "1", dst, res)
        assert not os.path.exists(dst)
    r = subprocess.run([sys.executable, "-m", "fithic_amd.juicer", "--dump", src, "--CHR1", "1", "--CHR2", "1", "--resolution", "5000", "--outFile",
                        str(tmp_path / "cli.txt")], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "line 901" in r.stderr and not os.path.exists(str(tmp_path / "cli.txt"))
    with pytest.raises(ValueError, match="line 901"):
        juicer.read([(src, "1", "1")], 5000)


def test_a_good_call_after_a_refused_one_gives_the_model_s_bytes(tmp_path):
    from fithic_amd import _capi
    rows = [b"%d\t%d\t%d\n" % (5000 * (k % 97), 5000 * (k % 89 + 100), 1 + k % 50) for k in range(1500)]
    good, bad = b"".join(rows), b"".join(rows[:1300]) + b"5000 10000\n" + b"".join(rows[1300:])
    assert 2 * 8192 < len(b"".join(rows[:1300])) and len(bad) < 4 * 8192     # line 1301 lies in the third batch at the earliest
    for name, data in (("bad.txt", bad), ("good.txt", good)):
        with open(str(tmp_path / name), "wb") as f:
            f.write(data)
    jc = _capi.JcContext(0)
    try:
        with batch_bytes("FHX_JC_BATCH_BYTES", 8192):
            with pytest.raises(_capi.JcRefused) as e:
                jc.convert_file(str(tmp_path / "bad.txt"), "chr1", "chrX", 5000, keep_rows=True)
            assert (e.value.why, e.value.line) == (jm.TOKENS, 1301)
            assert jc.counts() == dict(lines=0, rows=0, bytes=0) and jc.device_ptrs() == [0] * 5 and jc.text() == b""
            assert jc.convert_file(str(tmp_path / "good.txt"), "chr1", "chrX", 5000, keep_rows=True) == 1500
        want = model_bytes(good, 5000, "1", "X")                      # the .py writes `chr` before a name; the handle takes it whole
        assert jc.text() == want and jc.counts() == dict(lines=1500, rows=1500, bytes=len(want))
    finally:
        jc.close()


# ---- 4. the direct path -----------------------------------------------------------------------------------------------------------
def _one_pass(load):
    from fithic_amd import tables
    from fithic_amd.engine import Engine
    eng = Engine(0)
    try:
        eng.configure(10000, 20000, 2000000, 20, 1, "intraOnly")
        load(eng, tables.ChromIndex())
        eng.run_pass()
        v = eng.fetch()
        return v["p"].copy(), v["q"].copy()
    finally:
        eng.close()


def _synthetic_map(tmp_path):
    """dumps 1-1, 1-2 and 2-2 of a map of two chromosomes of 300 bins of 10 kb: every cell once, the upper triangle"""
    rng = np.random.default_rng(17)
    dumps = []
    for a, b, n in (("1", "1", 9000), ("1", "2", 2500), ("2", "2", 8000)):
        cells = rng.choice(300 * 300, 4 * n, replace=False)
        x, y = cells // 300, cells % 300
        keep = (x <= y) if a == b else np.ones(len(x), bool)
        x, y = x[keep][:n], y[keep][:n]
        count = np.maximum(1, (rng.pareto(1.1, len(x)) * 40 / (1 + np.abs(y - x))).astype(np.int64)) % 100000
        text = b"".join(b"%d\t%d\t%d%s\n" % (p * 10000, q * 10000, c, b".0" if c % 3 == 0 else b"") for p, q, c in zip(x, y, count))
        path = str(tmp_path / ("dump_%s_%s.txt" % (a, b)))
        with open(path, "wb") as f:
            f.write(text)
        dumps.append((path, a, b, text))
    return dumps


def test_read_feeds_an_engine_the_rows_of_the_written_file(tmp_path):
    from fithic_amd import fragments, juicer, tables
    dumps = _synthetic_map(tmp_path)
    sizes, con_path = str(tmp_path / "chrom.sizes"), str(tmp_path / "contacts.gz")
    with open(sizes, "w") as f:
        f.write("chr1\t3000000\nchr2\t3000000\n")
    names, *cols = jm.columns([(text, a.encode(), b.encode()) for _, a, b, text in dumps], 10000)
    with batch_bytes("FHX_JC_BATCH_BYTES", 32768), juicer.read([(p, a, b) for p, a, b, _ in dumps], 10000) as data:      # every dump takes several batches
        assert data.names == names == ["chr1", "chr2"] and len(data) == len(cols[0]) > 15000
        for g, w in zip(data.contacts(), cols):
            assert g.dtype == np.int32 and np.array_equal(g, np.asarray(w, np.int32))
        assert data.text() == b"".join(jm.convert(text, a.encode(), b.encode(), 10000) for _, a, b, text in dumps)
        assert set(data.stage_seconds()) == {"read_upload", "newline_scan", "parse", "format", "copy_out"}
        data.write(con_path)
    assert _gunzip(con_path).count(b"\n") == len(cols[0])

    def from_file(eng, chroms):
        con = tables.read_contacts(con_path, chroms)
        eng.load_fragments(*fragments.bins(sizes, 10000, chroms), chroms.sort_rank())
        eng.load_contacts(con.chr1, con.mid1, con.chr2, con.mid2, con.count)

    def direct(eng, chroms):
        with juicer.read([(p, a, b) for p, a, b, _ in dumps], 10000, keep_text=False) as data:     # the rows alone
            assert data.text() == b"" and len(data) == len(cols[0])
            data.intern(chroms)
            eng.load_fragments(*fragments.bins(sizes, 10000, chroms), chroms.sort_rank())
            data.load_into(eng, chroms)

    (wp, wq), (gp, gq) = _one_pass(from_file), _one_pass(direct)
    assert len(wp) == len(cols[0]) and np.isfinite(wp).any()
    assert bits_equal(gp, wp) and bits_equal(gq, wq)
