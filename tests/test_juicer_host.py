"""CPU tests of the Juicer dump path: the plain-Python model (tests/juicer_model.py) equals the real reference's output on the
fixtures of tests/golden/juicer (made by tests/golden/make_golden_juicer.py) and the installed mawk, running the script's own awk
program, on random lines from an adversarial token pool; it refuses each reason with the right line; and the Python surface
refuses names and resolutions outside the documented set before any file is opened."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import juicer_model as jm
from conftest import GOLDEN

JC = os.path.join(GOLDEN, "juicer")
with open(os.path.join(JC, "cases.json")) as _f:
    CASES = json.load(_f)
RUNS = {r["name"]: r for r in CASES["runs"]}
AWK_PROGRAM = '{ printf "%s\\t%s\\t%s\\t%s\\t%s\\n", chr1,$1,chr2,$2,$3}'           # createFitHiCContacts-hic_old.sh:6


def _gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def run_input(run):
    return _gunzip(os.path.join(JC, run["input"]))


def run_output(run):
    return _gunzip(os.path.join(JC, run["output"]))


def model_bytes(run, data=None):
    return jm.convert(run_input(run) if data is None else data, run["chr1"].encode(), run["chr2"].encode(), run["resolution"])


def test_fixtures_were_made_by_the_pinned_tools_and_cover_the_cases_of_the_issue():
    assert CASES["awk"].startswith("mawk 1.3.4") and CASES["locale"] == "LC_ALL=C"
    q = run_input(RUNS["jvq_01_1e3"])
    assert q == run_input(RUNS["jvq_chrX"])
    lines = q.split(b"\n")
    assert b"" in lines[:-1] and any(line.startswith((b" ", b"\t")) for line in lines) and b"12.50" in q
    assert {min(len(line.split()), 4) for line in lines[:-1]} == {0, 1, 2, 3, 4} and b" \t" in q and b"  " in q
    assert (RUNS["jvq_01_1e3"]["chr1"], RUNS["jvq_01_1e3"]["chr2"], RUNS["jvq_chrX"]["chr1"]) == ("01", "1e3", "chrX")
    out = run_output(RUNS["jvq_01_1e3"])
    assert out.count(b"\n") == len(lines) - 1 and b"01\t5000\t1e3\t10000\t12.50\n" in out and b"01\t\t1e3\t\t\n" in out
    assert not run_input(RUNS["jvn"]).endswith(b"\n") and run_output(RUNS["jvn"]).endswith(b"\n")
    assert run_input(RUNS["jve"]) == b"" and run_output(RUNS["jve"]) == b""
    assert RUNS["jmx_r5000"]["chr1"] != RUNS["jmx_r5000"]["chr2"] and RUNS["jmo_r10001"]["resolution"] % 2 == 1
    x = run_output(RUNS["jmx_r5000"])
    assert b"chr1\t2500\tchrX\t2500\t1.0\n" in x and b"\t0.0\n" in x and b"\t16777216.0\n" in x and x.count(b"\t17.0\n") == 3
    assert b"\t2147482500\t" in x and b"chr7\t1\tchr7\t2147483647\t3.0\n" in run_output(RUNS["jmr_r2"])


@pytest.mark.parametrize("name", sorted(RUNS))
def test_model_equals_the_reference_on_the_fixtures(name):
    assert model_bytes(RUNS[name]) == run_output(RUNS[name])


def test_int_of_half_an_odd_resolution_rounds_down():
    assert jm.convert(b"10001\t20002\t1\n", b"1", b"2", 10001) == b"chr1\t15001\tchr2\t25002\t1.0\n"
    assert jm.convert(b"0 3 2\n", b"1", b"1", 3) == b"chr1\t1\tchr1\t4\t2.0\n"
    assert jm.convert(b"0 1 2\n", b"1", b"1", 1) == b"chr1\t0\tchr1\t1\t2.0\n"
    assert b"chr2\t15001\tchrX\t" in run_output(RUNS["jmo_r10001"])                        # the reference: 10001 + int(10001 / 2)


# ---- the installed awk on random lines ------------------------------------------------------------------------------------------
POOL = [b"0", b"5000", b"12.50", b"1e3", b"-7", b"+0", b".5", b"0x1A", b"nan", b"inf", b"a", b"chr1", b"%s", b"%d", b"\\t", b"\\n", b"\\\\", b"$1",
        b"'", b'"', b"#", b"{}", b"~", b"!", b"0000", b"16777216", b"9" * 40, b"1.", b"..", b"-", b"&", b"*", b"a" * 300]
BLANKS = [b" ", b"\t", b"  ", b" \t", b"\t\t ", b"\t \t"]


def random_lines(seed, n=2000):
    rng = np.random.default_rng(seed)
    lines = []
    for _ in range(n):
        k = int(rng.integers(0, 6))
        line = BLANKS[int(rng.integers(0, len(BLANKS)))] if rng.random() < 0.2 else b""
        for j in range(k):
            line += POOL[int(rng.integers(0, len(POOL)))] + (BLANKS[int(rng.integers(0, len(BLANKS)))] if j + 1 < k or rng.random() < 0.2 else b"")
        lines.append(line)
    return b"\n".join(lines) + (b"\n" if seed % 2 else b"")


def _mawk():
    try:
        said = subprocess.run(["awk", "-W", "version"], capture_output=True, env=dict(os.environ, LC_ALL="C"), timeout=20).stdout.decode()
    except (OSError, subprocess.SubprocessError):
        return False
    return said.startswith("mawk 1.3.4")


@pytest.mark.skipif(not _mawk(), reason="the installed awk is not mawk 1.3.4")
@pytest.mark.parametrize("seed,chr1,chr2", [(1, "1", "1"), (2, "01", "1e3"), (3, "chrX", "chr_9.a-b")])
def test_model_equals_the_installed_awk_on_random_lines(seed, chr1, chr2, tmp_path):
    data = random_lines(seed)
    src = str(tmp_path / "dump.txt")
    with open(src, "wb") as f:
        f.write(data)
    script = subprocess.run(["awk", "-v", "chr1=" + chr1, "-v", "chr2=" + chr2, AWK_PROGRAM, src], env=dict(os.environ, LC_ALL="C"),
                            capture_output=True, check=True).stdout
    assert script.count(b"\n") == 2000
    assert jm.convert(data, chr1.encode(), chr2.encode()) == script


# ---- refusals -------------------------------------------------------------------------------------------------------------------
GOOD = b"5000\t10000\t3\n"
BAD_BOTH = {"NUL": (b"5000\t10000\t3\x00", jm.BYTES), "CR": (b"5000\t10000\t3\r", jm.BYTES), "form feed": (b"5000\f10000 3", jm.BYTES),
            "DEL": (b"5000 10000 3\x7f", jm.BYTES), "non-ASCII": (b"5000 10000 \xe9", jm.BYTES), "long line": (b"5000 10000 3" + b" " * 4085, jm.LONG_LINE)}
BAD_MIDPOINT = {"two tokens": (b"5000 10000", jm.TOKENS), "four tokens": (b"5000 10000 3 4", jm.TOKENS), "empty line": (b"", jm.TOKENS),
                "signed bin": (b"+5000 10000 3", jm.BIN), "11 digits": (b"5000 10000000000 3", jm.BIN), "bin with a point": (b"5000.0 10000 3", jm.BIN),
                "off the grid": (b"5000 10001 3", jm.GRID), "x off the grid": (b"1 10000 3", jm.GRID),
                "midpoint beyond int32": (b"5000 2147485000 3", jm.RANGE), "above 2^24": (b"5000 10000 16777217", jm.COUNT),
                "16 digits": (b"5000 10000 0000000000000001", jm.COUNT), "no number": (b"5000 10000 abc", jm.COUNT),
                "digits then text": (b"5000 10000 12x", jm.COUNT), "fraction": (b"5000 10000 12.50", jm.FRACTION),
                "exponent": (b"5000 10000 1e3", jm.FRACTION), "sign": (b"5000 10000 -3", jm.FRACTION), "nan": (b"5000 10000 NaN", jm.FRACTION),
                "inf": (b"5000 10000 -inf", jm.FRACTION), "point without zeros": (b"5000 10000 3.", jm.FRACTION),
                "bad bin and bad count": (b"5000 1x 1e3", jm.BIN), "off the grid and out of range": (b"5000 2147485001 3", jm.GRID)}


def test_the_pool_of_bad_lines_names_every_reason():
    seen = {why for _, why in list(BAD_BOTH.values()) + list(BAD_MIDPOINT.values())}
    assert seen == {jm.BYTES, jm.LONG_LINE, jm.TOKENS, jm.BIN, jm.GRID, jm.RANGE, jm.COUNT, jm.FRACTION}


@pytest.mark.parametrize("kind", sorted(BAD_BOTH) + sorted(BAD_MIDPOINT))
def test_model_refuses_a_bad_line_4_of_5_with_its_number(kind):
    bad, why = (BAD_BOTH.get(kind) or BAD_MIDPOINT[kind])
    data = GOOD * 3 + bad + b"\n" + GOOD
    for res in ([None, 5000] if kind in BAD_BOTH else [5000]):
        with pytest.raises(jm.Refused) as e:
            jm.records(data, res)
        assert (e.value.why, e.value.line) == (why, 4)
    if kind in BAD_MIDPOINT:
        assert jm.convert(data, b"1", b"1").count(b"\n") == 5                               # verbatim mode takes the line


def test_model_reports_the_smaller_of_two_bad_lines():
    data = GOOD + b"5000 10001 3\n" + GOOD + b"5000 10000\n" + GOOD
    with pytest.raises(jm.Refused) as e:
        jm.records(data, 5000)
    assert (e.value.why, e.value.line) == (jm.GRID, 2)
    with pytest.raises(jm.Refused) as e:
        jm.records(b"\n".join(reversed(data.split(b"\n")[:-1])), 5000)                     # no newline at the end: the last line counts
    assert (e.value.why, e.value.line) == (jm.TOKENS, 2)
    assert len(jm.records(b"5000 10000 3" + b" " * 4084 + b"\n", 5000)) == 1                # 4096 bytes are a line


@pytest.mark.parametrize("name", ["", "a b", "chr1\\t", "chr$1", "x" * 64, "chr/1", "ché", "a\n"])
def test_names_outside_the_set_are_a_value_error(name, tmp_path):
    from fithic_amd import juicer
    with pytest.raises(ValueError):
        jm.check_name(name.encode())
    missing = str(tmp_path / "absent.txt")                                                # never opened: the name is looked at first
    for args in ((missing, name, "1", str(tmp_path / "o.gz")), (missing, "1", name, str(tmp_path / "o.gz"), 5000)):
        with pytest.raises(ValueError, match="chromosome name"):
            juicer.convert(*args)
    with pytest.raises(ValueError, match="chromosome name"):
        juicer.read([(missing, "1", name)], 5000)
    assert not os.path.exists(str(tmp_path / "o.gz"))


def test_names_of_the_set_and_resolutions():
    from fithic_amd import juicer
    for name in ("1", "01", "1e3", "chrX", "a" * 63, "_.-"):
        assert juicer.check_name(name) == name and jm.check_name(name.encode())
    for res in (0, -1, 1 << 31, 5000.0, "5000", True):
        with pytest.raises(ValueError, match="resolution"):
            juicer.convert("absent.txt", "1", "1", "o.txt", res)
    assert juicer.check_resolution((1 << 31) - 1) and juicer.check_resolution(1)
