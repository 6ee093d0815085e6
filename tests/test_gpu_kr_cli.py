"""`fithic --kr` end to end: one command against the protocol's two steps (python -m fithic_amd.hickry, then fithic -t with its
file) - every output file, the log and the bias file equal - and against the REAL reference's two steps on the bundled hESC
chr1 set (tests/golden/kr_resident/, written by tests/golden/make_golden_kr_resident.py)."""
import contextlib
import gzip
import io
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
DATA = os.path.join(GOLDEN, "data")
FIXTURE = os.path.join(GOLDEN, "kr_resident")

# name -> (KR golden case, -x of HiCKRy as text, fithic arguments).  "hesc" is what make_golden_kr_resident.py ran the reference with
SETUPS = {
    "hesc": ("k1_kr_hESC", "0.12", ["-r", "40000", "-p", "2", "-x", "All"]),
    "irregular": ("k4_kr_irregular", "0.0", ["-r", "0", "-b", "15", "-p", "2", "-x", "All", "-L", "10000", "-U", "900000"]),
    "significant": ("k1_kr_hESC", "0.12", ["-r", "40000", "-p", "2", "-x", "All", "--significant", "0.05"]),
}


def _gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


class Pair:
    """run A (`fithic --kr`) and run B (hickry, then `fithic -t`) of one setup, each in a directory of its own with the same
    relative paths, so that the logs can be equal"""

    def __init__(self, base, setup):
        from fithic_amd import cli, hickry
        case, perc, args = SETUPS[setup]
        with open(os.path.join(GOLDEN, case + ".json")) as f:
            self.meta = json.load(f)
        con, frg = os.path.join(DATA, self.meta["contacts"]), os.path.join(DATA, self.meta["frags"])
        common = ["-i", con, "-f", frg, "-o", "out", "-l", "kr"] + args
        self.a, self.b = base / "a", base / "b"
        self.a.mkdir()
        self.b.mkdir()
        cwd, argv = os.getcwd(), sys.argv
        out_a, out_b = io.StringIO(), io.StringIO()
        try:
            os.chdir(str(self.a))
            with contextlib.redirect_stdout(out_a):
                cli.main(common + ["--kr", "--kr-percent", perc, "--kr-output", "bias.gz"])
            os.chdir(str(self.b))
            sys.argv = ["HiCKRy.py", "-i", con, "-f", frg, "-o", "bias.gz", "-x", perc]
            with contextlib.redirect_stdout(out_b):
                hickry.main()
                cli.main(common + ["-t", "bias.gz"])
        finally:
            sys.argv = argv
            os.chdir(cwd)
        self.stdout_a, self.stdout_b = out_a.getvalue(), out_b.getvalue()


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    cache = {}

    def get(setup):
        if setup not in cache:
            cache[setup] = Pair(tmp_path_factory.mktemp(setup), setup)
        return cache[setup]
    return get


# ---- 7. the resident run against the two-step run --------------------------------------------------------------------------------
@pytest.mark.parametrize("setup", sorted(SETUPS))
def test_one_command_equals_the_two_steps(setup, pairs):
    P = pairs(setup)
    files = sorted(os.listdir(str(P.a / "out")))
    assert files == sorted(os.listdir(str(P.b / "out")))
    res = SETUPS[setup][2][1]
    tag = "" if res == "0" else ".res" + res
    expected = ["kr.fithic.log"] + ["kr.fithic_pass%d%s.txt" % (k, tag) for k in (1, 2)] + \
               ["kr.spline_pass%d%s.significances.txt.gz" % (k, tag) for k in (1, 2)]
    if setup == "significant":
        expected += ["kr.spline_pass2%s.fdr_subset.txt.gz" % tag, "kr.spline_pass2%s.merged.txt.gz" % tag]
    assert files == sorted(expected)
    for name in files:
        read = _gunzip if name.endswith(".gz") else (lambda p: open(p, "rb").read())
        a, b = read(str(P.a / "out" / name)), read(str(P.b / "out" / name))
        assert a == b, name
        assert len(a) > 100, name
    assert "Spline successfully fit" in (P.a / "out" / "kr.fithic.log").read_text()      # (the log of the last pass: each pass starts it anew)
    assert _gunzip(str(P.a / "bias.gz")) == _gunzip(str(P.b / "bias.gz"))
    assert _gunzip(str(P.a / "bias.gz")).count(b"\n") == P.meta["out_lines"]
    # HiCKRy's own lines, as the golden run of the reference printed them (its two clock lines aside)
    printed = "\n".join(ln for ln in P.stdout_a.splitlines() if "took" not in ln)
    assert P.meta["stdout"] in printed
    assert P.meta["stdout"] in "\n".join(ln for ln in P.stdout_b.splitlines() if "took" not in ln)
    routes = [ln for ln in P.stdout_a.splitlines() if ln.startswith("stage: Knight-Ruiz biases")]
    assert len(routes) == 1 and routes[0].endswith("(resident rows)")
    assert "Sparse matrix creation took" in P.stdout_a and "Fit-Hi-C completed successfully" in P.stdout_a
    if setup == "significant":
        assert _gunzip(str(P.a / "out" / ("kr.spline_pass2%s.fdr_subset.txt.gz" % tag))).count(b"\n") > 0


def test_bias_bounds_apply_to_the_computed_biases_and_the_log_has_the_bias_lines(tmp_path, monkeypatch):
    """-tL / -tU discard computed biases exactly as a file's: the pair of runs with narrow bounds on the irregular set, one pass, so
    that the log still holds what read_biases writes into it (every pass starts the log anew)"""
    from fithic_amd import cli, hickry
    case, perc, args = SETUPS["irregular"]
    with open(os.path.join(GOLDEN, case + ".json")) as f:
        meta = json.load(f)
    con, frg = os.path.join(DATA, meta["contacts"]), os.path.join(DATA, meta["frags"])
    common = ["-i", con, "-f", frg, "-l", "kr", "-tL", "0.8", "-tU", "1.25"] + [a if a != "2" else "1" for a in args]
    assert common.count("-p") == 1 and common[common.index("-p") + 1] == "1"
    monkeypatch.setattr("sys.argv", ["HiCKRy.py", "-i", con, "-f", frg, "-o", str(tmp_path / "bias.gz"), "-x", perc])
    hickry.main()
    cli.main(common + ["-o", str(tmp_path / "b"), "-t", str(tmp_path / "bias.gz")])
    cli.main(common + ["-o", str(tmp_path / "a"), "--kr", "--kr-percent", perc])
    a = _gunzip(str(tmp_path / "a" / "kr.spline_pass1.significances.txt.gz"))
    assert a == _gunzip(str(tmp_path / "b" / "kr.spline_pass1.significances.txt.gz"))
    assert b"\t-1.000000e+00\t" in a                   # some bias was discarded
    log = (tmp_path / "a" / "kr.fithic.log").read_text()
    assert log == (tmp_path / "b" / "kr.fithic.log").read_text().replace(str(tmp_path / "b"), str(tmp_path / "a"))
    for k in ("5th", "50th", "95th"):
        assert sum(ln.startswith(k + " quantile of biases: ") for ln in log.splitlines()) == 1
    line = [ln for ln in log.splitlines() if "were discarded" in ln][0]
    assert line.startswith("Out of %d loci " % meta["n"]) and line.endswith("[0.8-1.25]") and int(line.split()[4]) > 0


# ---- 8. against the real reference ---------------------------------------------------------------------------------------------------
def _one_unit_apart(a, b):
    """two printed numbers (%e or %f) that differ by one unit of the last printed digit (9.999999e-01 and 1.000000e+00 do)"""
    from decimal import Decimal
    da, db = Decimal(a), Decimal(b)
    return abs(da - db) == Decimal(1).scaleb(min(da.as_tuple().exponent, db.as_tuple().exponent))


def test_against_the_reference_two_steps(pairs):
    """HiCKRy.py -x 0.12, then fithic.py -t on the hESC chr1 set: every 61st row of the reference's pass-1 significances file.

    In this order: the identity columns and the counts are equal; p and q, as printed, are within the project's 1e-10; the printed
    bias1, bias2 and ExpCC columns are equal as text or one unit off in the last printed digit.  The last allowance follows from a
    derivation: the GPU's bias differs from the reference's by <= 1e-12 relative (HiCKRy's ddot order belongs to its BLAS build),
    which can only move a rounding boundary.  The number of rows whose text differs is printed, not bounded."""
    with open(os.path.join(FIXTURE, "cases.json")) as f:
        cases = json.load(f)
    case, perc, args = SETUPS["hesc"]
    assert (perc, args) == (cases["perc"], ["-r", str(cases["res"]), "-p", str(cases["passes"]), "-x", cases["mode"]])
    P = pairs("hesc")
    want_bias = np.load(os.path.join(FIXTURE, "bias.npy"))
    got_bias = np.array([float(ln.split(b"\t")[2]) for ln in _gunzip(str(P.a / "bias.gz")).splitlines()])
    assert len(got_bias) == len(want_bias) == cases["bias_lines"]
    assert np.array_equal(got_bias == -1.0, want_bias == -1.0) and int((want_bias == -1.0).sum()) == cases["bias_removed"]
    ok = want_bias != -1.0
    rel = float(np.max(np.abs(got_bias[ok] - want_bias[ok]) / np.abs(want_bias[ok])))
    print("bias vector: largest relative difference to the reference's %.3g" % rel)
    assert rel <= 1e-12
    lines = _gunzip(str(P.a / "out" / ("kr.spline_pass1.res%d.significances.txt.gz" % cases["res"]))).decode().splitlines()
    assert lines[0].split("\t") == cases["header"] and len(lines) - 1 == cases["rows"]
    rows = [ln.split("\t") for ln in lines[1::cases["stride"]]]
    g = np.load(os.path.join(FIXTURE, "pass1_columns.npz"))
    text = _gunzip(os.path.join(FIXTURE, "pass1_text.txt.gz")).decode().splitlines()
    assert len(rows) == len(text) == cases["stored_rows"] == len(g["p"])
    assert {w[0] for w in rows} == set(cases["chr1"]) and {w[2] for w in rows} == set(cases["chr2"])
    for key, col in (("mid1", 1), ("mid2", 3), ("count", 4)):
        assert np.array_equal(np.array([int(w[col]) for w in rows]), g[key]), key
    for key, col in (("p", 5), ("q", 6)):
        got = np.array([float(w[col]) for w in rows])
        assert np.array_equal(np.isnan(got), np.isnan(g[key])), key
        d = float(np.nanmax(np.abs(got - g[key])))
        print("%s as printed: largest difference to the reference's %.3g" % (key, d))
        assert d <= 1e-10, (key, d)
    differing = 0
    for w, ref_line in zip(rows, text):
        ref = ref_line.split("\t")
        if w[7:10] != ref:
            differing += 1
            for a, b in zip(w[7:10], ref):
                assert a == b or _one_unit_apart(a, b), (w, ref)
    print("rows whose printed bias1 / bias2 / ExpCC differ from the reference's: %d of %d" % (differing, len(rows)))
