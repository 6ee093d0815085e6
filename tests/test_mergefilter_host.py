"""CPU tests of the merge-filter path: the plain-Python model (tests/mergefilter_model.py) equals the real script's subset on the
fixtures of tests/golden/mergefilter (made by tests/golden/make_golden_mergefilter.py) and the installed mawk on random lines
round the class boundaries, the host's key bisection equals brute force round its bound, and the Python surface refuses what
the module documents."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import mergefilter_model as mm
from conftest import GOLDEN

MF = os.path.join(GOLDEN, "mergefilter")
with open(os.path.join(MF, "cases.json")) as _f:
    CASES = json.load(_f)
RUNS = {r["name"]: r for r in CASES["runs"]}
THRESHOLDS = ["0", "1e-300", "1e-5", "0.05", ".1", "1e-1", "0.30", "1", "5"]


def _gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def run_input(run):
    return _gunzip(os.path.join(MF, run["input"]))


def test_fixtures_were_made_by_the_pinned_tools_and_cover_the_cases_of_the_issue():
    assert CASES["awk"].startswith("mawk 1.3.4") and CASES["locale"] == "LC_ALL=C"
    a, q, n = (run_input(RUNS[k]) for k in ("mfa", "mfq_5", "mfn"))
    assert a.startswith(b"chr1\tfragmentMid1") and len(set(line.split()[0] for line in a.splitlines()[1:])) == 3
    assert all(len(line.split()) == 10 for line in a.splitlines()) and b"  " in a and b" \t" in a
    for needle in (b"5.000000e-02", b"4.999999e-02", b"5.000001e-02", b"0.000000e+00", b"e-112"):
        assert needle in a
    sub = _gunzip(os.path.join(MF, RUNS["mfa"]["subset"]))
    assert b"5.000000e-02" in sub and b"4.999999e-02" in sub and b"5.000001e-02" not in sub and b"0.000000e+00" in sub
    assert RUNS["mfq_5"]["input"] == RUNS["mfq_1e-5"]["input"] and (RUNS["mfq_1e-5"]["fdr"], RUNS["mfq_5"]["fdr"]) == ("1e-5", "5")
    for needle in (b"1.000000e-320", b"2.225074e-308", b"2.225073e-308"):
        assert needle in q
    first = q.splitlines()[0]
    assert mm.classify(first.split()[6]) == "numeric" and float(first.split()[6]) <= 1e-5          # a data row on line 1 ...
    lo, hi = (_gunzip(os.path.join(MF, RUNS[k]["subset"])) for k in ("mfq_1e-5", "mfq_5"))
    assert first not in lo.splitlines() and first not in hi.splitlines()                          # ... is lost
    # mawk itself: the subnormal is kept at both thresholds ("1." < "1e", '1' < '5'), 2.225073e-308 only at 5, 2.225074e-308 at both
    assert b"1.000000e-320" in lo and b"1.000000e-320" in hi and b"2.225074e-308" in lo and b"2.225074e-308" in hi
    assert b"2.225073e-308" not in lo and b"2.225073e-308" in hi and b"9.000000e-315" not in hi
    assert not n.endswith(b"\n") and _gunzip(os.path.join(MF, RUNS["mfn"]["subset"])).endswith(n.splitlines()[-1] + b"\n")
    assert all(len(run_input(r).splitlines()) <= 400 for r in RUNS.values())
    # no row passes: the script leaves an empty subset and a merged file that holds only the header line
    assert _gunzip(os.path.join(MF, RUNS["mfe"]["subset"])) == b""
    assert _gunzip(os.path.join(MF, RUNS["mfe"]["merged"])) == b"chr1\tmid1\tchr2\tmid2\tCC\tp\tfdr\tbin1_low\tbin1_high\tbin2_low\tbin2_high\tsumCC\tStrongConn"


@pytest.mark.parametrize("name", sorted(RUNS))
def test_model_reproduces_the_script_s_subset(name):
    run = RUNS[name]
    assert mm.select(run_input(run), run["fdr"]) == _gunzip(os.path.join(MF, run["subset"]))


# ---- the installed awk ------------------------------------------------------------------------------------------------------
BOUNDARY_FIELDS = ["0.000000e+00", "0.000000e-00", "0.000000e+999", "0.000000e-05", "2.225074e-308", "2.225073e-308", "2.225075e-308",
                   "1.000000e-308", "9.999999e-309", "1.000000e-320", "4.940656e-324", "9.000000e-315", "1.000000e-400", "5.000000e-324",
                   "9.999999e+307", "1.000000e+307", "1.000000e+309", "9.999999e+309", "5.000000e+400", "1.000000e+999", "4.999999e+999",
                   "1.000000e+00", "9.999999e-01", "1.000001e+00", "5.000000e+00", "5.000001e+00", "4.999999e+00", "5.000000e-02",
                   "4.999999e-02", "5.000001e-02", "1.000000e-01", "9.999999e-02", "1.000001e-01", "3.000000e-01", "2.999999e-01",
                   "3.000001e-01", "1.000000e-05", "9.999999e-06", "1.000001e-05", "1.000000e-300", "9.999999e-301", "1.000001e-300",
                   "1.000000e-005", "1.000000e+000", "3.000000e-001"]


def random_lines(seed, n=2000):
    rng = np.random.default_rng(seed)
    fields = list(BOUNDARY_FIELDS)
    while len(fields) < n:
        kind = rng.integers(0, 4)
        digits = "%d.%06d" % (rng.integers(1, 10), rng.integers(0, 1000000))
        if kind == 0:
            ex = int(rng.integers(-12, 2))
        elif kind == 1:
            ex = int(rng.integers(-330, -300))
        elif kind == 2:
            ex = int(rng.choice([-400, -309, -308, -307, 306, 307, 309, 310, 400]))
        else:
            ex = int(rng.integers(-307, 308))
        fields.append("%se%s%02d" % (digits, "-" if ex < 0 else "+", abs(ex)))
    order = rng.permutation(len(fields))
    seps = ["\t", " ", "  ", " \t"]
    return b"".join(seps[k % 4].join(["chr1", "%d" % (5000 * k + 2500), "chr1", "%d" % (5000 * k + 52500), "9", "1.000000e-09", fields[i], "x"]).encode()
                    + b"\n" for k, i in enumerate(order))


def _mawk():
    try:
        said = subprocess.run(["awk", "-W", "version"], capture_output=True, env=dict(os.environ, LC_ALL="C"), timeout=20).stdout.decode()
    except (OSError, subprocess.SubprocessError):
        return False
    return said.startswith("mawk 1.3.4")


@pytest.mark.skipif(not _mawk(), reason="the installed awk is not mawk 1.3.4")
@pytest.mark.parametrize("fdr", THRESHOLDS)
def test_model_equals_the_installed_awk_on_random_lines(fdr, tmp_path):
    data = random_lines(THRESHOLDS.index(fdr))
    classes = set(mm.classify(line.split()[6]) for line in data.splitlines())
    assert classes == {"zero", "numeric", "string"}
    src = str(tmp_path / "lines.txt")
    with open(src, "wb") as f:
        f.write(data)
    env = dict(os.environ, LC_ALL="C")
    script = subprocess.run("cat %s | awk '{if(NR!=1){print $0}}' | awk -v q=\"%s\" '{if($7<=q){print $0}}'" % (src, fdr), shell=True, env=env,
                            capture_output=True, check=True).stdout
    assert mm.select(data, fdr) == script and (fdr == "0" or 0 < script.count(b"\n") < data.count(b"\n") - 1)
    strict = subprocess.run(["awk", "-v", "q=" + fdr, "{if($7<q){print $0}}", src], env=env, capture_output=True, check=True).stdout
    assert mm.select(data, fdr, strict=True, skip_first_line=False) == strict
    assert strict != script


# ---- the host's bisection ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("fdr", THRESHOLDS)
def test_key_bound_equals_brute_force_round_the_bound(fdr, strict):
    from fithic_amd import mergefilter as mf
    bound = mf.key_bound(fdr, strict)
    q = float(fdr)
    passes = lambda text: float(text) < q if strict else float(text) <= q
    if bound == 0:
        assert not passes(mf._field(mf._LOWEST)) and q < 2.3e-308
        return
    e, m = divmod(bound, 10000000)
    at = e * mf._MANTISSAS + m - 1000000
    assert mf.key_of(at) == bound
    for i in range(max(mf._LOWEST, at - 3000), min(mf._HIGHEST, at + 3000) + 1):
        text = mf._field(i)
        assert passes(text) == (mf.key_of(i) <= bound), text
        assert mm.classify(text.encode()) == "numeric" and mm.keeps(text.encode(), fdr.encode(), strict) == passes(text)
    # the ends of the numeric class, and what the bound says about fdr itself
    assert mf._field(mf._LOWEST) == "2.225074e-308" and mf._field(mf._HIGHEST) == "9.999999e+307"
    assert mf.key_of(mf._LOWEST) == 2225074 and mf.key_of(mf._HIGHEST) == 615 * 10000000 + 9999999
    assert float(mf._field(at)) <= q and (at == mf._HIGHEST or float(mf._field(at + 1)) >= q)


def test_key_bounds_of_the_thresholds_of_the_issue():
    from fithic_amd import mergefilter as mf
    key = lambda text: (int(text[9:]) + 308) * 10000000 + int(text[0] + text[2:8])
    assert mf.key_bound("0.05") == key("5.000000e-02") and mf.key_bound("0.05", True) == key("4.999999e-02")
    assert mf.key_bound(".1") == mf.key_bound("1e-1") == key("1.000000e-01") and mf.key_bound("5") == key("5.000000e+00")
    assert mf.key_bound("0") == 0 and mf.key_bound("1e-300", True) == key("9.999999e-301")
    assert mf.key_bound("0.0500000001") == key("5.000000e-02") == mf.key_bound("0.0500000001", True)


# ---- the Python surface -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fdr", ["", "-0.05", "+1", "nan", "inf", "0x10", "5.", "1e", "1E-5", "1e-5 ", " 1", "1e-320", "4e-324", "1e999", "0." + "0" * 31, "٥"])
def test_fdr_outside_the_grammar_is_refused(fdr, tmp_path):
    from fithic_amd import mergefilter as mf
    with pytest.raises(ValueError):
        mf.fdr_text(fdr)
    with pytest.raises(mm.Refused) as e:
        mm.check_fdr(fdr)
    assert e.value.why == mm.FDR
    path = str(tmp_path / "sig.txt")
    open(path, "w").close()
    with pytest.raises(ValueError):
        mf.select(path, fdr, device=1 << 20)                          # refused before a device is asked for


def test_fdr_inside_the_grammar_is_taken():
    from fithic_amd import mergefilter as mf
    for fdr in THRESHOLDS + ["0.0", "0e5", "00.5", "2.2250738585072014e-308", "1e308", "1" * 32]:
        assert mf.fdr_text(fdr) == fdr.encode() == mm.check_fdr(fdr)


def test_entry_points_raise_without_a_usable_device(tmp_path):
    from fithic_amd import _capi, mergefilter as mf
    path = str(tmp_path / "sig.txt")
    open(path, "w").close()
    with pytest.raises(_capi.FhxError):
        mf.select(path, "0.05", device=1 << 20)
    with pytest.raises(SystemExit):
        mf.main(["sig.txt", "5000", "out.gz"])
    assert not os.path.exists("out.gz")


def test_refusals_become_the_documented_exceptions(tmp_path):
    from fithic_amd import _capi, mergefilter as mf
    path = str(tmp_path / "sig.txt")
    with open(path, "wb") as f:
        f.write(b"header\nchr1 1 chr1 2 3 1e-3 -1.000000e-02\nchr1 1 chr1\n")
    e = mf._refusal(path, _capi.MsRefused(-4, "x", _capi.MS_FIELD, 2))
    assert isinstance(e, ValueError) and "line 2" in str(e) and "-1.000000e-02" in str(e) and "The reference accepts this" in str(e)
    e = mf._refusal(path, _capi.MsRefused(-4, "x", _capi.MS_TOKENS, 3))
    assert "line 3" in str(e) and "3 token(s)" in str(e) and "The reference accepts this" in str(e)
    for why in (_capi.MS_BYTES, _capi.MS_LONG_LINE):
        e = mf._refusal(path, _capi.MsRefused(-4, "x", why, 1))
        assert isinstance(e, ValueError) and "line 1" in str(e)


def test_chromosome_passes_follow_cut_sort_uniq(tmp_path):
    """Combine under -H 0 lists `cut -f1 | sort -k1,1 | uniq`: a line without a tab counts whole"""
    from fithic_amd import mergefilter as mf
    text = b"chr2\t1\tx\nchr10 5 y\nchr2\t7\tz\nchr10 5 y\nchr10 4 y\nchr2 9\tw\n"
    src = str(tmp_path / "s.txt")
    with open(src, "wb") as f:
        f.write(text)
    want = subprocess.run("cut -f1 %s | sort -k1,1 | uniq" % src, shell=True, env=dict(os.environ, LC_ALL="C"), capture_output=True, check=True).stdout
    got = mf.Selection(text, 6, 6, {}, 0).chromosome_passes()
    assert got == [line.split()[0].decode() for line in want.splitlines()] == ["chr10", "chr10", "chr2", "chr2"]
    for name in sorted(RUNS):                                         # and on the goldens: every merged row is there once per pass
        sub, merged = (_gunzip(os.path.join(MF, RUNS[name][k])) for k in ("subset", "merged"))
        passes = mf.Selection(sub, 0, sub.count(b"\n"), {}, 0).chromosome_passes()
        rows = merged.split(b"\n")[1:]
        for chrom in set(passes):
            mine = [r for r in rows if r.split(b"\t")[0] == chrom.encode()]
            assert len(mine) % passes.count(chrom) == 0 and len(set(mine)) * passes.count(chrom) == len(mine)
