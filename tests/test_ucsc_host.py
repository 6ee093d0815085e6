"""CPU tests of the interact-track path: the plain-Python model (tests/ucsc_model.py) equals the real script's file on the
fixtures of tests/golden/ucsc (made by tests/golden/make_golden_ucsc.py) and the installed mawk on random lines and on the
fields whose score lies next to an integer or a %.6g boundary; the library's host routes for the score (the deferred one, and
the kernel's certification run on the host) equal the model; the Python surface refuses what the module documents."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import ucsc_model as um
from conftest import GOLDEN
from test_mergefilter_host import _mawk

UC = os.path.join(GOLDEN, "ucsc")
with open(os.path.join(UC, "cases.json")) as _f:
    CASES = json.load(_f)
RUNS = {r["name"]: r for r in CASES["runs"]}
AWK = ('{print $1, ($2-1), ($4+1), NR, int(-log($7)/log(10)), -log($7)/log(10), "EXP", "0", $1, ($2-1), ($2+1), "SOURCE_NAME", ".", $3, '
       '($4-1), ($4+1), "TARGET_NAME", "+"}')


def _gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def run_input(run):
    return _gunzip(os.path.join(UC, run["input"]))


def run_track(run):
    return _gunzip(os.path.join(UC, run["track"]))


def line_of(track, field_text, data):
    """the track line of the first input row whose field 7 is field_text"""
    kept = [row for row in data.splitlines() if row.split()[6][:1].isdigit()]
    want = [row for row in kept if row.split()[6] == field_text][0].split()
    for line in track.splitlines()[2:]:
        t = line.split()
        if (t[0], int(t[1]) + 1, t[13], int(t[15]) - 1) == (want[0], int(want[1]), want[2], int(want[3])):
            return t
    return None


def test_fixtures_were_made_by_the_pinned_tools_and_cover_the_cases_of_the_issue():
    assert CASES["awk"].startswith("mawk 1.3.4") and CASES["locale"] == "LC_ALL=C"
    a, q, n, e = (run_input(RUNS[k]) for k in ("uca", "ucq_5", "ucn", "uce"))
    assert a.startswith(b"chr1\tfragmentMid1") and a.splitlines()[0].split()[6] == b"q-value" and b" " not in a
    rows = [line.split() for line in a.splitlines()[1:]]
    assert len(set(r[0] for r in rows)) == 3 and any(r[0] != r[2] for r in rows)
    for needle in (b"5.000000e-02", b"4.999999e-02", b"5.000001e-02"):
        assert needle in a
    ta = run_track(RUNS["uca"])
    assert ta.startswith(um.HEAD) and b"  chromStart  " in um.HEAD and ta.count(b"\n") == 2 + 67
    assert line_of(ta, b"4.999999e-02", a) and not line_of(ta, b"5.000000e-02", a) and not line_of(ta, b"5.000001e-02", a)       # strict
    assert [t[3] for t in map(bytes.split, ta.splitlines()[2:])] == [b"%d" % k for k in range(1, 68)]
    assert line_of(ta, b"1.000000e-03", a)[4:6] == [b"2", b"3"]
    assert (RUNS["ucq_1e-5"]["input"], RUNS["ucq_1e-5"]["qval"], RUNS["ucq_5"]["qval"]) == (RUNS["ucq_5"]["input"], "1e-5", "5")
    lo, hi = run_track(RUNS["ucq_1e-5"]), run_track(RUNS["ucq_5"])
    for k in range(1, 308):
        assert (b"1.000000e-%02d" % k) in q
    powers = [line_of(hi, b"1.000000e-%02d" % k, q)[4:6] for k in range(1, 308)]
    assert all(g == b"%d" % k for k, (_, g) in enumerate(powers, 1))
    assert sum(i == b"%d" % (k - 1) for k, (i, _) in enumerate(powers, 1)) == 171                  # just below their integer
    assert powers[0] == [b"0", b"1"] and powers[2] == [b"2", b"3"] and powers[299] == [b"299", b"300"]
    assert line_of(hi, b"0.000000e+00", q)[4:6] == [b"inf", b"inf"] and line_of(hi, b"1.000000e+00", q)[4:6] == [b"0", b"0"]
    assert line_of(hi, b"2.000000e+00", q)[4:6] == [b"0", b"-0.30103"] and line_of(hi, b"9.999999e-01", q)[4:6] == [b"0", b"4.34295e-08"]
    assert line_of(hi, b"1.234567e+02", q) is None and line_of(hi, b"1.000001e+00", q)[4:6] == [b"0", b"-4.34294e-07"]
    for track in (lo, hi):                                            # kept at both thresholds by the string comparison: '.' < 'e'
        assert line_of(track, b"1.000000e-320", q)[4:6] == [b"320", b"320"] and line_of(track, b"1.000000e+309", q)[4:6] == [b"-inf", b"-inf"]
    assert line_of(hi, b"4.940656e-324", q)[4:6] == [b"323", b"323.306"] and line_of(lo, b"4.940656e-324", q) is None         # '4' > '1'
    assert b"chr2 -1 8 " in lo and b" chr2 -1 1 SOURCE_NAME . chr2 6 8 TARGET_NAME +" in lo       # midpoints 0 and 007
    assert b"chr2 999999998 1 " in lo and b" chr2 999999998 1000000000 SOURCE_NAME " in lo
    assert not n.endswith(b"\n") and run_track(RUNS["ucn"]).endswith(b" chr6 4752499 4752501 TARGET_NAME +\n")
    assert n.splitlines()[0].split()[6] == b"q-value" and b"\t" not in n.splitlines()[0]
    assert run_track(RUNS["uce"]) == um.HEAD and e.count(b"\n") == 41
    assert all(os.path.getsize(os.path.join(UC, f)) < 16384 for f in os.listdir(UC))


@pytest.mark.parametrize("name", sorted(RUNS))
def test_model_reproduces_the_script_s_track(name):
    run = RUNS[name]
    got, kept = um.track(run_input(run), run["qval"])
    assert got == run_track(run) and kept == got.count(b"\n") - 2


# ---- the installed awk ------------------------------------------------------------------------------------------------------
def random_fields(seed, n):
    rng = np.random.default_rng(seed)
    mant, ex = rng.integers(1000000, 10000000, n), rng.integers(-307, 1, n)
    fields = [b"%d.%06de%s%02d" % (m // 1000000, m % 1000000, b"-" if x < 0 else b"+", abs(x)) for m, x in zip(mant.tolist(), ex.tolist())]
    fields[::997] = [b"1.000000e-%02d" % (1 + k % 307) for k in range(len(fields[::997]))]
    fields[5::1009] = [[b"0.000000e+00", b"1.000000e+00", b"1.000001e+00", b"2.000000e+00", b"5.000000e+307", b"1.000000e-320", b"4.940656e-324",
                        b"1.000000e+309", b"9.999999e-01", b"9.999990e-01"][k % 10] for k in range(len(fields[5::1009]))]
    return fields


def awk_track(data, qval, tmp_path):
    src = str(tmp_path / "lines.txt")
    with open(src, "wb") as f:
        f.write(data)
    r = subprocess.run("cat %s | awk -v q=\"%s\" '{if($7<q){print $0}}' | awk '%s'" % (src, qval, AWK), shell=True, env=dict(os.environ, LC_ALL="C"),
                       capture_output=True, check=True)
    return um.HEAD + r.stdout


@pytest.mark.skipif(not _mawk(), reason="the installed awk is not mawk 1.3.4")
@pytest.mark.parametrize("qval", ["1e-5", "0.05", "5"])
def test_model_equals_the_installed_awk_on_random_lines(qval, tmp_path):
    data = um.rows_of(random_fields(["1e-5", "0.05", "5"].index(qval), 100000))
    got, kept = um.track(data, qval)
    assert got == awk_track(data, qval, tmp_path) and 90000 < kept < 100000


@pytest.mark.skipif(not _mawk(), reason="the installed awk is not mawk 1.3.4")
def test_model_equals_the_installed_awk_next_to_the_boundaries(tmp_path):
    fields = um.near_boundary_fields()
    assert len(fields) == 800 and len(set(f[8:] for f in fields)) == 4
    data = um.rows_of(fields)
    got, kept = um.track(data, "5")
    assert kept == 800 and got == awk_track(data, "5", tmp_path)
    scores = [line.split()[5] for line in got.splitlines()[2:]]
    assert any(b"e-0" in s for s in scores) and any(s.startswith(b"119.") for s in scores)


# ---- the library's two routes for the score, on the host --------------------------------------------------------------------
def test_host_routes_give_the_model_s_score_fields():
    from fithic_amd import _capi
    fields = um.near_boundary_fields() + random_fields(7, 20000) + [b"1.000000e-%02d" % k for k in range(1, 308)]
    deferred = 0
    for f in fields:
        want = " ".join(um.score_fields(f)).encode()
        assert _capi.ms_score_text(f) == want, f
        if f[:1] != b"0" and um.mm.classify(f) == "numeric":
            got = _capi.ms_score_text(f, certify=True)
            assert got in (b"", want), f
            deferred += not got
            if f[:8] == b"1.000000":
                assert got == b""                                     # the score of a power of ten is an integer: never certified
    assert 307 <= deferred < 307 + 800 + 60                           # the powers of ten, the boundary set, 1 in 1000 of the rest


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def test_entry_points_raise_without_a_usable_device_and_refuse_the_threshold_first(tmp_path):
    from fithic_amd import _capi, ucsc
    path = str(tmp_path / "sig.txt")
    open(path, "w").close()
    with pytest.raises(_capi.FhxError):
        ucsc.track(path, "0.05", device=1 << 20)
    for qval in ("", "-0.05", "nan", "1e-320", "5%"):
        with pytest.raises(ValueError):
            ucsc.track(path, qval, device=1 << 20)
    with pytest.raises(SystemExit):
        ucsc.main([path, str(tmp_path / "out.txt")])
    assert not (tmp_path / "out.txt").exists()


def test_refusals_become_the_documented_exceptions(tmp_path):
    from fithic_amd import _capi, ucsc
    path = str(tmp_path / "sig.txt")
    with open(path, "wb") as f:
        f.write(b"header\nchr1 -5 chr1 2 3 1e-3 1.000000e-02\n" + b"c" * 64 + b" 1 chr1 2 3 4 1.000000e-02\nchr1 1 chr1\n")
    e = ucsc._refusal(path, _capi.MsRefused(-4, "x", _capi.MS_MIDPOINT, 2))
    assert isinstance(e, ValueError) and "line 2" in str(e) and "-5" in str(e) and "fithic_amd.ucsc does not take it" in str(e)
    e = ucsc._refusal(path, _capi.MsRefused(-4, "x", _capi.MS_NAME, 3))
    assert isinstance(e, ValueError) and "line 3" in str(e) and "63 bytes" in str(e)
    e = ucsc._refusal(path, _capi.MsRefused(-4, "x", _capi.MS_TOKENS, 4))
    assert isinstance(e, ValueError) and "line 4" in str(e) and "3 token(s)" in str(e) and "fithic_amd.ucsc" in str(e)
    assert isinstance(ucsc._refusal(path, _capi.MsRefused(-4, "x", _capi.MS_KEPT, 0)), ValueError)
    assert (_capi.MS_MIDPOINT, _capi.MS_NAME) == (um.MIDPOINT, um.NAME)
