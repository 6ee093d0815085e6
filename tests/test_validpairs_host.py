"""CPU tests of the validPairs path: the plain-Python model (tests/validpairs_model.py) equals the real script's output on the
fixtures of tests/golden/validpairs (made by tests/golden/make_golden_validpairs.py), fithic_amd.fragments equals the real
createFitHiCFragments-fixedsize.py, and the host writer pads the count as uniq -c does and writes a file the readers take."""
import gzip
import json
import os

import numpy as np
import pytest

import validpairs_model as vm
from conftest import GOLDEN

VP = os.path.join(GOLDEN, "validpairs")
with open(os.path.join(VP, "cases.json")) as _f:
    CASES = json.load(_f)
RUNS = {r["name"]: r for r in CASES["runs"]}
FRAGS = {r["name"]: r for r in CASES["fragments"]}


def _gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def run_input(run):
    data = _gunzip(os.path.join(VP, run["input"]))
    return gzip.compress(data) if run["gzipped_input"] else data


def test_fixtures_were_made_by_the_pinned_tools_and_cover_the_cases_of_the_issue():
    assert CASES["awk"].startswith("mawk 1.3.4") and CASES["locale"] == "LC_ALL=C"
    assert set(r["res"] for r in RUNS.values()) == {10000, 50} and any(r["gzipped_input"] for r in RUNS.values())
    a, b = run_input(RUNS["vpa_r10000"]), run_input(RUNS["vpb_r10000"])
    for needle in (b"\tchr2\t", b"\tchr10\t", b"\t2\t", b"\t10\t", b"\tX\t", b"\tchr11_\t", b"\tchrM\t", b".chrM.", b"chrM_tag", b"\t0\t"):
        assert needle in a
    assert b"\r\n" in b and b"  " in b and not b.endswith(b"\n") and len(a.splitlines()) <= 400
    out = _gunzip(os.path.join(VP, RUNS["vpa_r10000"]["output"]))
    assert out.index(b"chr3\t105000\t") < out.index(b"chr3\t25000\t")        # "100000" sorts before "20000"
    assert b"chr5\t75000\tchr6\t85000\t     16\n" in out                           # duplicates, in both orders of the ends


@pytest.mark.parametrize("name", sorted(RUNS))
def test_model_reproduces_the_script_s_output(name):
    run = RUNS[name]
    assert vm.text(run_input(run), run["res"]) == _gunzip(os.path.join(VP, run["output"]))


def test_the_examples_of_the_issue():
    line = lambda a, p, b, q: b"r\t%s\t%d\t+\t%s\t%d\t-\n" % (a, p, b, q)
    assert vm.pairs(line(b"chr1", 50000, b"chr1", 50101), 10000) == []        # 101^2 <= 20000
    assert len(vm.pairs(line(b"chr1", 50000, b"chr1", 50142), 10000)) == 1    # 142^2 > 20000
    assert vm.text(line(b"chr2", 7000, b"chr1", 21000) * 2, 10000) == b"chr1\t25000\tchr2\t5000\t      2\n"
    assert vm._awk_less(b"chr10", b"chr2") and vm._awk_less(b"2", b"10") and vm._awk_less(b"10", b"X") and not vm._awk_less(b"X", b"10")
    assert vm.text(b"", 10000) == b""


@pytest.mark.parametrize("bad, why", [(b"r chr1 5 + chr2", vm.TOKENS), (b"", vm.TOKENS), (b"r +x 5 + chr2 9", vm.NAME), (b"r 1x 5 + chr2 9", vm.NAME),
                                      (b"r 02 5 + chr2 9", vm.NAME), (b"r Inf 5 + chr2 9", vm.NAME), (b"r chr1 5 + nan1 9", vm.NAME),
                                      (b"r chr1 -5 + chr2 9", vm.POSITION), (b"r chr1 5 + chr2 1e3", vm.POSITION),
                                      (b"r chr1 2147480000 + chr2 9", vm.RANGE), (b"r chr1 5 + chr2 9 \x00", vm.BYTES),
                                      (b"r chr1 5 + ch\xe9 9", vm.BYTES), (b"r chr1 5\r + chr2 9", vm.BYTES), (b"r" * 4097 + b" chr1 5 + chr2 9", vm.LONG_LINE)])
def test_model_refuses_what_the_grammar_leaves_out(bad, why):
    good = b"r chr1 5 + chr2 9\n"
    with pytest.raises(vm.Refused) as e:
        vm.pairs(good * 3 + bad + b"\n" + good, 10000)
    assert (e.value.why, e.value.line) == (why, 4)


def test_model_drops_what_the_script_s_first_filters_drop_before_it_reads_names_and_positions():
    assert vm.pairs(b"r chr100 x + 1x -9\nr 02 1e3 + chr1 9 chrM\n", 10000) == []
    for res in (0, 1, 9999):
        with pytest.raises(vm.Refused) as e:
            vm.pairs(b"", res)
        assert e.value.why == vm.RES


# ---- fragments --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FRAGS))
def test_fragments_equal_the_reference_s(name, tmp_path, capsys):
    from fithic_amd import fragments, tables
    case = FRAGS[name]
    sizes, out = str(tmp_path / "chrom.sizes"), str(tmp_path / "frags.gz")
    with open(sizes, "w") as f:
        f.write(case["chr_lens"])
    fragments.main(["--chrLens", sizes, "--outFile", out, "--resolution", str(case["res"])])
    assert capsys.readouterr().out.replace(os.path.realpath(str(tmp_path)), "<DIR>") == case["stdout"]
    want = _gunzip(os.path.join(VP, case["output"]))
    assert _gunzip(out) == want and not want.endswith(b"\n")
    a, b = tables.ChromIndex(), tables.ChromIndex()
    got, read = fragments.bins(sizes, case["res"], a), tables.read_fragments(out, b)
    assert a.names == b.names
    for g, r in zip(got, read):
        assert g.dtype == np.int32 and np.array_equal(g, r)


# ---- the writer -------------------------------------------------------------------------------------------------------------
def test_writer_pads_the_count_as_uniq_does_and_the_reader_takes_the_file(tmp_path):
    from fithic_amd import _capi, tables
    names = ["10", "X", "chr1"]
    cols = [np.array(v, np.int32) for v in ([0, 1, 2, 2], [5000, 15000, 25, 2147483647], [1, 2, 2, 2], [25000, 5000, 75, 25], [1, 9999999, 10000000, 2147483647])]
    path = str(tmp_path / "lib_fithic.contactCounts.gz")
    _capi.vp_write_contacts(path, names, *cols)
    assert _gunzip(path) == (b"10\t5000\tX\t25000\t      1\nX\t15000\tchr1\t5000\t9999999\nchr1\t25\tchr1\t75\t10000000\n"
                             b"chr1\t2147483647\tchr1\t25\t2147483647\n")
    chroms = tables.ChromIndex()
    con = tables.read_contacts(path, chroms)
    assert chroms.names == names
    for got, want in zip((con.chr1, con.mid1, con.chr2, con.mid2, con.count), cols):
        assert np.array_equal(got, want)
    with gzip.open(path, "rt") as f:                                          # the reference's own loop (fithic.py:413-417)
        rows = [line.rstrip().split() for line in f]
    assert [int(r[4]) for r in rows] == cols[4].tolist()
    _capi.vp_write_contacts(path, [], *[np.zeros(0, np.int32)] * 5)
    assert _gunzip(path) == b""


@pytest.mark.parametrize("name", ["vpa_r10000", "vpb_r50"])
def test_model_cells_written_by_the_host_writer_are_the_script_s_bytes(name, tmp_path):
    from fithic_amd import _capi
    run = RUNS[name]
    names, *cols = vm.columns(run_input(run), run["res"])
    path = str(tmp_path / "out.gz")
    _capi.vp_write_contacts(path, names, *cols)
    assert _gunzip(path) == _gunzip(os.path.join(VP, run["output"]))


# ---- the Python surface -----------------------------------------------------------------------------------------------------
def test_entry_points_raise_without_a_usable_device(tmp_path):
    from fithic_amd import _capi, validpairs
    path = str(tmp_path / "x.validPairs")
    open(path, "w").close()
    with pytest.raises(_capi.FhxError):
        validpairs.read(path, 10000, device=1 << 20)
    with pytest.raises(SystemExit):
        validpairs.main(["10000", "lib"])


def test_refusals_become_the_documented_exceptions(tmp_path):
    from fithic_amd import _capi, validpairs
    path = str(tmp_path / "x.validPairs")
    with open(path, "wb") as f:
        f.write(b"r chr1 5 + chr2 9\nr 02 5 + chr2 9\nr chr1\n")
    e = validpairs._refusal(path, 10000, _capi.VpRefused(-4, "x", _capi.VP_NAME, 2))
    assert isinstance(e, ValueError) and "line 2" in str(e) and "'r 02 5 + chr2 9'" in str(e) and "The reference accepts this" in str(e)
    e = validpairs._refusal(path, 10000, _capi.VpRefused(-4, "x", _capi.VP_TOKENS, 3))
    assert "line 3" in str(e) and "2 token(s)" in str(e)
    e = validpairs._refusal(path, 9999, _capi.VpRefused(-4, "x", _capi.VP_RES, 0))
    assert "9999" in str(e) and "The reference accepts this" in str(e)
    for why in (_capi.VP_NAMES, _capi.VP_COUNT, _capi.VP_PAIRS, _capi.VP_BYTES, _capi.VP_LONG_LINE, _capi.VP_POSITION, _capi.VP_RANGE):
        assert isinstance(validpairs._refusal(path, 10000, _capi.VpRefused(-4, "x", why, 1)), ValueError)
