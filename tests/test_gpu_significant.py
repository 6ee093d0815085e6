"""Engine.significant / fhx_significant_select: the FDR subset of a pass taken from its resident q, and `fithic --significant`.

The acceptance relation is  direct == mergefilter.select(the file the same pass writes): the same bytes, n_lines and n_kept, or the
same refusal.  It is checked against that file route after real passes, and against tests/mergefilter_model.py (merge-filter.sh
restated, pinned to the real script by tests/golden/mergefilter) applied to Python's own % formatting of the fetched columns on q
columns the test writes through Context.device_ptr(1).  Small contexts are ranks of a larger run: their rows are the first n of a
synthetic set and the fit is made on the whole set's histogram (fhx_set_global_stats), as a shard of `--gpus N` does it, so that a
context of one row has p and q like any other.  No tolerance anywhere: text is compared byte for byte."""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

import mergefilter_model as mm
from conftest import DATA, GOLDEN

pytestmark = pytest.mark.gpu

RES = 5000
LOW, UP = 6 * RES, 36 * RES                       # the rows were made for 4..40 bins: some loaded rows are not emitted
DONOR_ROWS = 16383
SCAN_ROUND = 256                                   # workgroup counts fhxscan::scan_tiles takes per round
HEADER = b"chr1\tfragmentMid1\tchr2\tfragmentMid2\tcontactCount\tp-value\tq-value\tbias1\tbias2\tExpCC\n"
KEEP, DROP = 1e-3, 0.5                             # q of a kept and of a dropped row at fdr = 0.05
_cache = {}


def _synth():
    """(genome, the contact columns) of the set every context takes its first n rows from"""
    if "rows" not in _cache:
        import torch
        from fithic_amd import synth
        n = SCAN_ROUND * 256 + 1
        loci = n // 20 + 200
        genome = synth.Genome(RES, [RES * (loci * 3 // 5), RES * (loci - loci * 3 // 5)])
        amp = synth.solve_amplitude(0.66, 4, 40)
        cols = [torch.cat(c).numpy() for c in zip(*(synth.cis_contacts(genome, c, 4, 40, amp) for c in range(len(genome))))]
        assert len(cols[0]) >= n, (n, len(cols[0]))
        # rows of both chromosomes within the first few hundred: interleave the two chromosomes' rows
        first = int(np.searchsorted(cols[0], 1))
        order = np.empty(len(cols[0]), np.int64)
        k = min(first, len(order) - first)
        order[0:2 * k:2], order[1:2 * k:2] = np.arange(k), first + np.arange(k)
        order[2 * k:] = np.arange(k, first) if first > k else np.arange(first + k, len(order))
        _cache["rows"] = genome, [np.ascontiguousarray(c[order]) for c in cols]
    return _cache["rows"]


def _new_context(n):
    from fithic_amd.engine import Engine
    genome, cols = _synth()
    eng = Engine(0)                                # raises without a GPU or the library: no fallback
    eng.configure(RES, LOW, UP, 20, 1, "intraOnly")
    eng.load_fragments(*genome.fragments(), genome.sort_rank())
    eng.load_bias(*genome.bias_table())
    eng.load_contacts(*[c[:n] for c in cols])
    return eng


def _donor():
    """stats and distance histograms of the DONOR_ROWS-row set: what every smaller context fits on"""
    if "donor" not in _cache:
        from fithic_amd import _capi
        eng = _new_context(DONOR_ROWS)
        st = eng.pass_stats()
        _cache["donor"] = st, eng.ctx.get_array(_capi.A_HIST_SUMCC), eng.ctx.get_array(_capi.A_HIST_NPAIRS)
        eng.close()
    return _cache["donor"]


class Pass:
    """a context of the first n rows with p and q of one pass; q may then be rewritten"""

    def __init__(self, n, real=False):
        genome, cols = _synth()
        self.n, self.names = n, list(genome.names)
        self.cols = [c[:n] for c in cols]
        self.eng = _new_context(n)
        if real:
            self.eng.run_pass(collect=False)
        else:
            st, hist_cc, hist_np = _donor()
            self.eng.pass_stats()
            self.eng.ctx.set_global_stats(st, hist_cc, hist_np)
            info = self.eng.fit()
            self.eng.ctx.pvalues()
            self.eng.ctx.bh(info.bh_total_tests)
        d = np.abs(self.cols[1].astype(np.int64) - self.cols[3].astype(np.int64))
        self.emit = (self.cols[0] == self.cols[2]) & (d >= LOW) & (d <= UP)
        self.emitted = np.flatnonzero(self.emit)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.close()

    def write_q(self, q):
        q = np.ascontiguousarray(q, np.float64)
        assert len(q) == self.n
        self.eng.ctx.copy(self.eng.ctx.device_ptr(1), q.ctypes.data, 8 * self.n, 0)

    def lines(self):
        """[(loaded row, its line as the writer prints it)] of the emitted rows, from the columns as the context holds them now"""
        v = self.eng.fetch(p=True, q=True, expcc=True, bias=True)
        c = self.cols
        return [(i, ("%s\t%d\t%s\t%d\t%d\t%e\t%e\t%e\t%e\t%f\n" % (self.names[c[0][i]], c[1][i], self.names[c[2][i]], c[3][i], c[4][i], v["p"][i],
                                                                   v["q"][i], v["b1"][i], v["b2"][i], v["expcc"][i])).encode())
                for i in self.emitted.tolist()]

    def model(self, fdr, strict):
        """(text, rows) merge-filter.sh keeps of header + lines()"""
        lines = self.lines()
        text = mm.select(HEADER + b"".join(t for _, t in lines), fdr, strict=strict, skip_first_line=True)
        rows = [i for i, t in lines if mm.keeps(t.split(b"\t")[6], mm.check_fdr(fdr), strict)]
        return text, rows

    def direct(self, fdr, strict=False, names=None):
        """(Selection, rows) of the direct route"""
        sel = self.eng.significant(fdr, names or self.names, strict=strict, path="pass.gz")
        return sel, self.eng.ctx.significant_rows(sel.n_kept).tolist()

    def check(self, fdr, strict, what):
        want, want_rows = self.model(fdr, strict)
        sel, rows = self.direct(fdr, strict)
        assert sel.n_lines == len(self.emitted) + 1, (what, sel.n_lines, len(self.emitted))
        assert sel.n_kept == len(want_rows), (what, sel.n_kept, len(want_rows))
        assert rows == want_rows, (what, "kept rows differ")
        assert sel.subset_text() == want, (what, "text differs")
        return sel


# ---- against the file route, after real passes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [DONOR_ROWS, 3 * 16384 + 127])
def test_direct_equals_selection_from_the_written_file(n, tmp_path):
    from fithic_amd import mergefilter
    path = str(tmp_path / "pass.gz")
    with Pass(n, real=True) as P:
        written, _ = P.eng.ctx.write_significances_device(path, P.names)
        assert 0 < written == len(P.emitted) < n
        for fdr in ("0.05", "1e-5", "5", "0", "1"):
            for strict in (False, True):
                want = mergefilter.select(path, fdr, strict=strict, skip_first_line=True)
                got, _ = P.direct(fdr, strict)
                print(n, fdr, strict, "lines", got.n_lines, "kept", got.n_kept)
                assert (got.n_lines, got.n_kept) == (want.n_lines, want.n_kept), (fdr, strict)
                assert got.subset_text() == want.subset_text(), (fdr, strict)
        assert P.direct("1")[0].n_kept == written                      # every q is at most 1
        # the selection reads the pass, it does not end it: the writer still writes the same file
        again = str(tmp_path / "again.gz")
        P.eng.ctx.write_significances_device(again, P.names)
        with open(path, "rb") as f, open(again, "rb") as g:
            assert f.read() == g.read()


# ---- the rounding boundary, zero, subnormals ------------------------------------------------------------------------------------
def _boundary_values():
    half = float("4.9999995e-02")                   # between 4.999999e-02 and 5.000000e-02
    vals = [float("5.000000e-02"), float("4.999999e-02"), float("5.000001e-02"), np.nextafter(half, 0.0), np.nextafter(half, 1.0), half,
            np.nextafter(0.05, 0.0), np.nextafter(0.05, 1.0), 0.0, 1e-320, float("2.225074e-308"), float("2.225073e-308"),
            2.2250738585072014e-308, np.nextafter(2.2250738585072014e-308, 0.0), 5e-324, 1.0, 5.0, np.nextafter(5.0, 0.0),
            float("1.000000e-05"), float("1.000001e-05"), float("9.999999e-06"), 9.9999995e-06, np.nextafter(9.9999995e-06, 1.0)]
    assert "%e" % vals[3] == "4.999999e-02" and "%e" % vals[4] == "5.000000e-02"
    assert "%e" % vals[10] == "2.225074e-308" and "%e" % vals[11] == "2.225073e-308" and "%e" % vals[12] == "2.225074e-308"
    return np.array(vals, np.float64)


def test_boundary_columns_with_and_without_the_bracket(monkeypatch):
    vals = _boundary_values()
    n = 700
    with Pass(n) as P:
        q = vals[(np.arange(n) * 7) % len(vals)]      # 7 and the number of values are coprime: every value meets emitted rows
        assert set(q[P.emitted].tolist()) == set(vals.tolist())
        P.write_q(q)
        for fdr in ("0.05", "5", "1e-5", "0", "1", "2.225074e-308", "4.9999995e-02", "9.999999e+307"):
            for strict in (False, True):
                monkeypatch.delenv("FHX_SR_NO_BRACKET", raising=False)
                with_bracket = P.check(fdr, strict, ("bracket", fdr, strict))
                monkeypatch.setenv("FHX_SR_NO_BRACKET", "1")
                all_formatted = P.check(fdr, strict, ("no bracket", fdr, strict))
                assert with_bracket.subset_text() == all_formatted.subset_text()
        monkeypatch.delenv("FHX_SR_NO_BRACKET", raising=False)
        # subnormals are no numbers to mawk but strings.  The double 1e-320 prints 9.999889e-321: '9' > '0' drops it at 0.05 and
        # '9' > '5' at 5; 2.225073e-308 is dropped at 0.05 ('2' > '0') and kept at 5 ('2' < '5'); 2.225074e-308 is a number
        tiny = ("%e" % 1e-320).encode()
        assert tiny == b"9.999889e-321"
        col = lambda sel: [ln.split(b"\t")[6] for ln in sel.subset_text().splitlines()]
        at_005, at_5 = col(P.direct("0.05")[0]), col(P.direct("5")[0])
        assert tiny not in at_005 and tiny not in at_5
        assert b"2.225073e-308" not in at_005 and b"2.225073e-308" in at_5
        assert b"2.225074e-308" in at_005 and b"2.225074e-308" in at_5


# ---- row counts and kept patterns ------------------------------------------------------------------------------------------------
def _patterns(P):
    n, em = P.n, P.emitted
    out = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": np.arange(n) % 2 == 0}
    for name, rows in (("first", em[:1]), ("last", em[-1:])):
        out[name] = np.zeros(n, bool)
        out[name][rows] = True
    if n >= 511:                                   # one run from sr_decide's first workgroup into its second, over 256 kept rows
        run = np.zeros(n, bool)
        run[100:500] = True
        kept = run & P.emit
        assert kept[:256].any() and kept[256:].any() and kept.sum() > 256
        gaps = ~P.emit
        assert gaps[:100].any() and gaps[100:500].any() and gaps[500:].any()       # not emitted: before, inside and after the run
        out["run"] = run
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 511, 513, SCAN_ROUND * 256 + 1])
def test_row_counts_and_kept_patterns(n):
    with Pass(n) as P:
        for name, keep in _patterns(P).items():
            P.write_q(np.where(keep, KEEP, DROP))
            sel = P.check("0.05", False, (n, name))
            assert sel.n_kept == int((keep & P.emit).sum()), (n, name)
            print(n, name, "emitted", sel.n_lines - 1, "kept", sel.n_kept, "bytes", len(sel.subset_text()))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _line_of(P, row):
    return 2 + int(P.emit[:row].sum())


def test_refusals_name_the_line_of_the_written_file():
    from fithic_amd import _capi, mergefilter
    n = 2000
    with Pass(n) as P:
        em, off = P.emitted, np.flatnonzero(~P.emit)
        assert len(off) and off[0] < em[-1]
        base = np.where(np.arange(n) % 3 == 0, KEEP, DROP)
        early, late = int(em[len(em) // 3]), int(em[-2])              # in different workgroups, non-emitted rows before both
        assert early // 256 != late // 256 and _line_of(P, early) < early + 2
        for bad in (float("nan"), float("inf"), -0.0, -1e-3, 1e308):
            for row in (early, late, int(em[0])):
                q = base.copy()
                q[row] = bad
                P.write_q(q)
                with pytest.raises(ValueError) as e:
                    P.direct("0.05")
                want = mergefilter._refusal_at("pass.gz, line %d" % _line_of(P, row), _capi.MS_FIELD, "")
                assert not isinstance(e.value, _capi.FhxError) and str(e.value) == str(want), (bad, row, str(e.value))
        # two bad rows: the smaller line, whichever kind sits where and however often it is asked
        for first, second in ((float("nan"), -0.0), (float("inf"), float("nan"))):
            q = base.copy()
            q[early], q[late] = first, second
            P.write_q(q)
            for _ in range(2):
                with pytest.raises(ValueError) as e:
                    P.direct("0.05", strict=True)
                assert "pass.gz, line %d:" % _line_of(P, early) in str(e.value)
        # a bad q on a row the writer does not print is no refusal
        q = base.copy()
        q[off] = float("nan")
        P.write_q(q)
        good = P.check("0.05", False, "nan on rows that are not emitted")
        assert good.n_kept > 0
        # after a refusal nothing is retrievable
        q[early] = float("nan")
        P.write_q(q)
        with pytest.raises(ValueError):
            P.direct("0.05")
        text = np.full(len(good.subset_text()), 0x55, np.uint8)
        rows = np.full(good.n_kept, -7, np.int64)
        L, h = P.eng.ctx._L, P.eng.ctx._h
        assert L.fhx_significant_copy_text(h, text.ctypes.data, len(text)) == _capi.FHX_OK and (text == 0x55).all()
        assert L.fhx_significant_copy_rows(h, _capi._ptr(rows, __import__("ctypes").c_int64), len(rows)) == _capi.FHX_OK and (rows == -7).all()
        assert P.eng.ctx.significant_text(0) == b""


def test_a_kept_row_the_formatter_does_not_cover_is_unsupported():
    from fithic_amd import _capi
    n = 1500
    with Pass(n) as P:
        long_names = [P.names[0], "c" * 25]
        on_long = P.cols[0] == 1
        assert (on_long & P.emit).any() and (~on_long & P.emit).any()
        P.write_q(np.where(on_long, DROP, KEEP))                      # the rows with the 25-byte name are dropped: no text is made of them
        sel, rows = P.direct("0.05", names=long_names)
        assert sel.n_kept == int((~on_long & P.emit).sum()) > 0 and not on_long[rows].any()
        assert sel.subset_text() == P.model("0.05", False)[0]
        q = np.where(on_long, DROP, KEEP)
        q[np.flatnonzero(on_long & P.emit)[-1]] = KEEP                 # one of them kept
        P.write_q(q)
        with pytest.raises(_capi.FhxError) as e:
            P.direct("0.05", names=long_names)
        assert e.value.code == _capi.FHX_ERR_UNSUPPORTED and not isinstance(e.value, _capi.MsRefused)
        assert P.eng.ctx.significant_text(0) == b""
        assert P.direct("0.05")[0].n_kept == sel.n_kept + 1             # the short names: the same rows are fine


def test_only_between_bh_and_next_pass():
    from fithic_amd import _capi
    n = 600
    with Pass(n) as P:
        assert P.direct("0.05")[0].n_lines == len(P.emitted) + 1
        P.eng.next_pass()
        with pytest.raises(_capi.FhxError) as e:
            P.direct("0.05")
        assert e.value.code == _capi.FHX_ERR_ARG
        P.eng.pass_stats()                                                 # the next pass has begun: no q yet
        with pytest.raises(_capi.FhxError) as e:
            P.direct("0.05")
        assert e.value.code == _capi.FHX_ERR_ARG


# ---- the command line --------------------------------------------------------------------------------------------------------------
def _fixture():
    with open(os.path.join(GOLDEN, "significant", "cases.json")) as f:
        meta = json.load(f)
    with gzip.open(os.path.join(GOLDEN, "significant", meta["subset"]), "rb") as f:
        subset = f.read()
    with gzip.open(os.path.join(GOLDEN, "significant", meta["merged"]), "rb") as f:
        merged = f.read()
    return meta, subset, merged


def _gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def _hesc_argv(meta, out, inputs=None):
    inp = inputs or {k: os.path.join(DATA, v) for k, v in meta["inputs"].items()}
    return ["-i", inp["contacts"], "-f", inp["frags"], "-t", inp["bias"], "-o", str(out), "-r", str(meta["res"]), "-p", str(meta["passes"]),
            "-l", meta["lib"], "--significant", meta["fdr"]]


def test_cli_writes_the_reference_subset_and_merged_file(tmp_path, monkeypatch):
    from fithic_amd import cli, mergefilter
    meta, subset, merged = _fixture()

    def no_file_route(*a, **k):
        raise AssertionError("the subset was taken from the written file")
    monkeypatch.setattr(mergefilter, "select", no_file_route)
    full, only = tmp_path / "full", tmp_path / "only"
    cli.main(_hesc_argv(meta, full))
    prefix = "%s.spline_pass%d.res%d" % (meta["lib"], meta["passes"], meta["res"])
    assert hashlib.md5(_gunzip(str(full / (prefix + ".significances.txt.gz")))).hexdigest() == meta["significances_md5"]
    assert _gunzip(str(full / (prefix + ".fdr_subset.txt.gz"))) == subset
    assert _gunzip(str(full / (prefix + ".merged.txt.gz"))) == merged
    assert subset.count(b"\n") == meta["kept"] and len(merged.splitlines()) - 1 == meta["merged_records"]
    # --significant-only: the same two files, no significances file of any pass, everything else as it was
    cli.main(_hesc_argv(meta, only) + ["--significant-only"])
    assert not [f for f in os.listdir(str(only)) if f.endswith(".significances.txt.gz")]
    assert _gunzip(str(only / (prefix + ".fdr_subset.txt.gz"))) == subset
    assert _gunzip(str(only / (prefix + ".merged.txt.gz"))) == merged
    for p in range(1, meta["passes"] + 1):
        name = "%s.fithic_pass%d.res%d.txt" % (meta["lib"], p, meta["res"])
        assert (full / name).read_bytes() == (only / name).read_bytes()
    assert sorted(f for f in os.listdir(str(full)) if not f.endswith(".significances.txt.gz")) == sorted(os.listdir(str(only)))


def test_cli_without_a_bin_lattice_writes_the_subset_only(tmp_path, capsys):
    from fithic_amd import cli, mergefilter
    from conftest import load_case, case_args
    meta, _ = load_case("f8_nonfixed_hESC")
    kw = case_args(meta)
    assert kw["resolution"] == 0
    argv = ["-i", kw["contacts"], "-f", kw["frags"], "-o", str(tmp_path), "-l", "G", "--significant", "0.05"] + meta["argv"]
    if kw["bias_path"]:
        argv += ["-t", kw["bias_path"]]
    cli.main(argv)
    assert "needs a bin lattice" in capsys.readouterr().out
    prefix = "G.spline_pass%d" % meta["n_passes"]
    want = mergefilter.select(str(tmp_path / (prefix + ".significances.txt.gz")), "0.05")
    assert _gunzip(str(tmp_path / (prefix + ".fdr_subset.txt.gz"))) == want.subset_text()
    assert not [f for f in os.listdir(str(tmp_path)) if "merged" in f]


def test_cli_falls_back_to_the_written_file_for_a_long_name(tmp_path, monkeypatch):
    """the chromosome renamed to 25 bytes: the device formatter covers no kept row, the subset comes from the file the run wrote -
    the reference's two files with that name in them"""
    from fithic_amd import cli, mergefilter
    meta, subset, merged = _fixture()
    long_name = b"chr1_" + b"x" * 20
    inputs = {}
    for k, v in meta["inputs"].items():
        text = _gunzip(os.path.join(DATA, v))
        assert all(ln.startswith(b"chr1\t") for ln in text.splitlines()[:50])
        inputs[k] = str(tmp_path / v)
        with gzip.open(inputs[k], "wb", compresslevel=1) as f:
            f.write(text.replace(b"chr1\t", long_name + b"\t"))
    routes = []
    real = mergefilter.select
    monkeypatch.setattr(mergefilter, "select", lambda *a, **k: routes.append(a[0]) or real(*a, **k))
    cli.main(_hesc_argv(meta, tmp_path / "out", inputs))
    prefix = "%s.spline_pass%d.res%d" % (meta["lib"], meta["passes"], meta["res"])
    assert routes == [str(tmp_path / "out" / (prefix + ".significances.txt.gz"))]
    assert _gunzip(str(tmp_path / "out" / (prefix + ".fdr_subset.txt.gz"))) == subset.replace(b"chr1\t", long_name + b"\t")
    head, _, records = merged.partition(b"\n")                                     # the header line names its columns chr1, chr2
    assert _gunzip(str(tmp_path / "out" / (prefix + ".merged.txt.gz"))) == head + b"\n" + records.replace(b"chr1\t", long_name + b"\t")
