"""Engine.track / Engine.split (fhx_significant_track, fhx_significant_split): the UCSC interact track and the per-chromosome FDR
subsets of a pass taken from its resident q, and `fithic --significant FDR --significant-track --significant-split`.

The acceptance relation is  direct == the file route on the file the same pass writes  (ucsc.track, mergefilter_parallel.split):
the same bytes and counts, or the same refusal.  It is checked against those routes after real passes, against the real scripts'
output on the hESC set (tests/golden/significant_views), and against tests/ucsc_model.py / tests/mergesplit_model.py (the two
scripts restated, pinned to the real ones by tests/golden/ucsc and tests/golden/mergesplit) applied to Python's own % formatting
of the fetched columns, on q columns the test writes through Context.device_ptr(1).  Contexts are built as
tests/test_gpu_significant.py builds them: the first n rows of a two-chromosome synthetic set, fitted on a donor's statistics
(fhx_set_global_stats), so that a context of one row has p and q like any other; contexts over another genome run a real pass.
No tolerance anywhere: text is compared byte for byte."""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

import mergefilter_model as mm
import mergesplit_model as sm
import ucsc_model as um
from conftest import DATA, GOLDEN

pytestmark = pytest.mark.gpu

RES = 5000
LOW, UP = 6 * RES, 36 * RES                       # the rows were made for 4..40 bins: some loaded rows are not emitted
DONOR_ROWS = 16383
SCAN_ROUND = 256                                   # workgroup counts fhxscan::scan_tiles takes per round
HEADER = b"chr1\tfragmentMid1\tchr2\tfragmentMid2\tcontactCount\tp-value\tq-value\tbias1\tbias2\tExpCC\n"
KEEP, DROP = 1e-3, 0.5                             # q of a kept and of a dropped row at fdr = 0.05
_cache = {}


# ---- contexts (tests/test_gpu_significant.py's helper, restated, over any genome) ------------------------------------------------
class Source:
    """a genome as the engine's loaders take it, and contact rows on it"""

    def __init__(self, names, frag_chr, frag_mid, bias, cols):
        self.names, self.frag_chr, self.frag_mid, self.bias, self.cols = list(names), frag_chr, frag_mid, bias, cols

    def sort_rank(self):
        order = sorted(range(len(self.names)), key=lambda i: self.names[i])
        rank = np.empty(len(order), np.int32)
        rank[order] = np.arange(len(order), dtype=np.int32)
        return rank


def _synth():
    """the two-chromosome set every small context takes its first n rows from, the chromosomes interleaved row by row"""
    if "rows" not in _cache:
        import torch
        from fithic_amd import synth
        n = SCAN_ROUND * 256 + 1
        loci = n // 20 + 200
        genome = synth.Genome(RES, [RES * (loci * 3 // 5), RES * (loci - loci * 3 // 5)])
        amp = synth.solve_amplitude(0.66, 4, 40)
        cols = [torch.cat(c).numpy() for c in zip(*(synth.cis_contacts(genome, c, 4, 40, amp) for c in range(len(genome))))]
        assert len(cols[0]) >= n, (n, len(cols[0]))
        first = int(np.searchsorted(cols[0], 1))
        order = np.empty(len(cols[0]), np.int64)
        k = min(first, len(order) - first)
        order[0:2 * k:2], order[1:2 * k:2] = np.arange(k), first + np.arange(k)
        order[2 * k:] = np.arange(k, first) if first > k else np.arange(first + k, len(order))
        ch, mid, _ = genome.fragments()
        _cache["rows"] = Source(genome.names, ch, mid, genome.bias_table()[2], [np.ascontiguousarray(c[order]) for c in cols])
    return _cache["rows"]


def _extended(extra_names, extra_loci, extra_rows, offsets=None):
    """the synthetic set with more chromosomes behind its two (extra_loci bins each, the first midpoint at offsets[i], default
    RES // 2) and `extra_rows` (five columns) behind its first DONOR_ROWS rows"""
    base = _synth()
    offsets = offsets or [RES // 2] * len(extra_names)
    ids = np.arange(len(extra_names), dtype=np.int32) + len(base.names)
    frag_chr = np.concatenate([base.frag_chr] + [np.full(n, c, np.int32) for c, n in zip(ids, extra_loci)])
    frag_mid = np.concatenate([base.frag_mid] + [(np.arange(n, dtype=np.int64) * RES + off).astype(np.int32) for n, off in zip(extra_loci, offsets)])
    bias = np.concatenate([base.bias, np.ones(int(sum(extra_loci)))])
    cols = [np.ascontiguousarray(np.concatenate([c[:DONOR_ROWS], np.asarray(e, np.int32)])) for c, e in zip(base.cols, extra_rows)]
    return Source(base.names + list(extra_names), frag_chr, frag_mid, bias, cols)


def _new_context(src, n, mode="intraOnly"):
    from fithic_amd.engine import Engine
    eng = Engine(0)                                # raises without a GPU or the library: no fallback
    eng.configure(RES, LOW, UP, 20, 1, mode)
    eng.load_fragments(src.frag_chr, src.frag_mid, np.ones(len(src.frag_chr), np.int32), src.sort_rank())
    eng.load_bias(src.frag_chr, src.frag_mid, src.bias)
    eng.load_contacts(*[c[:n] for c in src.cols])
    return eng


def _donor():
    """stats and distance histograms of the DONOR_ROWS-row set: what every smaller context fits on"""
    if "donor" not in _cache:
        from fithic_amd import _capi
        eng = _new_context(_synth(), DONOR_ROWS)
        st = eng.pass_stats()
        _cache["donor"] = st, eng.ctx.get_array(_capi.A_HIST_SUMCC), eng.ctx.get_array(_capi.A_HIST_NPAIRS)
        eng.close()
    return _cache["donor"]


class Pass:
    """a context of the first n rows of a source with p and q of one pass; q may then be rewritten"""

    def __init__(self, n, real=False, src=None, mode="intraOnly", names=None):
        src = src or _synth()
        self.n, self.names = n, list(names or src.names)
        self.cols = [c[:n] for c in src.cols]
        self.eng = _new_context(src, n, mode)
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
        cis = self.cols[0] == self.cols[2]
        self.emit = (cis & (d >= LOW) & (d <= UP)) if mode == "intraOnly" else (~cis | ((d >= LOW) & (d <= UP)))
        self.emitted = np.flatnonzero(self.emit)
        self._fixed = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.close()

    def write_q(self, q):
        q = np.ascontiguousarray(q, np.float64)
        assert len(q) == self.n
        self.eng.ctx.copy(self.eng.ctx.device_ptr(1), q.ctypes.data, 8 * self.n, 0)

    def file(self, names=None):
        """the file the writer would write of the columns as the context holds them now: the header, then the emitted rows"""
        names = names or self.names
        if self._fixed is None:                    # everything but q stays as the pass left it
            self._fixed = self.eng.fetch(p=True, q=False, expcc=True, bias=True)
        v, q, c = self._fixed, self.eng.fetch(p=False, q=True)["q"], self.cols
        return HEADER + b"".join(("%s\t%d\t%s\t%d\t%d\t%e\t%e\t%e\t%e\t%f\n" % (names[c[0][i]], c[1][i], names[c[2][i]], c[3][i], c[4][i], v["p"][i],
                                                                                q[i], v["b1"][i], v["b2"][i], v["expcc"][i])).encode()
                                 for i in self.emitted.tolist())

    def line_of(self, row):
        return 2 + int(self.emit[:row].sum())

    def track(self, qval, names=None):
        return self.eng.track(qval, names or self.names, path="pass.gz")

    def split(self, fdr, names=None):
        return self.eng.split(fdr, names or self.names, path="pass.gz")

    def check_track(self, qval, what, names=None):
        want, kept = um.track(self.file(names), qval)
        got = self.track(qval, names)
        assert got.n_lines == len(self.emitted) + 1, (what, got.n_lines, len(self.emitted))
        assert got.n_kept == kept, (what, got.n_kept, kept)
        assert got.text() == want, (what, "track differs")
        nr = [int(ln.split(b" ")[3]) for ln in got.text().splitlines()[2:]]
        assert nr == list(range(1, kept + 1)), (what, "NR")
        return got

    def check_split(self, fdr, what, names=None):
        want = sm.split(self.file(names), fdr)
        got = self.split(fdr, names)
        assert got.n_lines == len(self.emitted) + 1, (what, got.n_lines, len(self.emitted))
        assert got.chromosomes == [c.decode() for c in sorted(want)], (what, got.chromosomes)
        for name, text in want.items():
            assert got.subset_text(name) == text, (what, name, "subset differs")
            assert got.n_kept(name) == text.count(b"\n"), (what, name)
        return got


def _same_track(a, b, what):
    assert (a.n_lines, a.n_kept, a.n_deferred) == (b.n_lines, b.n_kept, b.n_deferred), (what, (a.n_lines, a.n_kept, a.n_deferred),
                                                                                      (b.n_lines, b.n_kept, b.n_deferred))
    assert a.text() == b.text(), (what, "track differs")


def _same_split(a, b, what):
    assert a.chromosomes == b.chromosomes and a.n_lines == b.n_lines, (what, a.chromosomes, b.chromosomes, a.n_lines, b.n_lines)
    for name in b.chromosomes:
        assert a.n_kept(name) == b.n_kept(name), (what, name, a.n_kept(name), b.n_kept(name))
        assert a.subset_text(name) == b.subset_text(name), (what, name, "subset differs")


# ---- 1. the real scripts' output on the hESC set ------------------------------------------------------------------------------------
def _gunzip(path):
    with gzip.open(path, "rb") as f:
        return f.read()


def _fixture():
    with open(os.path.join(GOLDEN, "significant_views", "cases.json")) as f:
        meta = json.load(f)
    with open(os.path.join(GOLDEN, "significant_views", meta["chromosomes_used"]), "rb") as f:
        meta["used"] = f.read().decode().split("\n")[:-1]
    track = _gunzip(os.path.join(GOLDEN, "significant_views", meta["track"]))
    assert hashlib.md5(track).hexdigest() == meta["track_md5"]
    return meta, track, _gunzip(os.path.join(GOLDEN, "significant", "fithic_subset.gz")), _gunzip(os.path.join(GOLDEN, "significant", "merged.gz"))


def _hesc_argv(meta, out, inputs=None):
    inp = inputs or {k: os.path.join(DATA, v) for k, v in meta["inputs"].items()}
    return ["-i", inp["contacts"], "-f", inp["frags"], "-t", inp["bias"], "-o", str(out), "-r", str(meta["res"]), "-p", str(meta["passes"]),
            "-l", meta["lib"], "--significant", meta["fdr"], "--significant-track", "--significant-split", "--significant-only"]


def _count_writes(monkeypatch):
    from fithic_amd import fithic as F
    writes, real = [], F._write_significances
    monkeypatch.setattr(F, "_write_significances", lambda S, name: writes.append(name) or real(S, name))
    return writes


def test_cli_writes_the_scripts_track_and_tree(tmp_path, monkeypatch, capsys):
    from fithic_amd import cli, mergefilter, mergefilter_parallel, ucsc
    meta, track, subset, merged = _fixture()

    def no_file_route(*a, **k):
        raise AssertionError("a product was taken from the written file")
    monkeypatch.setattr(mergefilter, "select", no_file_route)
    monkeypatch.setattr(ucsc, "track", no_file_route)
    monkeypatch.setattr(mergefilter_parallel, "split", no_file_route)
    writes = _count_writes(monkeypatch)
    out = tmp_path / "out"
    cli.main(_hesc_argv(meta, out))
    said = capsys.readouterr().out
    prefix = "%s.spline_pass%d.res%d" % (meta["lib"], meta["passes"], meta["res"])
    assert not writes and not [f for f in os.listdir(str(out)) if f.endswith(".significances.txt.gz")]
    assert (out / (prefix + ".interact.txt")).read_bytes() == track
    assert track.count(b"\n") == meta["track_lines"]
    assert prefix + ".interact.txt" in said and prefix + ".fdr_split" in said
    tree = str(out / (prefix + ".fdr_split"))
    assert sorted(os.listdir(tree)) == sorted(meta["used"]) == sorted(meta["chromosomes"])
    for name, want in meta["chromosomes"].items():
        part = _gunzip(os.path.join(tree, name, "subset_fithic_%s.gz" % name))
        assert hashlib.md5(part).hexdigest() == want["subset_md5"] and part.count(b"\n") == want["subset_lines"], name
        with open(os.path.join(tree, name, "fithic_%s.job" % name)) as f:
            assert f.read() == want["job"].replace("{OUTDIR}", tree), name
    # one chromosome: its subset is the one-file subset and its postmerged file the one-file script's merged file
    assert meta["used"] == ["chr1"] and _gunzip(os.path.join(tree, "chr1", "subset_fithic_chr1.gz")) == subset
    assert _gunzip(os.path.join(tree, "chr1", "postmerged_fithic_chr1.gz")) == merged
    assert _gunzip(str(out / (prefix + ".merged.txt.gz"))) == merged


def test_cli_falls_back_to_one_written_file_for_a_long_name(tmp_path, monkeypatch):
    """the chromosome renamed to 25 bytes: the device formatter covers no kept row, so all three products come from the file - which
    --significant-only writes once and removes - and are the scripts' with that name in them; the header's chr1 is still listed"""
    from fithic_amd import cli, mergefilter, mergefilter_parallel, ucsc
    meta, track, subset, merged = _fixture()
    long_name = b"chr1_" + b"x" * 20
    inputs = {}
    for k, v in meta["inputs"].items():
        text = _gunzip(os.path.join(DATA, v))
        inputs[k] = str(tmp_path / v)
        with gzip.open(inputs[k], "wb", compresslevel=1) as f:
            f.write(text.replace(b"chr1\t", long_name + b"\t"))
    routes = []
    for module, entry in ((mergefilter, "select"), (ucsc, "track"), (mergefilter_parallel, "split")):
        real = getattr(module, entry)
        monkeypatch.setattr(module, entry, lambda *a, _real=real, _entry=entry, **k: routes.append((_entry, a[0])) or _real(*a, **k))
    writes = _count_writes(monkeypatch)
    out = tmp_path / "out"
    cli.main(_hesc_argv(meta, out, inputs))
    prefix = "%s.spline_pass%d.res%d" % (meta["lib"], meta["passes"], meta["res"])
    name = str(out / (prefix + ".significances.txt.gz"))
    assert routes == [("select", name), ("track", name), ("split", name)] and writes == [name] and not os.path.exists(name)
    renamed = long_name.decode()
    assert (out / (prefix + ".interact.txt")).read_bytes() == track.replace(b"chr1 ", long_name + b" ")
    tree = str(out / (prefix + ".fdr_split"))
    assert sorted(os.listdir(tree)) == ["chr1", renamed]
    assert _gunzip(os.path.join(tree, "chr1", "subset_fithic_chr1.gz")) == b""
    assert _gunzip(os.path.join(tree, renamed, "subset_fithic_%s.gz" % renamed)) == subset.replace(b"chr1\t", long_name + b"\t")
    head, _, records = merged.partition(b"\n")
    assert _gunzip(os.path.join(tree, renamed, "postmerged_fithic_%s.gz" % renamed)) == head + b"\n" + records.replace(b"chr1\t", long_name + b"\t")


# ---- 2. against the file routes, after real passes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [DONOR_ROWS, 3 * 16384 + 127])
def test_direct_equals_the_file_routes(n, tmp_path):
    from fithic_amd import mergefilter_parallel, ucsc
    path = str(tmp_path / "pass.gz")
    with Pass(n, real=True) as P:
        written, _ = P.eng.ctx.write_significances_device(path, P.names)
        assert 0 < written == len(P.emitted) < n
        for fdr in ("0.05", "1e-5", "5", "0", "1"):
            want, got = ucsc.track(path, fdr), P.track(fdr)
            print(n, fdr, "track: lines", got.n_lines, "kept", got.n_kept, "deferred", got.n_deferred)
            _same_track(got, want, (n, fdr))
            want, got = mergefilter_parallel.split(path, fdr), P.split(fdr)
            print(n, fdr, "split:", {c: got.n_kept(c) for c in got.chromosomes})
            _same_split(got, want, (n, fdr))
        assert P.track("5").n_kept == written and sum(P.split("1").n_kept(c) for c in P.names) == written        # every q is at most 1
        # the selections read the pass, they do not end it: the writer still writes the same file
        again = str(tmp_path / "again.gz")
        P.eng.ctx.write_significances_device(again, P.names)
        with open(path, "rb") as f, open(again, "rb") as g:
            assert f.read() == g.read()


# ---- 3. injected q against the models ---------------------------------------------------------------------------------------------------
def _patterns(P):
    n, em = P.n, P.emitted
    out = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "alternating": np.arange(n) % 2 == 0}
    for name, rows in (("first", em[:1]), ("last", em[-1:])):
        out[name] = np.zeros(n, bool)
        out[name][rows] = True
    if n >= 511:                                   # one run from the first workgroup into the second, over 256 kept rows
        run = np.zeros(n, bool)
        run[100:500] = True
        kept = run & P.emit
        assert kept[:256].any() and kept[256:].any() and kept.sum() > 256
        gaps = ~P.emit
        assert gaps[:100].any() and gaps[100:500].any() and gaps[500:].any()       # not emitted: before, inside and after the run
        out["run"] = run
    return out


def _kept_values():
    """q values below 0.05 of every route of the score: next to a boundary of int() or %.6g (certified or deferred by the error
    bound), exact powers of ten (deferred), zero (`inf inf`)"""
    if "kept_values" not in _cache:
        near = [float(f) for f in um.near_boundary_fields(exponents=(-5, -17, -120), each=40)]
        _cache["kept_values"] = np.array(near + [10.0 ** -k for k in range(2, 40)] + [0.0, KEEP, 1.234567e-7], np.float64)
    return _cache["kept_values"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 511, 513, SCAN_ROUND * 256 + 1])
def test_row_counts_and_kept_patterns(n):
    vals = _kept_values()
    with Pass(n) as P:
        for name, keep in _patterns(P).items():
            if n > 4096 and name in ("all", "none", "first"):
                continue                            # the large context: the three patterns whose kept rows differ in kind
            P.write_q(np.where(keep, vals[np.arange(n) % len(vals)], DROP))
            t = P.check_track("0.05", (n, name))
            s = P.check_split("0.05", (n, name))
            assert t.n_kept == int((keep & P.emit).sum()) == sum(s.n_kept(c) for c in s.chromosomes), (n, name)
            print(n, name, "emitted", t.n_lines - 1, "kept", t.n_kept, "deferred", t.n_deferred, "bytes", len(t.text()))


@pytest.mark.parametrize("kept", [9, 10, 99, 100, 999, 1000])
def test_nr_where_its_digit_count_changes(kept):
    """NR runs 1 ... n_kept with exactly `kept` kept rows: the last line's NR has one digit more than the line's before it, or not"""
    n = 2600
    with Pass(n) as P:
        assert len(P.emitted) >= 1000
        q = np.full(n, DROP)
        q[P.emitted[::2][:kept] if kept <= len(P.emitted[::2]) else P.emitted[:kept]] = KEEP
        P.write_q(q)
        t = P.check_track("0.05", kept)
        assert t.n_kept == kept and t.text().splitlines()[-1].split(b" ")[3] == b"%d" % kept


def half_up():
    return float("4.9999995e-02")                                   # between 4.999999e-02 and 5.000000e-02


def _all_values():
    near = [float(f) for f in um.near_boundary_fields()]           # exponents -1, -5, -17, -120
    half = half_up()                                                # the %e rounding boundary at the bound 0.05
    edge = [float("5.000000e-02"), float("4.999999e-02"), float("5.000001e-02"), np.nextafter(half, 0.0), np.nextafter(half, 1.0), half,
            np.nextafter(0.05, 0.0), np.nextafter(0.05, 1.0)]
    special = [0.0, 1.0, float("9.999999e-01"), 1e-320, float("2.225073e-308"), float("2.225074e-308"), 5e-324, 5.0, np.nextafter(5.0, 0.0), 2.5]
    assert "%e" % edge[3] == "4.999999e-02" and "%e" % edge[4] == "5.000000e-02" and "%e" % special[3] == "9.999889e-321"
    return np.array(near + [10.0 ** -k for k in range(0, 60)] + edge + special, np.float64)


def test_every_route_of_the_score_with_and_without_the_bracket(monkeypatch):
    from fithic_amd import _capi
    vals = _all_values()
    n = 2 * len(vals) + 300
    with Pass(n) as P:
        q = vals[(np.arange(n) * 7) % len(vals)]
        assert len(vals) % 7 != 0                                      # 7 and the number of values are coprime: every value is in q
        must = [0.0, 1.0, float("9.999999e-01"), 1e-320, float("2.225073e-308"), float("4.999999e-02"), np.nextafter(half_up(), 0.0), 1e-3, 1e-20]
        assert set(must) <= set(q[P.emitted].tolist())                 # and these meet rows the writer prints
        P.write_q(q)
        for fdr in ("0.05", "5", "1", "0", "1e-5", "2.225074e-308", "4.9999995e-02"):
            monkeypatch.delenv("FHX_SR_NO_BRACKET", raising=False)
            with_bracket = P.check_track(fdr, ("bracket", fdr))
            split_bracket = P.check_split(fdr, ("bracket", fdr))
            monkeypatch.setenv("FHX_SR_NO_BRACKET", "1")
            _same_track(P.check_track(fdr, ("no bracket", fdr)), with_bracket, fdr)
            _same_split(P.check_split(fdr, ("no bracket", fdr)), split_bracket, fdr)
            print(fdr, "kept", with_bracket.n_kept, "deferred", with_bracket.n_deferred)
        monkeypatch.delenv("FHX_SR_NO_BRACKET", raising=False)
        # the powers of ten are deferred, and so are q = 1 and the string class the comparison keeps at 5
        t = P.track("5")
        assert t.n_deferred > 0
        lines = t.text().splitlines()[2:]
        fields = {ln.split(b" ")[4:6] == [b"inf", b"inf"] for ln in lines}
        assert True in fields and False in fields                    # the zero class and the others
        kept_fields = [f for f in (("%e" % qi).encode() for qi in q[P.emitted].tolist()) if mm.keeps(f, mm.check_fdr("5"), True)]
        assert len(kept_fields) == t.n_kept
        # every power of ten and every field of the string class has to go to the host; the error bound may defer more
        must_defer = sum(1 for f in kept_fields if mm.classify(f) == "string" or (f.startswith(b"1.000000e") and mm.classify(f) == "numeric"))
        assert t.n_deferred >= must_defer > 60
        assert any(mm.classify(f) == "string" for f in kept_fields)


# ---- 4. split shapes ----------------------------------------------------------------------------------------------------------------------
def test_split_of_interleaved_chromosomes_and_an_empty_one():
    n = 1500
    with Pass(n) as P:
        assert (P.cols[0][:64] == 0).any() and (P.cols[0][:64] == 1).any()         # both chromosomes within one wave
        on2 = P.cols[0] == 1
        P.write_q(np.where(np.arange(n) % 3 == 0, KEEP, DROP))
        s = P.check_split("0.05", "interleaved")
        assert s.chromosomes == ["chr1", "chr2"] and s.n_kept("chr1") > 0 and s.n_kept("chr2") > 0
        P.write_q(np.where(on2, DROP, KEEP))                                       # chr2: listed, no kept row
        s = P.check_split("0.05", "one chromosome empty")
        assert s.chromosomes == ["chr1", "chr2"] and s.n_kept("chr2") == 0 and s.subset_text("chr2") == b"" and s.n_kept("chr1") > 0


def test_split_lists_the_headers_chr1_and_orders_names_bytewise():
    n = 1500
    with Pass(n) as P:
        P.write_q(np.where(np.arange(n) % 3 == 0, KEEP, DROP))        # the chromosomes alternate row by row: both have kept rows
        s = P.check_split("0.05", "no chr1 in the genome", names=["chrA", "chrB"])
        assert s.chromosomes == ["chr1", "chrA", "chrB"] and s.n_kept("chr1") == 0 and s.subset_text("chr1") == b""
        s = P.check_split("0.05", "chr10 sorts before chr2", names=["chr2", "chr10"])           # id order is the other one
        assert s.chromosomes == ["chr1", "chr10", "chr2"] and s.n_kept("chr10") > 0 and s.n_kept("chr2") > 0
        t = P.check_track("0.05", "names", names=["chr2", "chr10"])
        assert t.n_kept == s.n_kept("chr10") + s.n_kept("chr2")


@pytest.mark.parametrize("n", [257, 600])
def test_the_subset_the_split_and_the_track_of_one_pass_agree(n):
    """Engine.significant and Engine.split run the same kept-row steps (kept_extras, format_kept) over the kept rows in file order
    and in name order: the cis lines of the one text, grouped by field 1, are byte for byte the subsets of the other.  257 loaded
    rows are one full workgroup of sr_decide and one row; at 600 the kept rows themselves fill more than one workgroup of 256,
    whose byte offset is no multiple of 16 (window_out's vector and bytewise paths), at another row in the split than in the
    subset.  The track's kept count is the strict subset's."""
    with Pass(n) as P:
        assert (P.cols[0][:64] == 0).any() and (P.cols[0][:64] == 1).any()         # the chromosomes alternate row by row
        for what, keep in (("every third row", np.arange(n) % 3 == 0), ("all", np.ones(n, bool))):
            P.write_q(np.where(keep, KEEP, DROP))
            subset = P.eng.significant("0.05", P.names)
            s = P.split("0.05")
            assert subset.n_kept == int((keep & P.emit).sum()) > 0 and subset.n_lines == s.n_lines, (n, what)
            by_name = {}
            for line in subset.subset_text().splitlines(keepends=True):
                f = line.split(b"\t")
                if f[0] == f[2]:
                    by_name[f[0].decode()] = by_name.get(f[0].decode(), b"") + line
            assert set(by_name) == {"chr1", "chr2"} and s.chromosomes == ["chr1", "chr2"], (n, what, sorted(by_name), s.chromosomes)
            for name in s.chromosomes:
                assert s.subset_text(name) == by_name[name], (n, what, name, "the split's subset is not the subset's lines")
                assert s.n_kept(name) == by_name[name].count(b"\n"), (n, what, name)
            assert P.track("0.05").n_kept == P.eng.significant("0.05", P.names, strict=True).n_kept, (n, what)
            if n == 600 and what == "all":
                second = sum(len(line) for line in subset.subset_text().splitlines(keepends=True)[:256])
                assert subset.n_kept > 256 and second % 16 != 0, (subset.n_kept, second)      # the second workgroup's first byte


def _trans_source():
    """the synthetic set and a third chromosome that only has trans rows (its first chromosome: listed, no cis row)"""
    base = _synth()
    k = 40
    third = len(base.names)
    rows = [np.full(k, third), np.arange(k) * RES + RES // 2, np.zeros(k), base.frag_mid[base.frag_chr == 0][10:10 + k], np.arange(k) % 5 + 1]
    return _extended(["chr3"], [100], rows)


def test_split_of_an_all_run_lists_trans_rows_and_keeps_none_of_them():
    src = _trans_source()
    n = len(src.cols[0])
    with Pass(n, real=True, src=src, mode="All") as P:
        trans = P.cols[0] != P.cols[2]
        assert trans.sum() == 40 and P.emit[trans].all()
        P.write_q(np.where(np.arange(n) % 2 == 0, KEEP, DROP))
        assert (trans & (np.arange(n) % 2 == 0)).any()                              # trans rows that pass the threshold
        s = P.check_split("0.05", "All")
        assert s.chromosomes == ["chr1", "chr2", "chr3"] and s.n_kept("chr3") == 0 and s.subset_text("chr3") == b""
        t = P.check_track("0.05", "All")                                            # the track takes trans rows
        assert t.n_kept == s.n_kept("chr1") + s.n_kept("chr2") + int((trans & (np.arange(n) % 2 == 0)).sum())


def _many_names_source(extra):
    """`extra` more chromosomes of 40 bins behind the two of the synthetic set, each with one row of an in-range distance"""
    k = np.arange(extra)
    delta = 6 + k % 31
    rows = [k + 2, np.full(extra, RES // 2), k + 2, delta * RES + RES // 2, np.maximum(1, 40 // delta) + k % 3]
    return _extended(["chr%d" % (i + 3) for i in range(extra)], [40] * extra, rows)


def test_split_takes_4096_names_and_refuses_4097():
    """FHX_MS_SPLIT_NAMES listed names (the header's chr1 is the first chromosome's name) are accepted, one more is refused without
    a line, as the file route does it.  The chromosomes have 40 bins and not two: a row is listed when the writer prints it, so its
    distance has to lie in the run's range."""
    from fithic_amd import _capi, mergefilter_parallel
    src = _many_names_source(_capi.MS_SPLIT_NAMES - 1)
    assert len(src.names) == _capi.MS_SPLIT_NAMES + 1
    n = len(src.cols[0])
    with Pass(n - 1, real=True, src=src) as P:                                       # without the row of the last chromosome
        assert P.emit[DONOR_ROWS:].all()
        P.write_q(np.where(np.arange(n - 1) % 2 == 0, KEEP, DROP))
        s = P.check_split("0.05", "4096 names")
        assert len(s.chromosomes) == _capi.MS_SPLIT_NAMES and s.chromosomes == sorted(src.names[:-1])
    with Pass(n, real=True, src=src) as P:
        P.write_q(np.where(np.arange(n) % 2 == 0, KEEP, DROP))
        with pytest.raises(ValueError) as e:
            P.split("0.05")
        assert not isinstance(e.value, _capi.FhxError) and str(e.value) == str(mergefilter_parallel._refusal_names("pass.gz"))
        with pytest.raises(mm.Refused) as m:
            sm.split(P.file(), "0.05")
        assert (m.value.why, m.value.line) == (sm.NAMES, 0)
        assert P.eng.ctx.significant_split_parts(0) == []


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
def _raises_like_the_model(P, model, call, builder, names=None):
    """the direct route raises the file route's ValueError for the reason and the line the model gives for the same file"""
    from fithic_amd import _capi
    with pytest.raises(mm.Refused) as m:
        model(P.file(names), "0.05")
    with pytest.raises(ValueError) as e:
        call("0.05", names)
    want = builder("pass.gz, line %d" % m.value.line, m.value.why, "")
    assert not isinstance(e.value, _capi.FhxError) and str(e.value) == str(want), (m.value.why, m.value.line, str(e.value))
    return m.value.why, m.value.line


def test_a_q_outside_the_grammar_names_its_line():
    from fithic_amd import _capi, mergefilter_parallel, ucsc
    n = 2000
    with Pass(n) as P:
        em, off = P.emitted, np.flatnonzero(~P.emit)
        base = np.where(np.arange(n) % 3 == 0, KEEP, DROP)
        early, late = int(em[len(em) // 3]), int(em[-2])              # in different workgroups, non-emitted rows before both
        assert early // 256 != late // 256 and P.line_of(early) < early + 2
        for bad in (float("nan"), -1e-3, 1e308):
            for row in (early, late):
                q = base.copy()
                q[row] = bad
                P.write_q(q)
                assert _raises_like_the_model(P, um.track, P.track, ucsc._refusal_at) == (um.FIELD, P.line_of(row))
                assert _raises_like_the_model(P, sm.split, P.split, mergefilter_parallel._refusal_at) == (mm.FIELD, P.line_of(row))
        # the same fault on rows the writer does not print is no refusal
        q = base.copy()
        q[off] = float("nan")
        P.write_q(q)
        good = P.check_track("0.05", "nan on rows that are not emitted")
        parts = P.check_split("0.05", "nan on rows that are not emitted")
        assert good.n_kept > 0
        # after a refusal the copy calls return nothing
        q[early] = float("nan")
        P.write_q(q)
        with pytest.raises(ValueError):
            P.track("0.05")
        with pytest.raises(ValueError):
            P.split("0.05")
        text = np.full(len(good.text()), 0x55, np.uint8)
        L, h = P.eng.ctx._L, P.eng.ctx._h
        assert L.fhx_significant_copy_track(h, text.ctypes.data, len(text)) == _capi.FHX_OK and (text == 0x55).all()
        assert P.eng.ctx.significant_track_text(0) == b"" and P.eng.ctx.significant_split_parts(0) == []
        assert L.fhx_significant_copy_split(h, 0, text.ctypes.data, len(text)) == _capi.FHX_ERR_ARG
        # a refused track leaves a split alone, and the other way round
        q[early] = KEEP
        P.write_q(q)
        parts = P.split("0.05")
        q[early] = float("nan")
        P.write_q(q)
        with pytest.raises(ValueError):
            P.track("0.05")
        kept = P.eng.ctx.significant_split_parts(len(parts.chromosomes))
        assert [(name.decode(), rows) for name, rows, _ in kept] == [(c, parts.n_kept(c)) for c in parts.chromosomes]
        assert all(text == parts.subset_text(name) for name, _, text in kept)


def _big_midpoint_source():
    """a third chromosome whose bins have their midpoints at multiples of RES, with a row that ends on midpoint 1 000 000 000"""
    bins = 1000000000 // RES + 2
    rows = [[2, 2], [1000000000 - 7 * RES, 10 * RES], [2, 2], [1000000000, 17 * RES], [3, 4]]
    return _extended(["chr3"], [bins], rows, offsets=[0])


def test_track_refuses_a_ten_digit_midpoint_on_a_dropped_row():
    from fithic_amd import mergefilter_parallel, ucsc
    src = _big_midpoint_source()
    n = len(src.cols[0])
    with Pass(n, real=True, src=src) as P:
        big = n - 2
        assert P.cols[3][big] == 1000000000 and P.emit[big] and P.emit[big + 1]
        q = np.where(np.arange(n) % 3 == 0, KEEP, DROP)
        q[big] = DROP                                                  # emitted, dropped: the file route checks every parsed line
        P.write_q(q)
        assert _raises_like_the_model(P, um.track, P.track, ucsc._refusal_at) == (um.MIDPOINT, P.line_of(big))
        P.check_split("0.05", "the split has no rule for midpoints")
        # two faults on one line: field 7 comes before the midpoint (fhx_sigtrack.inc, ut_select: refusal(cls, midpoints, names))
        q[big] = float("nan")
        P.write_q(q)
        assert _raises_like_the_model(P, um.track, P.track, ucsc._refusal_at) == (um.FIELD, P.line_of(big))
        # the same midpoint on a row the writer does not print is no refusal
        q[big] = KEEP
        P.write_q(q)
    far = [c.copy() for c in src.cols]
    far[1][n - 2] = 1000000000 - 40 * RES                              # 40 bins: outside the run's distances
    other = Source(src.names, src.frag_chr, src.frag_mid, src.bias, far)
    with Pass(n, real=True, src=other) as P:
        assert not P.emit[n - 2] and P.cols[3][n - 2] == 1000000000
        P.write_q(np.where(np.arange(n) % 3 == 0, KEEP, DROP))
        assert P.check_track("0.05", "a ten-digit midpoint that is not emitted").n_kept > 0


def test_name_rules_of_the_track_and_of_the_split():
    from fithic_amd import mergefilter_parallel, ucsc
    n = 1500
    with Pass(n) as P:
        on2 = P.cols[0] == 1
        first2 = int(np.flatnonzero(on2 & P.emit)[0])
        P.write_q(np.where(on2, DROP, KEEP))                           # the rows of the second name are emitted and dropped
        # the track: 64 bytes are refused on a dropped row; 63 are taken there, and unsupported once such a row is kept
        long64 = ["chr1", "c" * 64]
        assert _raises_like_the_model(P, um.track, P.track, ucsc._refusal_at, long64) == (um.NAME, P.line_of(first2))
        assert _raises_like_the_model(P, sm.split, P.split, mergefilter_parallel._refusal_at, long64) == (sm.NAME, P.line_of(first2))
        long63 = ["chr1", "c" * 63]
        t = P.check_track("0.05", "63 bytes on dropped rows", names=long63)
        assert t.n_kept == int((~on2 & P.emit).sum()) > 0
        s = P.check_split("0.05", "63 bytes on dropped rows", names=long63)
        assert s.chromosomes == ["c" * 63, "chr1"] and s.n_kept("c" * 63) == 0
        # the split: names awk might compare as numbers, and bytes a shell word does not take
        for bad, why in (("01", sm.NAME_NUMERIC), ("1.5", sm.NAME_NUMERIC), ("2a", sm.NAME_NUMERIC), ("chr+2", sm.NAME_BYTES)):
            names = ["chr1", bad]
            assert _raises_like_the_model(P, sm.split, P.split, mergefilter_parallel._refusal_at, names) == (why, P.line_of(first2)), bad
            P.check_track("0.05", ("the track takes the name", bad), names=names)
        # two faults on one line: the split reports the name before field 7, the track field 7 before the name
        q = np.where(on2, DROP, KEEP)
        q[first2] = float("nan")
        P.write_q(q)
        assert _raises_like_the_model(P, sm.split, P.split, mergefilter_parallel._refusal_at, ["chr1", "2a"]) == (sm.NAME_NUMERIC, P.line_of(first2))
        assert _raises_like_the_model(P, um.track, P.track, ucsc._refusal_at, long64) == (um.FIELD, P.line_of(first2))


def test_a_refused_name_on_rows_the_writer_does_not_print_is_no_refusal():
    """a third chromosome whose only row lies outside the run's distances: whatever its name, it is neither refused nor listed"""
    src = _extended(["2a"], [100], [[2], [RES // 2], [2], [50 * RES + RES // 2], [3]])
    n = len(src.cols[0])
    with Pass(n, real=True, src=src) as P:
        assert not P.emit[n - 1] and P.cols[0][n - 1] == 2
        P.write_q(np.where(np.arange(n) % 3 == 0, KEEP, DROP))
        s = P.check_split("0.05", "2a is not emitted")
        assert s.chromosomes == ["chr1", "chr2"]
        t = P.check_track("0.05", "64 bytes are not emitted", names=["chr1", "chr2", "c" * 64])
        assert t.n_kept > 0


def test_a_kept_row_with_a_long_name_is_unsupported():
    from fithic_amd import _capi
    n = 1500
    with Pass(n) as P:
        names = [P.names[0], "c" * 25]
        on_long = P.cols[0] == 1
        P.write_q(np.where(on_long, DROP, KEEP))                       # the rows with the 25-byte name are dropped: no text is made of them
        t = P.check_track("0.05", "25 bytes on dropped rows", names=names)
        s = P.check_split("0.05", "25 bytes on dropped rows", names=names)
        assert t.n_kept == s.n_kept("chr1") == int((~on_long & P.emit).sum()) > 0
        q = np.where(on_long, DROP, KEEP)
        q[np.flatnonzero(on_long & P.emit)[-1]] = KEEP                 # one of them kept
        P.write_q(q)
        for call in (P.track, P.split):
            with pytest.raises(_capi.FhxError) as e:
                call("0.05", names)
            assert e.value.code == _capi.FHX_ERR_UNSUPPORTED and not isinstance(e.value, _capi.MsRefused)
        assert P.eng.ctx.significant_track_text(0) == b"" and P.eng.ctx.significant_split_parts(0) == []
        assert P.track("0.05").n_kept == t.n_kept + 1                  # the short names: the same rows are fine


def test_only_between_bh_and_next_pass():
    from fithic_amd import _capi
    n = 600
    with Pass(n) as P:
        assert P.track("0.05").n_lines == len(P.emitted) + 1 == P.split("0.05").n_lines
        P.eng.next_pass()
        for call in (P.track, P.split):
            with pytest.raises(_capi.FhxError) as e:
                call("0.05")
            assert e.value.code == _capi.FHX_ERR_ARG
        P.eng.pass_stats()                                             # the next pass has begun: no q yet
        for call in (P.track, P.split):
            with pytest.raises(_capi.FhxError) as e:
                call("0.05")
            assert e.value.code == _capi.FHX_ERR_ARG
    host = _capi.Context(-1)                                           # a host-only context
    try:
        for call in (host.significant_track, host.significant_split):
            with pytest.raises(_capi.FhxError) as e:
                call(["chr1"], b"0.05", 0, True)
            assert e.value.code == _capi.FHX_ERR_NO_DEVICE
    finally:
        host.close()


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------------------------
def test_the_same_selection_twice_gives_the_same_bytes():
    n = 3 * 4096 + 77
    vals = _kept_values()
    with Pass(n) as P:
        P.write_q(np.where(np.arange(n) % 3 != 0, vals[np.arange(n) % len(vals)], DROP))
        a, b = P.track("0.05"), P.track("0.05")
        _same_track(a, b, "twice")
        assert a.n_kept > 4096 and a.n_deferred > 0
        c, d = P.split("0.05"), P.split("0.05")
        _same_split(c, d, "twice")
        assert all(c.n_kept(name) > 0 for name in P.names)
        _same_track(P.track("0.05"), a, "after a split")
