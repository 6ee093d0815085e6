"""Who owns device memory (csrc/fhx_devmem.hpp), seen through fhx_debug_device_blocks: the live device blocks of the process and
their bytes.  Every test compares two readings taken in this process - other fixtures may hold contexts, so no absolute value
means anything: a handle that is created, used once and closed gives back all it took; a call that refuses its input three times
in a row holds no more after the third refusal than after the second, and a good call still works; the K2 hooks hold nothing once
they have returned; a text path whose second batch is larger than its first (DeviceScratch::grow reallocates) and the Knight-Ruiz
vectors regrown for larger matrices end where they started.  The inputs are the smallest the tests of each path already use."""
import os

import numpy as np
import pytest

import juicer_model as jm
import mergefilter_model as mm
import validpairs_model as vm
from batch_env import batch_bytes
from test_gpu_hicpro import _device as hp_parse_once
from test_gpu_juicer import model_bytes as jc_model_bytes
from test_gpu_mergefilter import DROPPED, HEADER, KEPT, row, third_batch_texts

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")


def _blocks():
    from fithic_amd import _capi
    return _capi.device_blocks()                 # (live blocks, live bytes) of this process


def _write(path, data):
    with open(str(path), "wb") as f:
        f.write(data)
    return str(path)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- the texts of the existing "refusal in the third batch" tests, at 8192 bytes a batch ------------------------------------------
def vp_texts():
    rows = [b"r\tchr%d\t%d\t+\tchr%d\t%d\t-\n" % (1 + k % 3, 1000 * k, 1 + k % 2, 700 * k + 5) for k in range(900)]
    good, bad = b"".join(rows), b"".join(rows[:700]) + b"r chr1 5 + chr2\n" + b"".join(rows[700:])
    assert 2 * 8192 < len(b"".join(rows[:700])) and len(bad) < 4 * 8192
    return good, bad


def jc_texts():
    rows = [b"%d\t%d\t%d\n" % (5000 * (k % 97), 5000 * (k % 89 + 100), 1 + k % 50) for k in range(1500)]
    good, bad = b"".join(rows), b"".join(rows[:1300]) + b"5000 10000\n" + b"".join(rows[1300:])
    assert 2 * 8192 < len(b"".join(rows[:1300])) and len(bad) < 4 * 8192
    return good, bad


def _ms_select(ms, path):
    from fithic_amd import mergefilter as mf
    return ms.select_file(path, b"0.05", mf.key_bound("0.05"), True)


def _smoke_engine():
    """an Engine with the smallest golden contacts set loaded, one pass run"""
    from fithic_amd import tables
    from fithic_amd.engine import Engine
    chroms = tables.ChromIndex()
    con = tables.read_contacts(os.path.join(DATA, "quirk.contacts.gz"), chroms)
    fc, fm, fh = tables.read_fragments(os.path.join(DATA, "quirk.frags.gz"), chroms)
    eng = Engine(0)
    eng.configure(10000, 20000, 400000, 12, 1, "All")
    eng.load_fragments(fc, fm, fh, chroms.sort_rank())
    eng.load_contacts(con.chr1, con.mid1, con.chr2, con.mid2, con.count)
    eng.run_pass()
    assert len(eng.fetch()["p"]) == len(con)
    return eng


# ---- 1. create, one small call, close ---------------------------------------------------------------------------------------------
def _open_use_close(kind, tmp_path):
    from fithic_amd import _capi
    if kind == "ctx":
        _smoke_engine().close()
    elif kind == "kr":
        kr = _capi.KrContext(0)
        kr.load_loci([0, 0, 0], [5, 15, 25])
        kr.load_pairs([0, 0, 0, 0], [5, 5, 15, 25], [0, 0, 0, 0], [15, 15, 15, 5], [1.5, 2.25, 4.0, 8.0])
        assert kr.get_csr(0)[2].sum() == 2 * (3.75 + 8.0) + 8.0
        kr.close()
    elif kind == "cni":
        cn = _capi.CniContext(0)
        cn.load([0, 0], [40000, 80000], [80000, 120000], [5, 6], [1e-3, 1e-4], [1e-2, 1e-3], 40000)
        assert len(cn.run(8, 100, 2, 0)[0]) == 1
        cn.close()
    elif kind == "hp":
        import hicpro_model as hm
        cols, _ = hp_parse_once(hm.fixture_bytes("hp2.bed.gz"), b"3\t4\t5\n", tmp_path)      # creates, parses, fetches, closes
        assert all(len(c) == 1 for c in cols)
    elif kind == "vp":
        vp = _capi.VpContext(0)
        assert vp.bin_file(_write(tmp_path / "one.validPairs", b"r\tchr1\t5\t+\tchr2\t9\t-\n" * 3), 10000) == 1
        vp.close()
    elif kind == "ms":
        ms = _capi.MsContext(0)
        data = HEADER + row(1, KEPT) + row(2, DROPPED) + row(3, KEPT)
        assert _ms_select(ms, _write(tmp_path / "sig.txt", data)) == len(mm.select(data, "0.05"))
        ms.close()
    else:
        jc = _capi.JcContext(0)
        assert jc.convert_file(_write(tmp_path / "dump.txt", b"5000\t10000\t3\n10000\t15000\t1\n"), "chr1", "chrX", 5000) == 2
        jc.close()


@pytest.mark.parametrize("kind", ["ctx", "kr", "cni", "hp", "vp", "ms", "jc"])
def test_create_use_close_returns_to_the_start(kind, tmp_path):
    before = _blocks()
    _open_use_close(kind, tmp_path)
    assert _blocks() == before


# ---- 2. a refused call leaves nothing behind ----------------------------------------------------------------------------------------
def _refused_three_times(refused_call):
    """the readings after the second and after the third of three refusals in a row"""
    seen = []
    for _ in range(3):
        refused_call()
        seen.append(_blocks())
    return seen[1], seen[2]


def test_kr_unknown_locus_refusals_hold_nothing():
    from fithic_amd import _capi
    kr = _capi.KrContext(0)
    try:
        kr.load_loci([0, 0, 0, 0], [5, 15, 5, 25])

        def refused():
            with pytest.raises(KeyError):
                kr.load_pairs([0, 0], [5, 15], [0, 0], [15, 35], [1.0, 2.0])
        second, third = _refused_three_times(refused)
        assert second == third
        kr.load_pairs([0, 0, 0, 0], [5, 5, 15, 25], [0, 0, 0, 0], [15, 15, 15, 5], [1.5, 2.25, 4.0, 8.0])
        indptr, col, val = kr.get_csr(0)
        dense = np.zeros((4, 4))
        for r in range(4):
            dense[r, col[indptr[r]:indptr[r + 1]]] = val[indptr[r]:indptr[r + 1]]
        want = np.zeros((4, 4))
        want[2, 1] = want[1, 2] = 3.75
        want[1, 1] = 8.0
        want[3, 2] = want[2, 3] = 8.0
        assert np.array_equal(dense, want)
    finally:
        kr.close()


def test_kr_resident_unknown_locus_refusals_hold_nothing():
    from fithic_amd import _capi
    from fithic_amd.engine import Engine
    n = 200
    rng = np.random.default_rng(4)
    a, b = rng.integers(0, 50, n), rng.integers(0, 50, n)
    a[[40, 130]] = 60                                  # locus 60 is no fragment line of the first load_loci
    zeros, cnt = np.zeros(n, np.int32), rng.integers(1, 9, n).astype(np.int32)
    eng, kr, by_file = Engine(0), _capi.KrContext(0), _capi.KrContext(0)
    try:
        eng.configure(1000)
        eng.load_contacts(zeros, a * 1000 + 500, zeros, b * 1000 + 500, cnt)
        kr.load_loci(np.zeros(50, np.int32), np.arange(50) * 1000 + 500)

        def refused():
            with pytest.raises(KeyError) as e:
                kr.load_pairs_resident(eng.ctx)
            assert e.value.args == (40,)
        second, third = _refused_three_times(refused)
        assert second == third
        loci = (np.zeros(61, np.int32), np.arange(61) * 1000 + 500)
        kr.load_loci(*loci)
        kr.load_pairs_resident(eng.ctx)
        by_file.load_loci(*loci)
        by_file.load_pairs(zeros, a * 1000 + 500, zeros, b * 1000 + 500, cnt.astype(np.float64))
        for got, want in zip(kr.get_csr(0), by_file.get_csr(0)):
            assert np.array_equal(got, want)
    finally:
        kr.close()
        by_file.close()
        eng.close()


def test_cni_off_lattice_refusals_hold_nothing():
    from fithic_amd import _capi
    cn = _capi.CniContext(0)
    try:
        def refused():
            with pytest.raises(_capi.FhxError):
                cn.load([0, 0], [40000, 60001], [80000, 120000], [5, 6], [1e-3, 1e-4], [1e-2, 1e-3], 40000)
        second, third = _refused_three_times(refused)
        assert second == third
        cn.load([0, 0], [40000, 80000], [80000, 120000], [5, 6], [1e-3, 1e-4], [1e-2, 1e-3], 40000)
        rec, info = cn.run(8, 100, 2, 0)
        assert info.nodes == 2 and info.components == 1 and len(rec) == 1 and rec[0]["q"] == 1e-3
    finally:
        cn.close()


def test_vp_third_batch_refusals_hold_nothing(tmp_path):
    from fithic_amd import _capi
    good, bad = vp_texts()
    good_path, bad_path = _write(tmp_path / "good.validPairs", good), _write(tmp_path / "bad.validPairs", bad)
    vp = _capi.VpContext(0)
    try:
        with batch_bytes("FHX_VP_BATCH_BYTES", 8192):
            def refused():
                with pytest.raises(_capi.VpRefused) as e:
                    vp.bin_file(bad_path, 10000)
                assert (e.value.why, e.value.line) == (vm.TOKENS, 701)
            second, third = _refused_three_times(refused)
            assert second == third
            names, *cols = vm.columns(good, 10000)
            assert vp.bin_file(good_path, 10000) == len(cols[0])
        assert vp.names() == names
        for g, w in zip(vp.fetch_cells(), cols):
            assert np.array_equal(g, np.asarray(w, np.int32))
    finally:
        vp.close()


def test_jc_third_batch_refusals_hold_nothing(tmp_path):
    from fithic_amd import _capi
    good, bad = jc_texts()
    good_path, bad_path = _write(tmp_path / "good.txt", good), _write(tmp_path / "bad.txt", bad)
    jc = _capi.JcContext(0)
    try:
        with batch_bytes("FHX_JC_BATCH_BYTES", 8192):
            def refused():
                with pytest.raises(_capi.JcRefused) as e:
                    jc.convert_file(bad_path, "chr1", "chrX", 5000, keep_rows=True)
                assert (e.value.why, e.value.line) == (jm.TOKENS, 1301)
            second, third = _refused_three_times(refused)
            assert second == third
            assert jc.convert_file(good_path, "chr1", "chrX", 5000, keep_rows=True) == 1500
        want = jc_model_bytes(good, 5000, "1", "X")
        assert jc.text() == want and jc.counts() == dict(lines=1500, rows=1500, bytes=len(want))
    finally:
        jc.close()


def test_ms_third_batch_refusals_hold_nothing(tmp_path):
    from fithic_amd import _capi
    good, bad = third_batch_texts()
    good_path, bad_path = _write(tmp_path / "good.txt", good), _write(tmp_path / "bad.txt", bad)
    ms = _capi.MsContext(0)
    try:
        with batch_bytes("FHX_MS_BATCH_BYTES", 8192):
            def refused():
                with pytest.raises(_capi.MsRefused) as e:
                    _ms_select(ms, bad_path)
                assert (e.value.why, e.value.line) == (mm.TOKENS, 252)
            second, third = _refused_three_times(refused)
            assert second == third
            want = mm.select(good, "0.05")
            assert _ms_select(ms, good_path) == len(want)
        assert ms.subset() == want and ms.counts() == dict(lines=301, kept=200, bytes=len(want))
    finally:
        ms.close()


# ---- 3. the K2 hooks hold nothing after they return ---------------------------------------------------------------------------------
def test_k2_hooks_hold_nothing_after_they_return():
    from fithic_amd import _capi
    count = np.array([1, 2, 3, 5, 8, 40, 300, 2000], np.int32)
    prior = np.array([0.5, 1e-3, 1e-6, 0.02, 1e-4, 3e-5, 2e-4, 1e-3])
    x = np.linspace(0.05, 0.9, 8)
    start = _blocks()
    ctx = _capi.Context(0)
    assert _blocks()[0] > start[0] and _blocks()[1] > start[1]       # the counters move: a context holds its device words
    hooks = {"bdtrc_array": lambda: ctx.bdtrc_array(1.0e6, count, prior),
             "debug_contfrac": lambda: ctx.debug_contfrac(0, 0, count.astype(np.float64), count + 7.0, x),
             "debug_lean_div": lambda: ctx.debug_lean_div(prior, x),
             "debug_table_div": lambda: ctx.debug_table_div(0, x),
             "debug_classify": lambda: ctx.debug_classify(1.0e6, count, prior, thresholds=True),
             "debug_k2_rows": lambda: ctx.debug_k2_rows(1.0e6, 2.0e6, count, prior, np.arange(8) % 2 == 1)}
    try:
        for name, call in hooks.items():
            call()                                     # the first call may make tables that live as long as the context
            before = _blocks()
            call()
            assert _blocks() == before, name
        # what the hooks compute is checked where they are used; here only that the entry and the pass still agree
        p = ctx.debug_k2_rows(1.0e6, 2.0e6, count, prior, np.zeros(8, np.uint8))[0]
        assert np.array_equal(_bits(p), _bits(ctx.bdtrc_array(1.0e6, count, prior)))
    finally:
        ctx.close()
    assert _blocks() == start


# ---- 4. DeviceScratch::grow and drop as the text paths use them ---------------------------------------------------------------------
def test_a_second_batch_larger_than_the_first_leaves_nothing(tmp_path):
    """The first 8192-byte batch holds ~25 long lines, the later ones ~100 short lines each: the per-line arrays of the call grow
    (the old block dropped, a larger one taken) in the second batch."""
    from fithic_amd import _capi
    long_rows = b"".join(row(k, KEPT if k % 2 else DROPPED, pad=250) for k in range(30))
    data = HEADER + long_rows + b"".join(row(k, KEPT if k % 3 else DROPPED) for k in range(300))
    first = (HEADER + long_rows)[:8192]
    assert len(HEADER + long_rows) > 8192 and first.count(b"\n") < 30 < data[8192:2 * 8192].count(b"\n")
    path = _write(tmp_path / "sig.txt", data)
    want = mm.select(data, "0.05")
    ms = _capi.MsContext(0)
    try:
        with batch_bytes("FHX_MS_BATCH_BYTES", 8192):
            assert _ms_select(ms, path) == len(want)   # warms the handle: the pinned pair, the kept subset
            before = _blocks()
            assert _ms_select(ms, path) == len(want)
            assert _blocks() == before
        assert ms.subset() == want
    finally:
        ms.close()


# ---- 5. the Knight-Ruiz vectors regrown ---------------------------------------------------------------------------------------------
def test_kr_vectors_regrown_for_larger_matrices_are_all_given_back():
    """spmv and dot on n = 5, then 300 (the ten vectors regrow), then 1500 (two reduction tiles of 1024: the partial arrays regrow
    too); every result equals the oracle's bit for bit, and close gives everything back."""
    from fithic_amd import _capi
    from oracle import hickry_oracle as ho
    rng = np.random.default_rng(5)
    before = _blocks()
    kr = _capi.KrContext(0)
    try:
        for n in (5, 300, 1500):
            m = 8 * n
            x = rng.integers(0, n, m)
            y = np.clip(x + rng.geometric(0.3, m) - 1, 0, n - 1)
            z = rng.integers(1, 50, m).astype(np.float64) + rng.integers(0, 2, m) * 0.25
            A = ho.assemble(x.astype(np.int64), y.astype(np.int64), z, n)
            kr.load_loci(np.zeros(n, np.int32), np.arange(n, dtype=np.int32))
            zeros = np.zeros(m, np.int32)
            kr.load_pairs(zeros, x.astype(np.int32), zeros, y.astype(np.int32), z)
            v, w = rng.lognormal(0, 1, n), rng.normal(0, 1, n)
            assert np.array_equal(_bits(kr.spmv(v)[0]), _bits(A.dot(v))), n
            assert kr.dot(v, w) == ho.dot(v, w) and kr.dot(v) == ho.dot(v), n
    finally:
        kr.close()
    assert _blocks() == before
