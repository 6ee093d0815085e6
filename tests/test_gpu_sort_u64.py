"""fhx_sort_u64 - the one stable u64 sort behind the Knight-Ruiz cell assembly, the nearby-contact merging, validPairs binning and
both per-chromosome FDR splits - against numpy's stable argsort.  A stable ascending sort has exactly one answer, so the
permutation is compared element for element; nothing here has a tolerance.

Sizes and key patterns: tests/sort_keys.py (checked without a GPU by tests/test_sort_u64_inputs.py)."""
import numpy as np
import pytest

from sort_keys import CASES, M20, make_keys

pytestmark = pytest.mark.gpu


def sort_on(ctx, keys):
    """-> (sorted keys, perm, the input buffer read back) as numpy arrays; keys: uint64"""
    import torch
    t = torch.from_numpy(keys.view(np.int64).copy()).to("cuda:0")
    out = torch.full_like(t, 0x1234567)
    perm = torch.full((len(keys),), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.sort_u64(t.data_ptr(), len(keys), out.data_ptr(), perm.data_ptr())
    return out.cpu().numpy().view(np.uint64), perm.cpu().numpy().view(np.uint32), t.cpu().numpy().view(np.uint64)


def check_sort(ctx, keys, what):
    got_keys, got_perm, after = sort_on(ctx, keys)
    want_perm = np.argsort(keys, kind="stable")
    assert np.array_equal(after, keys), (what, "the input was written")
    if not np.array_equal(got_perm, want_perm):
        bad = np.flatnonzero(got_perm != want_perm)
        r = int(bad[0])
        raise AssertionError("%s: perm differs at %d places, first at %d (tile %d, offset %d): got row %d, want row %d" % (
            what, len(bad), r, r // 4096, r % 4096, int(got_perm[r]), int(want_perm[r])))
    assert np.array_equal(got_keys, keys[want_perm]), (what, "keys")


@pytest.fixture(scope="module")
def ctx():
    from fithic_amd import _capi
    c = _capi.Context(0)                                          # raises without a GPU or the library: no fallback
    yield c
    c.close()


@pytest.mark.parametrize("pattern,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_sort_equals_the_stable_argsort(ctx, pattern, n):
    keys = make_keys(pattern, n)
    if pattern in ("all_zero", "all_ones", "ascending"):
        assert np.array_equal(np.argsort(keys, kind="stable"), np.arange(n))       # perm must be the identity
    check_sort(ctx, keys, (pattern, n))


def test_smaller_sorts_after_a_larger_one_on_one_context():
    """the device counter and the count matrix of the larger sort (128 workgroups, two tiles per chunk) must not leak into the
    smaller ones that follow on the same context"""
    from fithic_amd import _capi
    c = _capi.Context(0)
    try:
        for n in (M20 + 1, 4097, 1, 262145):
            for pattern in ("random64", "eight_bits0_10"):
                check_sort(c, make_keys(pattern, n), ("reuse", pattern, n))
    finally:
        c.close()


def test_boundaries_of_the_call():
    import torch
    from fithic_amd import _capi
    c = _capi.Context(0)
    try:
        c.sort_u64(0, 0, 0, 0)                                    # n = 0 with null pointers: OK, nothing touched
        small = [torch.zeros(8, dtype=torch.int64, device="cuda:0") for _ in range(3)]
        torch.cuda.synchronize()
        with pytest.raises(_capi.FhxError) as err:                # refused before any device work (fhx_k3.hip, fhx_sort_u64)
            c.sort_u64(small[0].data_ptr(), 1 << 32, small[1].data_ptr(), small[2].data_ptr())
        assert err.value.code == _capi.FHX_ERR_UNSUPPORTED
        assert all(int(t.abs().sum()) == 0 for t in small)
        check_sort(c, make_keys("random64", 4097), "after the refusal")
    finally:
        c.close()


def _engine(name):
    from conftest import load_case, case_args
    from fithic_amd import tables
    from fithic_amd.engine import Engine
    meta, _ = load_case(name)
    kw = case_args(meta)
    chroms = tables.ChromIndex()
    con = tables.read_contacts(kw["contacts"], chroms)
    eng = Engine(0)
    eng.configure(kw["resolution"], kw["L"], kw["U"], kw["n_bins"], kw["mapp_thres"], kw["mode"], kw["tL"], kw["tU"])
    eng.load_fragments(*tables.read_fragments(kw["frags"], chroms), chroms.sort_rank())
    if kw["bias_path"]:
        eng.load_bias(*tables.read_bias(kw["bias_path"], chroms))
    eng.load_contacts(con.chr1, con.mid1, con.chr2, con.mid2, con.count)
    return eng


def _pass_steps(eng, between):
    """pass_stats, fit, pvalues, bh - twice, because only a context's second pass_stats zeroes K2's histograms ahead (k2_prezeroed) -
    with between() after pass_stats and after pvalues -> [(p bits, q bits, class rows)] of both rounds"""
    out = []
    for _ in range(2):
        eng.ctx.pass_stats()
        between()
        info = eng.ctx.fit()
        eng.ctx.pvalues()
        classes = eng.ctx.k2_class_rows()
        between()
        eng.ctx.bh(info.bh_total_tests)
        v = eng.fetch()
        out.append((v["p"].view(np.int64).copy(), v["q"].view(np.int64).copy(), classes))
    return out


@pytest.mark.parametrize("name", ["f2_all", "f6_quirk_all"])
def test_a_sort_between_the_steps_of_a_pass_changes_nothing(name):
    """radix_passes shares the count matrix with K2's heavy-class histogram and clears the context's k2_prezeroed mark: a sort of
    5000 keys on the pass's own context after pass_stats() and after pvalues() must leave p, q and the class rows as they are"""
    plain = _engine(name)
    try:
        want = _pass_steps(plain, lambda: None)
    finally:
        plain.close()
    assert sum(want[0][2].values()) > 0
    eng = _engine(name)
    try:
        seeds = iter(range(100))
        got = _pass_steps(eng, lambda: check_sort(eng.ctx, make_keys("random64", 5000, next(seeds)), "between the steps"))
    finally:
        eng.close()
    for round_no, (w, g) in enumerate(zip(want, got)):
        assert np.array_equal(w[0], g[0]), (name, round_no, "p")
        assert np.array_equal(w[1], g[1]), (name, round_no, "q")
        assert w[2] == g[2], (name, round_no, "k2_class_rows")
