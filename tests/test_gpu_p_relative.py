"""K2's p-values held to the relative bar of tests/p_relative.py on the chosen rows of tests/golden/f16_bdtrc_tail.npz: every
outcome of k2_classify in every band of p down to the subnormal range and the reference's 0, where the absolute bar of 1e-10 accepts
anything.  Context.bdtrc_array (one lane per row through bdtrc_count -> incbet) and the pass kernels through the fhx_debug_k2_rows
hook, in a default context (the five totals below 2^31) and in a TOTALS_WIDE one (all six).  tests/test_p_relative_inputs.py checks
the fixture and the helper without a GPU.

The device is run once per context (the `device` fixture); the tests only compare.

Measured on an MI355X, default context (bdtrc_array and both hook variants give the same bits; the wide context adds the sixth
total and shows the same picture) - rows, share bit-identical to the oracle, largest |got - o| / bar:

    outcome       band of p          rows  bit-identical    max |got-o|/bar
    pseries       >=1e-10             100         96.00%              0.157
    pseries       1e-40..1e-10         90         93.33%              0.118
    pseries       1e-150..1e-40        90         90.00%              0.121
    pseries       normal<1e-150        90         86.67%              0.125
    pseries       subnormal            90        100.00%                  0
    pseries       zero                 91        100.00%                  0
    cf_bcf        >=1e-10              90         82.22%              0.234
    cf_bcf        1e-40..1e-10         90         83.33%              0.276
    cf_bcf        1e-150..1e-40       110         88.18%              0.265
    cf_bcf        normal<1e-150        90         85.56%              0.211
    cf_bcf        subnormal            54         98.15%            0.00132
    cf_bcf        zero                 65        100.00%                  0
    cf_bd         >=1e-10              90         90.00%              0.185
    cf_swapped    >=1e-10              90         94.44%              0.243
    closed_pow    >=1e-10              90        100.00%                  0
    closed_local  >=1e-10             104         99.04%              0.156
    closed_local  1e-40..1e-10        100        100.00%                  0
    closed_local  1e-150..1e-40        90        100.00%                  0
    closed_local  normal<1e-150        90        100.00%                  0
    closed_local  subnormal            90        100.00%                  0
    all           all                1813         94.26%              0.276"""
import numpy as np
import pytest

import k2_rows as kr
import p_relative as pr
from conftest import bits_equal

pytestmark = pytest.mark.gpu

MODES = ("reference", "wide")


def _pairs(totals):
    """(intra, inter) as k2_rows.BOUNDARY_PAIRS: each total once on each side"""
    return tuple(zip(totals, totals[2:] + totals[:2]))


def _run(c, cols, totals):
    """per fixture row: lane = bdtrc_array, (side, nonfixed) = the hook's p with the row's total as that binomial; NaN-filled
    where the context does not run the row (`ran`)"""
    n = len(cols["count"])
    out = {"lane": np.full(n, np.nan), "ran": np.zeros(n, bool), "classes": []}
    for side in ("intra", "inter"):
        for nonfixed in (False, True):
            out[(side, nonfixed)] = np.full(n, np.nan)
    for n_intra, n_inter in _pairs(totals):
        ii, ie = np.flatnonzero(cols["total"] == n_intra), np.flatnonzero(cols["total"] == n_inter)
        r = kr.two_sided(n_intra, (cols["count"][ii], cols["prior"][ii]), n_inter, (cols["count"][ie], cols["prior"][ie]))
        for nonfixed in (False, True):
            p, by_class, _, _ = c.debug_k2_rows(r.n_intra, r.n_inter, r.count, r.prior, r.is_inter, nonfixed=nonfixed)
            out[("intra", nonfixed)][ii], out[("inter", nonfixed)][ie] = p[:len(ii)], p[len(ii):]
            out["classes"].append(((n_intra, n_inter, nonfixed), by_class, kr.class_rows(r.outcomes())))
        out["lane"][ii] = c.bdtrc_array(n_intra, cols["count"][ii], cols["prior"][ii])
        out["ran"][ii] = True
    return out


@pytest.fixture(scope="module")
def device():
    from fithic_amd import _capi
    cols, _ = pr.load_fixture()
    for v in cols.values():
        v.setflags(write=False)
    got = {}
    for mode in MODES:
        c = _capi.Context(0)          # raises if there is no GPU or the library is missing: no fallback
        try:
            if mode == "wide":
                c.set_params(10000, totals=_capi.TOTALS_WIDE)
            totals = tuple(t for t in pr.FIXTURE_TOTALS if mode == "wide" or t < 2.0 ** 31)
            got[mode] = _run(c, cols, totals)
        finally:
            c.close()
    return cols, got


def _held(cols, got, mode, sel, what):
    return pr.assert_p_faithful(got[sel], cols["count"][sel], cols["total"][sel], cols["prior"][sel], totals=mode, what=what)


@pytest.mark.parametrize("mode", MODES)
def test_bdtrc_array_is_faithful_on_the_chosen_rows(device, mode):
    cols, got = device
    ran = got[mode]["ran"]
    assert ran.sum() == (len(ran) if mode == "wide" else (cols["total"] < 2.0 ** 31).sum())
    table = _held(cols, got[mode]["lane"], mode, ran, "bdtrc_array, %s totals" % mode)
    print("\nbdtrc_array, %s totals\n%s" % (mode, table))
    assert table.n_rows >= 0.98 * ran.sum() > 1700              # all but the few rows that are NaN on purpose


@pytest.mark.parametrize("nonfixed", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_pass_kernels_are_faithful_on_the_chosen_rows(device, mode, nonfixed):
    """the launches of a pass (k2_classify or its nonfixed twin, the closed forms, the class kernels, the count-sorted heavy class)
    on the same rows, each total once as the intra binomial and once as the inter one: the bar, bit-equality with the per-lane
    entry, and the class counts of the numpy restatement"""
    cols, got = device
    g = got[mode]
    for side in ("intra", "inter"):
        p = g[(side, nonfixed)]
        table = _held(cols, p, mode, g["ran"], "debug_k2_rows, %s totals, %s side, nonfixed %s" % (mode, side, nonfixed))
        assert bits_equal(np.nan_to_num(p[g["ran"]], nan=-1.0), np.nan_to_num(g["lane"][g["ran"]], nan=-1.0)), (mode, side, nonfixed)   # NaN: any payload
        if side == "intra":
            print("\ndebug_k2_rows, %s totals, nonfixed %s\n%s" % (mode, nonfixed, table))
    seen = 0
    for what, by_class, want in g["classes"]:
        if what[2] == nonfixed:
            assert by_class == want, what
            seen += 1
    assert seen == (6 if mode == "wide" else 5)


@pytest.mark.parametrize("mode", MODES)
def test_rows_whose_oracle_value_is_zero_or_subnormal(device, mode):
    """on their own, so that a failure names them: where Cephes returns 0 below MINLOG (and both nudged builds do) the device must
    return 0 up to two subnormal steps, and a subnormal value must be that subnormal value"""
    cols, got = device
    g = got[mode]
    o, _, _ = pr.reference(cols["count"], cols["total"], cols["prior"], mode)
    with np.errstate(invalid="ignore"):
        tiny = g["ran"] & (np.abs(o) < pr.MIN_NORMAL) & (kr.outcome(cols["count"], cols["total"], cols["prior"]) != kr.TRIVIAL)
    assert (o[tiny] == 0.0).sum() >= 100 and (o[tiny] != 0.0).sum() >= 100
    for key in ("lane", ("intra", False), ("inter", False), ("intra", True), ("inter", True)):
        table = _held(cols, g[key], mode, tiny, "oracle value 0 or subnormal, %s totals, %s" % (mode, key))
        assert np.all(g[key][tiny & (o == 0.0)] <= pr.TINY_U)
    print("\noracle value 0 or subnormal, %s totals (the last result)\n%s" % (mode, table))
