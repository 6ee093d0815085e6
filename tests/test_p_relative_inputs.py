"""The relative bar on p-values (tests/p_relative.py) and its fixture of chosen rows (tests/golden/f16_bdtrc_tail.npz), checked
without a GPU: the fixture fills every cell it claims, the oracle is scipy on it bit for bit, the bar has teeth on nearly all rows,
and the helper refuses the defects that the absolute bar of 1e-10 lets through."""
import numpy as np
import pytest

import k2_rows as kr
import p_relative as pr
from conftest import bits_equal, max_abs_diff

TOL = 1e-10                    # the absolute bar of the GPU tests, for the "passes today" halves below


@pytest.fixture(scope="module")
def fx():
    cols, meta = pr.load_fixture()
    ref_mode = cols["total"] < 2.0 ** 31
    o, S = np.empty(len(ref_mode)), np.empty(len(ref_mode))
    for mode, sel in (("reference", ref_mode), ("wide", ~ref_mode)):
        o[sel], S[sel], _ = pr.reference(cols["count"][sel], cols["total"][sel], cols["prior"][sel], mode)
    o.setflags(write=False)
    S.setflags(write=False)
    return cols, meta, ref_mode, o, S


def test_every_reachable_cell_holds_its_rows(fx):
    cols, meta, ref_mode, _, _ = fx
    assert len(cols["count"]) == meta["rows"] <= 4200
    assert set(np.unique(cols["total"])) == set(pr.FIXTURE_TOTALS) and (~ref_mode).sum() == (cols["total"] == 7150761687.0).sum() > 0
    cells = pr.fixture_cells(cols)
    every = {pr.cell_name(t, w, b) for t in pr.FIXTURE_TOTALS for w in pr.FIXTURE_OUTCOMES for b in range(len(pr.FIXTURE_BANDS))}
    assert all(len(v) >= pr.FIXTURE_PER_CELL for v in cells.values()), {k: len(v) for k, v in cells.items() if len(v) < pr.FIXTURE_PER_CELL}
    assert sorted(every - set(cells)) == meta["unreachable"]
    assert set(cells) == set(meta["cells"]) and all(meta["cells"][k]["rows"] == len(v) for k, v in cells.items())
    # the small tail is there: every band of the power series, of incbcf (where the total allows it) and of the local closed form
    for t in pr.FIXTURE_TOTALS:
        for b in range(len(pr.FIXTURE_BANDS)):
            assert pr.cell_name(t, kr.PSERIES, b) in cells
            assert b > 3 or pr.cell_name(t, kr.CF_BCF, b) in cells
            assert b > 3 or pr.cell_name(t, kr.CLOSED_LOCAL, b) in cells
    # the counts the issue names, and the tiny prior of count 1 whose p is a small multiple of 2^-53
    for c in (1, 2, 3, 126, 127, 128, 129, 1022, 1023, 1024, 5000):
        assert (cols["count"] == c).any(), c
    assert ((cols["count"] == 1) & (cols["total"] == 1.0e6) & (cols["prior"] == 1e-12)).any()
    assert np.isnan(cols["scipy"][~ref_mode]).all()


def test_oracle_reproduces_the_scipy_column_bit_for_bit(fx):
    cols, _, ref_mode, o, _ = fx
    assert bits_equal(np.isnan(o[ref_mode]), np.isnan(cols["scipy"][ref_mode])) and np.isnan(o[ref_mode]).sum() >= 15
    assert bits_equal(np.nan_to_num(o[ref_mode], nan=-1.0), np.nan_to_num(cols["scipy"][ref_mode], nan=-1.0))


def test_reference_error_record_is_reproduced(fx):
    """the reference against the exact tail, per cell: a record (up to 2.5e-6 relative at total 645040870), not a bar"""
    cols, meta, _, o, S = fx
    worst = 0.0
    for name, idx in pr.fixture_cells(cols).items():
        rec, want = pr.cell_record(o[idx], S[idx], cols["exact"][idx]), meta["cells"][name]
        for key in ("ref_abs_err_max", "ref_rel_err_max", "bar_abs_max"):
            assert rec[key] == pytest.approx(want[key], rel=1e-6, abs=0.0), (name, key)
        assert (rec["bar_rel"] is None) == (want["bar_rel"] is None)
        if rec["bar_rel"] is not None:
            assert all(rec["bar_rel"][k] == pytest.approx(want["bar_rel"][k], rel=1e-6) for k in ("median", "p99", "max")), name
        worst = max(worst, rec["ref_rel_err_max"] or 0.0)
    assert 1e-6 < worst < 1e-5                         # Cephes is that far from the exact value: the oracle is the yardstick
    # below the double range the reference gives 0
    deep = pr.fixture_band(cols["exact_log10"]) == 5
    assert deep.sum() >= 16 * 10 and (o[deep] == 0.0).all() and (cols["exact"][deep] == 0.0).all()


def test_the_bar_has_teeth_on_nearly_every_row(fx):
    cols, meta, _, o, S = fx
    in_cells = np.concatenate(list(pr.fixture_cells(cols).values()))
    normal = in_cells[np.abs(o[in_cells]) >= pr.MIN_NORMAL]
    rel = pr.bar_of(o, S)[normal] / np.abs(o[normal])
    share = float((rel <= pr.TIGHT).mean())
    small = o[normal] < 1e-10
    print("bar <= 1e-9 relative on %.4f of %d normal-range rows, on %.4f of the %d with p < 1e-10" % (share, len(normal), (rel[small] <= pr.TIGHT).mean(), small.sum()))
    assert share >= 0.95 and float((rel[small] <= pr.TIGHT).mean()) >= 0.95
    assert share == pytest.approx(meta["share_bar_le_1e-9"], abs=1e-3)
    assert small.mean() > 0.5                                        # most of the fixture lies where the absolute bar sees nothing
    # the closed forms of count 1 take no libm call on most rows: only the 4-ulp floor applies
    local = in_cells[kr.outcome(cols["count"], cols["total"], cols["prior"])[in_cells] == kr.CLOSED_LOCAL]
    assert (S[local] == 0.0).mean() > 0.9


def _doctored(fx):
    """(name, doctored column, rows touched) on the reference-mode rows of the fixture whose bar is at most 1e-9 relative"""
    cols, _, ref_mode, o, S = fx
    with np.errstate(invalid="ignore", divide="ignore"):
        tight = ref_mode & (np.abs(o) >= pr.MIN_NORMAL) & (pr.bar_of(o, S) / np.abs(o) <= pr.TIGHT)
    oc = kr.outcome(cols["count"], cols["total"], cols["prior"])
    small = tight & (o < 1e-10)
    assert small.sum() > 300
    g = o.copy()
    g[small] = o[small] * (1.0 + 1e-8)
    yield "o (1 + 1e-8)", g, small
    g = o.copy()
    g[small] = 0.0
    yield "0 in place of a normal p < 1e-10", g, small
    zero = ref_mode & (o == 0.0) & (S == 0.0) & (oc != kr.TRIVIAL)
    assert zero.sum() > 100
    g = o.copy()
    g[zero] = 1e-200
    yield "a normal p in place of the reference's 0", g, zero
    local = small & (oc == kr.CLOSED_LOCAL)
    assert local.sum() >= 48
    g = o.copy()
    g[local] = (o[local].view(np.int64) + 64).view(np.float64)
    yield "64 ulp on closed_local rows", g, local
    i = int(np.flatnonzero(np.isnan(o) & ref_mode)[0])
    j = int(np.flatnonzero(small)[0])
    g = o.copy()
    g[i], g[j] = o[j], np.nan
    yield "a NaN moved to another row", g, None


def test_the_helper_is_not_vacuous(fx):
    cols, _, ref_mode, o, S = fx
    from oracle import fithic_oracle as fo
    args = (cols["count"][ref_mode], cols["total"][ref_mode], cols["prior"][ref_mode])
    table = pr.assert_p_faithful(o[ref_mode], *args, what="the oracle itself")
    assert table.n_same == table.n_rows == int((~np.isnan(o[ref_mode])).sum()) and table.worst == 0.0
    for nudged in fo.bdtrc_nudged(args[0].astype(np.float64) - 1.0, args[1], args[2]):
        assert not bits_equal(nudged, o[ref_mode])
        t = pr.assert_p_faithful(nudged, *args, what="a nudged libm")
        assert 0.0 < t.worst <= 0.5 + 1e-12                           # S measures exactly this; the bar holds 2 S
    wide = ~ref_mode
    pr.assert_p_faithful(o[wide], cols["count"][wide], cols["total"][wide], cols["prior"][wide], totals="wide", what="the oracle, wide")
    for name, g, touched in _doctored(fx):
        with pytest.raises(AssertionError, match="NaN pattern" if touched is None else "further from the oracle"):
            pr.assert_p_faithful(g[ref_mode], *args, what=name)
        if touched is not None:
            assert max_abs_diff(g[ref_mode], o[ref_mode]) <= TOL, name          # ... and today's absolute bar accepts it
            msg, _ = pr.check_p_faithful(g[ref_mode], *args)
            assert "%d of" % touched.sum() in msg, name                         # every doctored row is refused, no other
        else:
            with pytest.raises(AssertionError, match="NaN pattern differs"):
                max_abs_diff(g[ref_mode], o[ref_mode])


def test_the_report_names_rows_and_outcomes(fx):
    cols, _, ref_mode, o, S = fx
    name, g, touched = next(_doctored(fx))
    msg, table = pr.check_p_faithful(g[ref_mode], cols["count"][ref_mode], cols["total"][ref_mode], cols["prior"][ref_mode])
    assert msg.count("count ") == 5 and "oracle" in msg and " S " in msg and any(n in msg for n in kr.OUTCOME_NAMES)
    text = str(table)
    assert "bit-identical" in text and all(kr.OUTCOME_NAMES[w] in text for w in pr.FIXTURE_OUTCOMES)
    assert set(table.per_outcome()) >= {kr.OUTCOME_NAMES[w] for w in pr.FIXTURE_OUTCOMES}


def test_pass_result_carries_prior_and_total():
    """PassResult.prior / bdtrc_n: bdtrc on them is the pass's p, and the rows without them keep p = 1"""
    from conftest import load_case, case_args
    from oracle import fithic_oracle as fo
    meta, _ = load_case("f6_quirk_all")
    kw = case_args(meta)
    pairs = fo.read_contacts_file(kw["contacts"])
    for r in fo.run(**kw):
        reach = ~np.isnan(r.bdtrc_n)
        assert 0 < reach.sum() < len(reach)
        assert (r.p[~reach] == 1.0).all() and np.isnan(r.prior[~reach]).all()
        assert set(np.unique(r.bdtrc_n[reach])) <= {float(r.sums[3]), float(r.sums[1])}
        assert bits_equal(fo.bdtrc(pairs.count[reach] - 1.0, r.bdtrc_n[reach], r.prior[reach]), r.p[reach])
        pr.assert_pass_p_faithful(r.p, pairs.count, r, what="the oracle's own pass")
