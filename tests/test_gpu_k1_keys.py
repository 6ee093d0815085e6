"""k1_classify_hist on the 32-bit key column (fithic_amd/csrc/fhx_k1key.hpp, written by k0_slots) against the same kernel on the
three int32 columns (fhx_debug_k1_wide) and against a count made here with numpy: the seven sums, max_count, n_skipped and both
histograms of fhx_pass_stats, all three equal exactly.

a. three chromosomes, 4 099 rows (three tail rows): counts 0, 1, 8191, 8192 and 2^31 - 1 (the last two escape), inter rows with
   inline and with escaped counts, distances below, on and above both of -L / -U
b. one chromosome of 262 200 loci at resolution 1 without -U - the 24 576-bin instantiation - with d = 262 142 (the last inline
   distance), 262 143 and 262 144 (escaped) among a few hundred ordinary rows
c. every row escaped
d. later passes, with outliers injected through the p column as tests/test_gpu_pass_state.py does (tests/pass_state_model.py):
   skip bytes and the limit of the first duplicated outlier line are active, narrow and 24 576-bin instantiation
e. after (a), a shorter and different row set loaded into the same context: the key column follows the reload

Everything compared is an integer: == and array_equal."""
import numpy as np
import pytest

import pass_state_model as pm
from k1_windows import numpy_k1            # the count made with numpy: shared with tests/test_gpu_k1_windows.py

pytestmark = pytest.mark.gpu

RES = 10000
CHROMS = ((300, 5000), (220, 2500), (100, 5000))            # loci, offset of the midpoints in their bins
STAT_FIELDS = ("n_rows", "inter_count", "inter_sum", "intra_all_count", "intra_all_sum", "in_range_count", "in_range_sum", "max_count",
               "n_dist", "n_skipped")
BIG = 2 ** 31 - 1


def device_k1(c, wide):
    from fithic_amd import _capi
    c.debug_k1_wide(wide)
    try:
        st = c.pass_stats().as_dict()
    finally:
        c.debug_k1_wide(False)
    return st, c.get_array(_capi.A_HIST_SUMCC).copy(), c.get_array(_capi.A_HIST_NPAIRS).copy()


def load(c, rows, res, low, up, offsets):
    from fithic_amd import _capi
    c1, i1, c2, i2, cnt = (np.asarray(v, np.int64) for v in rows)
    off = np.asarray(offsets, np.int64)
    c.set_params(res, low, up, 10, 1, _capi.MODE_ALL)
    c.load_pairs(c1, i1 * res + off[c1], c2, i2 * res + off[c2], cnt)


def three_ways(c, rows, res, low, up, what):
    want = numpy_k1(rows, res, low, up)
    for wide in (False, True):
        got = device_k1(c, wide)
        for f in STAT_FIELDS:
            assert got[0][f] == want[0][f], (what, "columns" if wide else "keys", f, got[0][f], want[0][f])
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (what, "columns" if wide else "keys")


def rows_a(n=4099, seed=11):
    """(a): the named edges first, then a shuffled mix; row n - 1 .. n - 3 (the tail) are edges too"""
    rng = np.random.default_rng(seed)
    edge_counts = (0, 1, 8191, 8192, BIG)
    rows = [(0, 0, 0, 299, 1), (1, 0, 1, 219, 2)]
    for k, c in enumerate(edge_counts):
        for d in (1, 2, 3, 249, 250, 251):                   # -L 2 bins, -U 250 bins: below, on, above each
            rows.append((0, k, 0, k + d, c))
        rows.append((0, 7 * k, 1, 3 * k, c))                 # inter rows with both kinds of count
        rows.append((2, k, 0, 200 + k, c))
    while len(rows) < n - 3:
        if rng.random() < 0.15:
            a, b = rng.choice(3, 2, replace=False)
            rows.append((a, int(rng.integers(CHROMS[a][0])), b, int(rng.integers(CHROMS[b][0])), int(rng.choice((1, 3, 8191, 8192, 70000)))))
        else:
            ch = int(rng.integers(3))
            i, j = (int(v) for v in rng.integers(CHROMS[ch][0], size=2))
            rows.append((ch, i, ch, j, int(rng.choice((0, 1, 2, 5, 40, 8191, 8192, 12345, BIG), p=(.05, .4, .2, .1, .1, .05, .04, .03, .03)))))
    rows += [(0, 10, 0, 260, BIG), (1, 5, 2, 5, 8192), (2, 0, 2, 2, 8191)]
    return tuple(np.array(v, np.int64) for v in zip(*rows))


@pytest.fixture()
def ctx():
    from fithic_amd import _capi
    c = _capi.Context(0)            # raises if there is no GPU or the library is missing: no fallback
    yield c
    c.close()


def test_edges_of_both_fields_and_both_bounds_then_a_reload(ctx):
    """a. and e."""
    offsets = [c[1] for c in CHROMS]
    rows = rows_a()
    assert len(rows[0]) == 4099
    load(ctx, rows, RES, 2 * RES, 250 * RES, offsets)
    three_ways(ctx, rows, RES, 2 * RES, 250 * RES, "a")
    # e. other rows, fewer of them (n mod 4 = 1), into the same context: stale keys would count the old rows
    rng = np.random.default_rng(5)
    n = 1001
    ch = rng.integers(3, size=n)
    sizes = np.array([c[0] for c in CHROMS])
    again = (ch, rng.integers(sizes[ch]), ch, rng.integers(sizes[ch]), rng.choice((1, 2, 9, 8191, 8192, 30000), size=n))
    again[0][:5], again[2][:5] = 0, 1                         # some inter rows
    again[1][5], again[3][5] = 0, 299                         # the histogram keeps its length
    load(ctx, again, RES, 2 * RES, 250 * RES, offsets)
    three_ways(ctx, again, RES, 2 * RES, 250 * RES, "e")


def test_wide_window_with_distances_around_the_last_inline_one(ctx):
    """b."""
    rng = np.random.default_rng(3)
    loci = 262200
    rows = [(0, 0, 0, 262199, 3), (0, 0, 0, 262142, 5), (0, 1, 0, 262144, 7), (0, 0, 0, 262143, 11), (0, 2, 0, 262146, 8191), (0, 50, 0, 262194, 8192),
            (0, 57, 0, 262199, 1), (0, 1, 0, 262143, 13)]
    for _ in range(400):
        i = int(rng.integers(loci - 30000))
        rows.append((0, i, 0, i + int(rng.integers(30000)), int(rng.choice((1, 2, 3, 8191, 9000, BIG)))))
    rows.append((0, 5, 0, 262148, 2))                        # 409 rows: one tail row, escaped
    rows = tuple(np.array(v, np.int64) for v in zip(*rows))
    assert len(rows[0]) % 4 == 1
    d = np.abs(rows[1] - rows[3])
    assert {262142, 262143, 262144} <= set(d.tolist())
    load(ctx, rows, 1, 0, None, [0])
    three_ways(ctx, rows, 1, 0, None, "b")
    assert ctx.stats().n_dist - 1 > pm.K1_LDS_BINS           # more bins than the 12-byte window holds: the other instantiation


def test_every_row_escaped(ctx):
    """c."""
    rng = np.random.default_rng(9)
    n = 1030
    ch = rng.integers(3, size=n)
    sizes = np.array([c[0] for c in CHROMS])
    rows = (ch, rng.integers(sizes[ch]), ch.copy(), rng.integers(sizes[ch]), rng.choice((8192, 8193, 65536, BIG), size=n))
    rows[2][::7] = (rows[0][::7] + 1) % 3                     # inter rows: their counts escape as well
    rows[3][::7] = np.minimum(rows[3][::7], 99)
    rows[1][0], rows[3][0], rows[0][0], rows[2][0] = 0, 299, 0, 0
    load(ctx, rows, RES, 2 * RES, 250 * RES, [c[1] for c in CHROMS])
    three_ways(ctx, rows, RES, 2 * RES, 250 * RES, "c")


@pytest.mark.parametrize("name", ["narrow4103", "wide"])
def test_later_passes_with_a_skip_mask(ctx, name):
    """d. two rounds of injected outliers: after the second the limit of the first duplicated outlier line is set"""
    from fithic_amd import _capi
    from fithic_amd.engine import MODES
    sc = {s.name: s for s in pm.all_scenarios()}[name]
    P = sc.params
    ctx.set_params(P["resolution"], P["L"], P["U"], P["n_bins"], P["mapp_thres"], MODES[P["mode"]])
    ctx.load_fragments(*sc.frag_columns())
    ctx.load_pairs(sc.chr1, sc.mid1, sc.chr2, sc.mid2, sc.count)
    m = pm.Model(sc)
    _, info = ctx.run_pass()
    for k, rnd in enumerate(sc.schedule[:2]):
        p = np.ascontiguousarray(rnd.p_column(info.outlier_thres))
        ctx.copy(ctx.device_ptr(0), p.ctypes.data, 8 * len(p), 0)
        ctx.next_pass()
        m.fold(rnd.rows)
        want, _, cc, npairs = m.next_k1(None)
        for wide in (False, True):
            st, got_cc, got_np = device_k1(ctx, wide)
            for f in pm.STAT_FIELDS:
                assert st[f] == want[f], (name, k, "columns" if wide else "keys", f, st[f], want[f])
            assert np.array_equal(got_cc, cc) and np.array_equal(got_np, npairs), (name, k, "columns" if wide else "keys")
        assert want["n_skipped"] > 0
        _, info = ctx.run_pass()
    assert ctx.get_skip_limit() == m.limit() != _capi.INT64_MAX
