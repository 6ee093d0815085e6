"""The inputs of tests/test_gpu_k1_windows.py, checked without a GPU: every table of tests/k1_windows.py must reach the seam of
k1_classify_hist's window it is named for - by the model of which workgroup meets which row (k1_windows.per_workgroup) - or the GPU
tests would pass without testing anything.  The numpy count the device is held to is itself held to a count made with a dict."""
import numpy as np
import pytest

import k1_windows as kw
from k1_windows import BIG, WRAP, GUARD


def small(name, lo):
    return kw.small_case(name, lo)


def dict_k1(case):
    """the histograms and sums of numpy_k1 once more, row by row in plain Python"""
    lo = -(-case.low // case.res)
    longest = 0
    for c1, i1, c2, i2, cnt in zip(*(v.tolist() for v in case.rows)):
        longest = max(longest, i1, i2)
    hi = longest + 1 if case.up is None else min(case.up // case.res, longest + 1)
    st = dict.fromkeys(kw.STAT_FIELDS, 0)
    st["n_dist"] = longest + 2
    cc, rows = {}, {}
    for c1, i1, c2, i2, cnt in zip(*(v.tolist() for v in case.rows)):
        st["n_rows"] += 1
        st["max_count"] = max(st["max_count"], cnt)
        if c1 != c2:
            st["inter_count"] += 1
            st["inter_sum"] += cnt
            continue
        st["intra_all_count"] += 1
        st["intra_all_sum"] += cnt
        d = abs(i1 - i2)
        if lo <= d <= hi:
            st["in_range_count"] += 1
            st["in_range_sum"] += cnt
            cc[d] = cc.get(d, 0) + cnt
            rows[d] = rows.get(d, 0) + 1
    return st, cc, rows


@pytest.mark.parametrize("case", kw.small_cases() + kw.switch_cases(), ids=lambda c: c.name)
def test_numpy_reference_agrees_with_a_dict_count(case):
    st, cc, npairs = kw.numpy_k1(case.rows, case.res, case.low, case.up)
    want_st, want_cc, want_rows = dict_k1(case)
    assert st == want_st
    assert cc.dtype == npairs.dtype == np.int64 and len(cc) == len(npairs) == st["n_dist"]
    assert {int(d): int(cc[d]) for d in np.flatnonzero(npairs)} == want_cc
    assert {int(d): int(npairs[d]) for d in np.flatnonzero(npairs)} == want_rows
    assert not cc[npairs == 0].any()


@pytest.mark.parametrize("lo", kw.LOWS)
def test_small_tables_are_one_wide_workgroup_and_a7_has_an_odd_low_index(lo):
    for name in kw.SMALL_NAMES:
        L = kw.launch(small(name, lo))
        assert L.wide and L.lo == lo and L.width > kw.K1_WIDE_BINS + 100, name
        assert L.blocks == (3 if name == "A8" else 1) and L.n <= (8211 if name == "A8" else 4096), name
    assert kw.LOWS[0] % 2 == 0 and kw.LOWS[1] % 2 == 1          # A7: b = d - lo_idx and d differ in parity


def _rows_of_bin(case, b):
    """row numbers and counts of window bin b, in table order"""
    c1, i1, c2, i2, cnt = case.rows
    L = kw.launch(case)
    at = np.flatnonzero((c1 == c2) & (np.abs(i1 - i2) - L.lo == b))
    return at, cnt[at]


@pytest.mark.parametrize("lo", kw.LOWS)
def test_a1_to_a5_sums_per_workgroup(lo):
    want = {"A1": lambda s: s == WRAP - 2, "A2": lambda s: s == WRAP, "A3": lambda s: s == WRAP + 1,
            "A4": lambda s: 5 * WRAP <= s < 6 * WRAP, "A5": lambda s: WRAP < s == 2 * BIG + 8191}
    for name, ok in want.items():
        case = small(name, lo)
        rows, s = kw.per_workgroup(case).at(0, kw.SMALL_BIN[name])
        assert ok(s) and rows == len(kw.SCENARIOS[name]), (name, rows, s)
        at, cnt = _rows_of_bin(case, kw.SMALL_BIN[name])
        assert at[0] % 4 == 0 and np.array_equal(at, at[0] + np.arange(len(at))), name      # from a group boundary on, consecutive
        assert tuple(cnt.tolist()) == kw.SCENARIOS[name], name
    # A5: the two escaped rows and the inline one are one lane's step, in this order
    at, cnt = _rows_of_bin(small("A5", lo), kw.SMALL_BIN["A5"])
    assert len(set((at // 4).tolist())) == 1 and cnt[-1] == 8191 < 8192 and int(cnt[:2].sum()) < WRAP
    assert {b % 2 for b in kw.SMALL_BIN.values()} == {0, 1}


@pytest.mark.parametrize("lo", kw.LOWS)
def test_a6_hits_the_first_bin_the_last_lds_bin_and_two_hbm_bins_only(lo):
    for k, name in enumerate(("A1", "A2", "A3", "A4")):
        pw = kw.per_workgroup(small("A6-%d" % (k + 1), lo))
        assert pw.bins() == [0, 24575, 24576, 24577]
        want = (len(kw.SCENARIOS[name]), sum(kw.SCENARIOS[name]))
        for b in (0, 24575):
            assert pw.at(0, b, lds=True) == want and pw.at(0, b, lds=False) == (0, 0)
        for b in (24576, 24577):                                    # not in LDS
            assert pw.at(0, b, lds=False) == want and pw.at(0, b, lds=True) == (0, 0)


@pytest.mark.parametrize("lo", kw.LOWS)
def test_a8_residues_of_one_bin_in_three_workgroups(lo):
    pw = kw.per_workgroup(small("A8", lo))
    assert pw.launch.blocks == 3
    B = kw.A8_BINS
    sums = {k: [pw.at(w, b)[1] for w in range(3)] for k, b in B.items()}
    assert sums["no_wrap"] == [BIG, BIG, 0] and sum(sums["no_wrap"]) < WRAP
    assert len(pw.workgroups(B["one_wraps"])) >= 3
    assert sums["one_wraps"] == [BIG, WRAP + 1, 7]                       # one workgroup wraps, two hold a residue only
    assert sums["exact"] == [1, 8191 + 8192, WRAP] and len(pw.workgroups(B["exact"])) >= 3
    assert sums["five_wraps"][0] >= 5 * WRAP and sums["five_wraps"][1:] == [BIG, BIG + 1]
    # the 2^32 of the last workgroup is one lane's BIG, BIG, 2 and lies in front of the tail rows, which workgroup 0 takes
    at, cnt = _rows_of_bin(small("A8", lo), B["exact"])
    assert at[-3:].tolist() == [8200, 8201, 8202] and cnt[-3:].tolist() == [BIG, BIG, 2] and (len(small("A8", lo)) >> 2) << 2 == 8208


@pytest.mark.parametrize("lo", kw.LOWS)
def test_a9_negative_count_goes_past_the_lds_window(lo):
    case = small("A9", lo)
    pw = kw.per_workgroup(case)
    assert pw.at(0, kw.A9_BINS["alone"], lds=False) == (1, -1) and pw.at(0, kw.A9_BINS["alone"], lds=True) == (0, 0)
    assert pw.at(0, kw.A9_BINS["shared"], lds=False) == (1, -1) and pw.at(0, kw.A9_BINS["shared"], lds=True) == (2, 5 + 8192)
    st, cc, npairs = kw.numpy_k1(case.rows, case.res, case.low, case.up)
    assert cc[lo + kw.A9_BINS["alone"]] == -1 and npairs[lo + kw.A9_BINS["alone"]] == 1 and st["max_count"] >= 8192


def test_large_table_rows_per_workgroup():
    case = kw.large_table()
    assert len(case) == 256 * 4096 * 17 + 3 >= 2 ** 24
    pw = kw.per_workgroup(case)
    L = pw.launch
    assert L.wide and L.blocks == 256 and L.lo == 1 and L.lo % 2 == 1 and L.width > kw.LARGE_LAST_BIN
    met = np.bincount(kw.workgroup_of_rows(L.n, L.blocks, L.threads))
    assert met[0] == 69632 + 3 and (met[1:] == 69632).all()
    H = kw.H
    rows_h = [pw.at(w, H)[0] for w in range(9)]
    assert rows_h == [32767, 32768, 32769, 65535, 65536, 65537, 69632, 34000, 34000]
    assert [GUARD - 1, GUARD, GUARD + 1, 2 * GUARD - 1, 2 * GUARD, 2 * GUARD + 1] == rows_h[:6]
    for w in range(7):
        assert [b for b in pw.b[pw.wg == w].tolist()] == [H], w            # nothing else in range there
    # 7: the neighbour shares H's word; 8: it lies in the next word.  Alternating rows: both guards are crossed at the same step
    assert pw.at(7, H ^ 1)[0] == 34000 and (H ^ 1) >> 1 == H >> 1 and sorted(pw.b[pw.wg == 7].tolist()) == [H ^ 1, H]
    assert pw.at(8, H + 1)[0] == 34000 and (H + 1) >> 1 != H >> 1 and sorted(pw.b[pw.wg == 8].tolist()) == [H, H + 1]
    c1, i1, c2, i2, cnt = case.rows
    wg = kw.workgroup_of_rows(L.n, L.blocks, L.threads)
    for w, other in kw.LARGE_PAIRED.items():
        mine = np.flatnonzero(wg == w)[:68000]
        assert (i2[mine[0::2]] == L.lo + H).all() and (i2[mine[1::2]] == L.lo + other).all() and (c2[mine] == 0).all()
    # 64, 65, 255: the flush's start bin is a remainder there
    for w in kw.LARGE_LATE:
        product, start = L.rotation(w)
        assert product >= kw.K1_WIDE_BINS and start == product % 24576 != product
        assert pw.at(w, 24575 - w)[0] >= 40000 > GUARD
    # every workgroup flushes, and the bins beyond the window get rows from nearly all of them at once
    assert sorted(set(pw.wg.tolist())) == list(range(256))
    for b in (0, 24575):
        assert len(pw.workgroups(b, lds=True)) >= 240
    for b in (24576, kw.LARGE_LAST_BIN):
        assert len(pw.workgroups(b, lds=False)) >= 240 and not pw.workgroups(b, lds=True)
    assert pw.b.max() == kw.LARGE_LAST_BIN
    # bin H passes 2^32 over all workgroups, in none of them
    own = pw.sum[(pw.b == H) & pw.lds]
    assert pw.total(H)[1] >= WRAP and own.max() < WRAP and len(own) >= 12
    # counts 1 and 2 (inline keys) but for the three rows of BIG
    values, how_many = np.unique(cnt, return_counts=True)
    assert values.tolist() == [1, 2, BIG] and how_many[2] == 3 and min(how_many[:2]) > 8_000_000
    assert (c2 == 1).sum() > 8_000_000 and ((c2 == 0) & (i2 == 0)).sum() > 8_000_000          # both kinds of filler


def test_switch_tables_stand_on_both_sides_of_6144_bins():
    n1, n2 = kw.switch_cases()
    assert all(np.array_equal(a, b) for a, b in zip(n1.rows, n2.rows)) and 8900 <= len(n1) <= 9100
    L1, L2 = kw.launch(n1), kw.launch(n2)
    assert (L1.width, L1.wide, L1.threads, L1.blocks) == (6144, False, 512, 5)
    assert (L2.width, L2.wide, L2.threads, L2.blocks) == (6145, True, 1024, 3)
    assert L1.n_dist == 7001 and L1.lo == L2.lo and L2.hi == L1.hi + 1
    c1, i1, c2, i2, cnt = n1.rows
    d = set(np.abs(i1 - i2)[c1 == c2].tolist())
    for L in (L1, L2):
        assert {L.lo - 1, L.lo, L.hi, L.hi + 1} <= d
        assert set(range(L.lo, L.hi, 100)) <= d
    pw = kw.per_workgroup(n1)
    assert pw.lds.all() and {0, 4} <= set(pw.workgroups(0)) & set(pw.workgroups(6143))  # first and last workgroup, both ends of the window
    assert L1.rotation(4)[1] > 0                                   # its flush wraps around the window's end
    pw2 = kw.per_workgroup(n2)
    assert pw2.lds.all() and pw2.b.max() == 6144 and 2 in pw2.workgroups(6144)
