"""k1_classify_hist where the counters of its LDS window overflow, on the tables of tests/k1_windows.py (what each one reaches is
held by tests/test_k1_window_inputs.py, without a GPU): u32 sums that wrap, 15-bit row counts that set their guard bit, residues of
exactly 0 at the flush, the last LDS bin and the first bins beyond it, a rotated flush whose start bin is a remainder, and the
switch between the 6144-bin and the 24 576-bin instantiation at 6144 / 6145 distance values.

Every table is loaded with Context.load_pairs, so k0_slots writes the key column, and counted twice: by the keys and by the three
int32 columns (debug_k1_wide).  The ten statistics fields and both histograms equal the count made with numpy (k1_windows.numpy_k1)
exactly: everything is an integer, == and array_equal.  A failure names the first differing distance and both values: a difference
of 32 768 rows or of 2^32 in a sum names the path.

What a break of fhx_k1.hip would fail here (reasoned, not run):
  no atomicSub of the guard bit                  the large table: workgroups 1 - 8 flush their 2^15 a second time, and from 65 536
                                                  rows on (workgroups 4 - 6) the half-word carries into its neighbour or out of the word
  the guard bit's `<< sh` lost on either side    the large table: H is odd, its neighbours in workgroups 7 and 8 are even
  `& 0xFFFF` lost from `was`                     the large table's workgroup 7: the even bin's crossing with rows in the odd half of
                                                  its word; workgroup 8 is the control with the neighbour in the next word
  2^15 rows added at `lo_idx + d` or at `b`      the large table (-L 1) and nothing else: only there a guard bit is set
  `was == 0x8000` for `was == 0x7FFF`            nothing, and rightly: that kernel counts the same.  The flush reads all 16 bits of
                                                  a half-word, so a count left at 0x8000 is flushed as 32 768 (workgroups 1 and 4), and
                                                  the add that finds 0x8000 moves 2^15 one row later (workgroups 2, 3, 5 - 8); a half-word
                                                  stays below 0x8000 + 1024 either way
  no `1ull << 32` added on a wrap                A3 (2^32 short), A2, A4, A5, A6, A8
  `if (sum)` around the row-count flush as well  A2: a sum of exactly 2^32 leaves residue 0 with three rows in the bin
  `d` for `b` in the half-word shift             every -L7 case (A7) and the large table (-L 1): the row count lands in the
                                                  neighbour's half
  a missed or repeated bin when the flush wraps  the large table's workgroups 64, 65, 255; N1's workgroup 4
  `>` for `>=` at the end of the LDS window      A6: bins 24 575 and 24 576
  `>` 6144 read as `>=` in launch_k1             N1 would still be right (both kernels are), which is why N1 and N2 are held to
                                                  numpy and not to each other"""
import numpy as np
import pytest

import k1_windows as kw

pytestmark = pytest.mark.gpu


def device_k1(c, columns):
    from fithic_amd import _capi
    c.debug_k1_wide(columns)
    try:
        st = c.pass_stats().as_dict()
    finally:
        c.debug_k1_wide(False)
    return st, c.get_array(_capi.A_HIST_SUMCC).copy(), c.get_array(_capi.A_HIST_NPAIRS).copy()


def same_histogram(got, want, what):
    assert got.shape == want.shape, what + (got.shape, want.shape)
    if not np.array_equal(got, want):
        d = int(np.flatnonzero(got != want)[0])
        raise AssertionError(what + ("first differing distance %d of %d: device %d, numpy %d, difference %d"
                                     % (d, int((got != want).sum()), int(got[d]), int(want[d]), int(got[d]) - int(want[d])),))


def both_ways(c, case, want):
    for columns in (False, True):
        how = "columns" if columns else "keys"
        st, cc, npairs = device_k1(c, columns)
        for f in kw.STAT_FIELDS:
            assert st[f] == want[0][f], (case.name, how, f, st[f], want[0][f])
        same_histogram(npairs, want[2], (case.name, how, "rows per distance"))
        same_histogram(cc, want[1], (case.name, how, "sum of counts per distance"))


def load(c, case):
    from fithic_amd import _capi
    c.set_params(case.res, case.low, case.up, 10, 1, _capi.MODE_ALL)
    c.load_pairs(*case.mids())


@pytest.fixture()
def ctx():
    from fithic_amd import _capi
    c = _capi.Context(0)            # raises if there is no GPU or the library is missing: no fallback
    yield c
    c.close()


@pytest.mark.parametrize("case", kw.small_cases(), ids=lambda c: c.name)
def test_sums_that_wrap_and_the_edges_of_the_lds_window(ctx, case):
    """A1 - A6, A8, A9, each with -L 0 and with an odd lo_idx (A7)"""
    load(ctx, case)
    both_ways(ctx, case, kw.numpy_k1(case.rows, case.res, case.low, case.up))
    assert ctx.stats().n_dist - 1 - case.low > kw.K1_WIDE_BINS          # bins beyond the LDS window exist: the 24 576-bin kernel


@pytest.fixture(scope="module")
def large():
    """one context, one load, one count with numpy for the module"""
    from fithic_amd import _capi
    case = kw.large_table()
    want = kw.numpy_k1(case.rows, case.res, case.low, case.up)
    c = _capi.Context(0)
    load(c, case)
    yield c, case, want
    c.close()


def test_row_counts_that_set_the_guard_bit(large):
    """the large table: 32 767 .. 65 537 rows of one bin in one workgroup, two bins of one word crossing together, 256 flushes"""
    c, case, want = large
    both_ways(c, case, want)
    on_h = sum(kw.LARGE_H_ROWS.values()) + len(kw.LARGE_PAIRED) * kw.LARGE_PAIRED_ROWS + len(kw.LARGE_BIG_WGS)
    assert want[2][case.low + kw.H] >= on_h > 13 * kw.GUARD and want[1][case.low + kw.H] >= kw.WRAP


@pytest.mark.parametrize("case", kw.switch_cases(), ids=lambda c: c.name)
def test_switch_between_the_two_instantiations(ctx, case):
    """N1 (6144 distance values: the narrow kernel) and N2 (6145: the 24 576-bin kernel) on the same rows"""
    load(ctx, case)
    both_ways(ctx, case, kw.numpy_k1(case.rows, case.res, case.low, case.up))
