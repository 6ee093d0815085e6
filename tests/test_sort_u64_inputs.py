"""The inputs of tests/test_gpu_sort_u64.py, checked without a GPU: each size of tests/sort_keys.py must sit on the seam it names
and each key pattern must have the property it is there for, or the GPU test would pass without aiming at anything."""
import numpy as np

import sort_keys as sk

DIGIT_SHIFTS = (0, 11, 22, 33, 44, 55)                            # six passes of 11 bits, the last sees bits 55..63


def test_sizes_sit_on_the_seams_they_name():
    M = sk.M20
    assert [sk.blocks_for(n) for n in (M, M + 1, 3 * M + 1, 9 * M, 15728640, 15728641)] == [64, 128, 256, 576, 960, 1024]
    assert [sk.chunk_for(n) for n in (262143, 262144, 262145)] == [4096, 4096, 8192]
    assert 9 * M in sk.LARGE and 15728641 in sk.LARGE and 576 // 64 == 9       # rs_scan: nine waves, then its launch bound
    assert {1, 2, 3, 63, 64, 65, 4095, 4096, 4097, 8191, 262143, 262144, 262145, M, M + 1, 3 * M + 1} == set(sk.SIZES)
    odd_tail = [n for n in sk.SIZES + sk.LARGE if (n - (sk.blocks_for(n) - 1) * sk.chunk_for(n)) % 2 == 1 or (n < sk.chunk_for(n) and n % 2)]
    assert len(odd_tail) >= 5                                     # rs_count's single key after the pairs
    for n in sk.SIZES + sk.LARGE:
        assert n < 2 ** 31 and sk.blocks_for(n) * sk.chunk_for(n) >= n


def test_cases_cover_every_size_and_pattern_by_name():
    assert len(sk.CASES) == len(sk.SIZES) * len(sk.PATTERNS) + len(sk.LARGE) * len(sk.LARGE_PATTERNS) == len(set(sk.CASES))
    assert {p for p, n in sk.CASES if n in sk.LARGE} == {"random64", "eight_bits55_63", "eight_bits0_10", "eight_bits22_32"}


def test_patterns_have_their_properties():
    n = 8191
    for p in sk.PATTERNS:
        keys = sk.make_keys(p, n)
        assert keys.dtype == np.uint64 and len(keys) == n
        assert np.array_equal(keys, sk.make_keys(p, n)), "deterministic"
    assert not np.array_equal(sk.make_keys("random64", 5000, 0), sk.make_keys("random64", 5000, 1))
    assert set(sk.make_keys("all_ones", 5).tolist()) == {sk.FULL} and set(sk.make_keys("all_zero", 5).tolist()) == {0}
    hot = sk.make_keys("one_hot", n)
    assert len(np.unique(hot)) == 64 and all(bin(int(k)).count("1") == 1 for k in np.unique(hot))
    for shift in DIGIT_SHIFTS:                                    # every pass sees one non-zero digit value at most per key ...
        digits = (hot >> np.uint64(shift)) & np.uint64(0x7FF)
        assert len(np.unique(digits)) == 1 + min(11, 64 - shift)  # ... and every bit of the digit decides somewhere
    asc, desc = sk.make_keys("ascending", n), sk.make_keys("descending", n)
    assert np.all(asc[1:] > asc[:-1]) and np.all(desc[1:] < desc[:-1]) and int(desc[0]) == sk.FULL
    big = np.arange(3 * sk.M20 + 1, dtype=np.uint64)[-1] * np.uint64((1 << 40) + (1 << 11) + 1)
    assert int(big) == (3 * sk.M20) * ((1 << 40) + (1 << 11) + 1) < 2 ** 63        # no wrap at the largest size that runs them


def test_eight_value_patterns_differ_only_in_their_field_and_are_mostly_stability():
    for p, lo, width in (("eight_bits55_63", 55, 9), ("eight_bits0_10", 0, 11), ("eight_bits22_32", 22, 11)):
        keys = sk.make_keys(p, 4097)
        vals = np.unique(keys)
        assert len(vals) == 8
        mask = ((1 << width) - 1) << lo
        assert len({int(v) & ~mask & sk.FULL for v in vals}) == 1 and len({int(v) & mask for v in vals}) == 8
        counts = np.bincount(np.searchsorted(vals, keys))
        assert counts.min() >= 4097 // 8                          # n/8 copies each: the order inside a value is all the sort's stability
        perm = np.argsort(keys, kind="stable")
        assert not np.array_equal(perm, np.arange(len(keys)))
    assert int(sk.make_keys("eight_bits55_63", 64).max()) >> 63 == 1
