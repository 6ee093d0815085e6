"""TEST INFRASTRUCTURE - sizes and key patterns of tests/test_gpu_sort_u64.py, no GPU needed (tests/test_sort_u64_inputs.py checks
that each size sits on the seam it names and each pattern has the property it is there for).

Sizes come from the code (fhx_k3.hip): nblk = clamp(roundup64(ceil(n / 16384)), 64, 1024) workgroups (sort_blocks_for), chunk =
roundup4096(ceil(n / nblk)) keys per workgroup, a scatter tile of 4096 keys, two keys per lane in rs_count with an odd-length
tail, rs_scan with blockDim = nblk.  Patterns aim at the digit seams of the six passes (11 bits each, the last over nine), at
stability, and at the dead-lane filler ~0, which is also a legal key."""
import numpy as np

M20 = 1 << 20
TILE = 4096
SIZES = [1, 2, 3, 63, 64, 65, 4095, 4096, 4097, 8191,
         262143, 262144, 262145,                  # the first size whose chunks are two tiles
         M20, M20 + 1,                            # 64 -> 128 workgroups
         3 * M20 + 1]                             # 256 workgroups
LARGE = [9 * M20,                                 # 576 workgroups: rs_scan with nine waves
         15728641]                                # the first size with 1024 workgroups: rs_scan at its launch bound
FULL = (1 << 64) - 1
EIGHT_9 = (0, 1, 2, 0x0FF, 0x100, 0x101, 0x1FE, 0x1FF)           # eight values of a 9-bit field, both ends and the middle
EIGHT_11 = (0, 1, 2, 0x3FF, 0x400, 0x401, 0x7FE, 0x7FF)


def blocks_for(n):
    """sort_blocks_for restated"""
    want = -(-n // 16384)
    return max(64, min(1024, -(-want // 64) * 64))


def chunk_for(n):
    """keys per workgroup, as rs_count and rs_scatter compute it"""
    return -(-(-(-n // blocks_for(n))) // TILE) * TILE


def _eight(n, rng, field, shift):
    fill = 0x5555555555555555 & ~(((1 << (11 if field is EIGHT_11 else 9)) - 1) << shift)
    vals = np.array([fill | (v << shift) for v in field], np.uint64)
    return vals[rng.permutation(n) % 8]


def make_keys(pattern, n, salt=0):
    rng = np.random.default_rng(1000003 * len(pattern) + n + 7919 * salt)
    i = np.arange(n, dtype=np.uint64)
    if pattern == "random64":
        keys = rng.integers(0, FULL, n, dtype=np.uint64, endpoint=True)
        if n >= 64:
            assert (keys >> np.uint64(63)).any() and not (keys >> np.uint64(63)).all()
        return keys
    if pattern == "all_zero":
        return np.zeros(n, np.uint64)
    if pattern == "all_ones":
        return np.full(n, FULL, np.uint64)
    if pattern == "one_hot":
        return (np.uint64(1) << (i % np.uint64(64)))[rng.permutation(n)]
    if pattern == "eight_bits55_63":
        return _eight(n, rng, EIGHT_9, 55)
    if pattern == "eight_bits0_10":
        return _eight(n, rng, EIGHT_11, 0)
    if pattern == "eight_bits22_32":
        return _eight(n, rng, EIGHT_11, 22)
    step = np.uint64((1 << 40) + (1 << 11) + 1)                  # n < 2^22 here: i * step stays below 2^63
    if pattern == "ascending":
        return i * step
    if pattern == "descending":
        return np.uint64(FULL) - i * step
    raise KeyError(pattern)


PATTERNS = ["random64", "all_zero", "all_ones", "one_hot", "eight_bits55_63", "eight_bits0_10", "eight_bits22_32", "descending", "ascending"]
LARGE_PATTERNS = ["random64", "eight_bits55_63", "eight_bits0_10", "eight_bits22_32"]
CASES = [(p, n) for n in SIZES for p in PATTERNS] + [(p, n) for n in LARGE for p in LARGE_PATTERNS]
