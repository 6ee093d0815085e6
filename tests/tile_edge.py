"""Runs of equal sort keys laid across the 1024-key tiles of the run-heads kernels (csrc/fhx_scan.hpp: count_heads, scan_tiles,
head_positions, run by fhx::run_heads for the validPairs and the fragment paths), shared by test_gpu_validpairs.py and
test_gpu_fragpairs.py.  Needs no GPU."""
import numpy as np

TILE = 1024
SIZES = [1, 1023, 1024, 1025, 2049]                                  # kept pairs


def hits(n):
    """how often cell 0, 1, 2, ... (in the order of the sort keys) is hit by n kept pairs: 1000 runs of one key, a run over the
    indices 1000 .. 1023 (it starts in tile 0 and ends with it), and a run from index 1024 to the end - for 2049 pairs all of
    tile 1 and the first key of tile 2"""
    return [1] * min(n, 1000) + ([min(n, TILE) - 1000] if n > 1000 else []) + ([n - TILE] if n > TILE else [])


def file_order(n):
    """the order in which the n pairs stand in the file: the sort has to bring the runs together"""
    return np.random.default_rng(1000 + n).permutation(n).tolist()


def assert_runs_meet_the_edge(counts, n):
    """counts: the model's cell counts in the order of its sorted keys.  Cell c is the run [head[c], head[c + 1]) of them."""
    head = np.r_[0, np.cumsum(np.asarray(counts, np.int64))]
    assert head[-1] == n and np.all(np.diff(head) > 0)
    if n >= TILE:                                                    # a run ends at index 1023 and began in tile 0 at 1000 or later
        c = int(np.flatnonzero(head == TILE)[0]) - 1
        assert 1000 <= head[c] < TILE - 1
    if n > TILE:                                                     # a new run starts exactly at index 1024
        assert TILE in head[:-1]
    if n > 2 * TILE:                                                 # ... and covers all of tile 1 and reaches into tile 2
        c = int(np.flatnonzero(head == TILE)[0])
        assert head[c + 1] > 2 * TILE
