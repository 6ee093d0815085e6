"""K3's entry points one after another on ONE context: no call depends on what another left behind.

fhx_bh, fhx_bh_array and the sharded sequence (fhx_bh_top_hist, fhx_bh_set_cutoff, fhx_bh_local_sort, fhx_bh_apply_sorted,
fhx_bh_scatter) share the compaction, the sorts and the BH scan; what one call's steps hand to each other (whether the survivors'
number comes from the key histogram, who zeroed the counter, whether that number is a bound) lives in a value on that call's stack.
Every result is held bit for bit to the oracle's Benjamini-Hochberg (oracle.fithic_oracle.benjamini_hochberg).

The array of step 3 has 131 073 values that take a rank - one more than the LDS tile sorts hold, so the one-sweep passes and their
repair run - and three NaN on top of them: NaN rows are not compacted, so NaN among the 131 073 would have left 131 070 keys to the
tile sorts and step 3 would not have met the large sort at all."""
import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

RES = 5000


def _same(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and bits_equal(np.nan_to_num(got, nan=-1.0), np.nan_to_num(want, nan=-1.0))


def _array(rng, n_ranked, n_nan, n_ones, shared_tops):
    """n_ranked values in [0, 1] (n_ones of them 1.0) that share their top 40 key bits in runs of a few and differ below, n_nan NaN"""
    tops = rng.random(shared_tops).view(np.uint64) & ~np.uint64((1 << 24) - 1)
    p = (rng.choice(tops, n_ranked) | rng.integers(0, 1 << 24, n_ranked).astype(np.uint64)).view(np.float64)
    p[rng.choice(n_ranked, n_ones, replace=False)] = 1.0
    assert p.min() >= 0.0 and p.max() <= 1.0
    return rng.permutation(np.concatenate([p, np.full(n_nan, np.nan)]))


def test_entry_points_in_sequence_on_one_context():
    import torch
    from fithic_amd import _capi, synth
    from fithic_amd.engine import MODES
    from oracle import fithic_oracle as fo
    rng = np.random.default_rng(17)
    genome = synth.Genome(RES, [1_000_000, 600_000])
    amp = synth.solve_amplitude(0.66, 4, 40)
    cols = [torch.cat(c).numpy() for c in zip(*(synth.cis_contacts(genome, c, 4, 40, amp) for c in range(len(genome))))]
    n = len(cols[0])
    assert 3000 < n < 20000
    ctx = _capi.Context(0)
    try:
        ctx.set_params(RES, 4 * RES, 40 * RES, 20, 1, MODES["intraOnly"])
        ctx.load_fragments(*genome.fragments(), genome.sort_rank())
        ctx.load_bias(*genome.bias_table())
        ctx.load_pairs(*cols)

        # 1. the engine's own pass
        ctx.pass_stats()
        N = ctx.fit().bh_total_tests
        ctx.pvalues()
        ctx.bh(N)
        first = ctx.fetch(n)
        p = first["p"]
        want = fo.benjamini_hochberg(p, N)
        assert (want < 1.0).any() and (want == 1.0).any()         # rows below the cutoff and rows it spares the sort
        assert _same(first["q"], want)

        # 2. a caller's array, small: LDS tile sorts + merge
        a = _array(rng, 4990, 10, 40, 900)
        assert _same(ctx.bh_array(a, 20000.0), fo.benjamini_hochberg(a, 20000.0))
        assert ctx.bh_sort_stats()["passes"] == 0

        # 3. a caller's array, one key more than the tile sorts hold and nothing saturates: one-sweep passes + repair
        b = _array(rng, 131073, 3, 500, 20000)
        assert _same(ctx.bh_array(b, 1.0), fo.benjamini_hochberg(b, 1.0))
        st = ctx.bh_sort_stats()
        assert st["passes"] == 5 and st["inversions"] > 0

        # 4. the sharded sequence, one rank, on the engine's own p
        ctx.bh_set_cutoff(ctx.bh_top_hist(), N)
        ctx.bh_local_sort()
        kept = ctx.n_sorted()
        assert np.count_nonzero(want < 1.0) <= kept <= n              # every row with q < 1 is below the cutoff
        q_sorted = torch.empty(kept, dtype=torch.float64, device="cuda:0")
        ctx.bh_apply_sorted(ctx.device_ptr(2), kept, 0, 0.0, N, q_sorted.data_ptr())
        ctx.bh_scatter(q_sorted.data_ptr())
        sharded = ctx.fetch(n)
        assert _same(sharded["p"], p) and _same(sharded["q"], want) and _same(sharded["q"], first["q"])

        # 5. the engine's own pass again
        ctx.bh(N)
        again = ctx.fetch(n)
        assert _same(again["q"], want) and _same(again["q"], first["q"])
    finally:
        ctx.close()
