"""K3 as a pass runs it - fhx_bh on the engine's own p column - on columns the test writes (tests/k3_columns.py) through
Context.device_ptr(0): the dense-q path (k3_compact<true>, k3_fill_q) and the threshold at which the device switches to it, several
tiles per workgroup with the LDS strip (forced by fhx_debug_k3_tiles_per_group), the q column prefilled behind K1 and not, the
far_below guess carried from one fhx_bh to the next, the pair and tail handling round a tile, a wave chunk and a ballot step, the
sorts as the pass selects them, and the sharded sequence on the same columns.

Every q is held to oracle.fithic_oracle.benjamini_hochberg: NaN where it has NaN, every other value bit for bit - no tolerance
anywhere.  p must come back as written, and fhx_k3_pass_info must say what tests/k3_columns.py predicts, slot by slot, so that a
column cannot quietly take another path than the one it was built for (tests/test_k3_pass_inputs.py checks the predictions cover
every branch)."""
import numpy as np
import pytest

import k3_columns as kc
from conftest import bits_equal

pytestmark = pytest.mark.gpu

RES = 5000
_rows, _oracle = {}, {}


def _same(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and bits_equal(np.nan_to_num(got, nan=-1.0), np.nan_to_num(want, nan=-1.0))


def _synth(n):
    """(genome, the first n contact rows of it): about 24 rows per locus survive at this amplitude"""
    if n not in _rows:
        import torch
        from fithic_amd import synth
        loci = n // 20 + 200
        genome = synth.Genome(RES, [RES * (loci * 3 // 5), RES * (loci - loci * 3 // 5)])
        amp = synth.solve_amplitude(0.66, 4, 40)
        cols = [torch.cat(c).numpy() for c in zip(*(synth.cis_contacts(genome, c, 4, 40, amp) for c in range(len(genome))))]
        assert len(cols[0]) >= n, (n, len(cols[0]))
        _rows[n] = genome, [np.ascontiguousarray(c[:n]) for c in cols]
    return _rows[n]


def _want(col):
    from oracle import fithic_oracle as fo
    key = (len(col.p), col.N, hash(col.p.tobytes()))
    if key not in _oracle:
        q = fo.benjamini_hochberg(col.p, col.N)
        q.setflags(write=False)
        _oracle[key] = q
    return _oracle[key]


class Pass:
    """one context with n synth rows loaded; run() is the common body of every test"""

    def __init__(self, n):
        from fithic_amd import _capi
        from fithic_amd.engine import MODES
        genome, cols = _synth(n)
        self.n, self.last, self.stage_runs = n, None, 0
        self.ctx = _capi.Context(0)                   # raises without a GPU or the library: no fallback
        self.ctx.set_params(RES, 4 * RES, 40 * RES, 20, 1, MODES["intraOnly"])
        self.ctx.load_fragments(*genome.fragments(), genome.sort_rank())
        self.ctx.load_bias(*genome.bias_table())
        self.ctx.load_pairs(*cols)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()

    def stages(self):
        """pass_stats, fit, pvalues: p is the engine's own; from the context's second pass_stats on the q column is filled with 1.0
        behind K1 (the first one finds the scratch that launch also zeroes not yet allocated)"""
        self.stage_runs += 1
        self.ctx.pass_stats()
        self.ctx.fit()
        self.ctx.pvalues()

    def write(self, col):
        p = np.ascontiguousarray(col.p, np.float64)
        assert len(p) == self.n
        self.ctx.copy(self.ctx.device_ptr(0), p.ctypes.data, 8 * len(p), 0)

    def check(self, col, what):
        got = self.ctx.fetch(self.n)
        assert _same(got["p"], col.p), (what, "p did not come back as written")
        want = _want(col)
        if not _same(got["q"], want):
            bad = np.flatnonzero(~((got["q"].view(np.int64) == want.view(np.int64)) | (np.isnan(got["q"]) & np.isnan(want))))
            r = int(bad[0])
            raise AssertionError("%s: q differs on %d rows, first row %d (tile %d, wave %d, offset %d): p %r, got %r, want %r" % (
                what, len(bad), r, r // kc.TILE, r % kc.TILE // kc.CHUNK, r % kc.CHUNK, col.p[r], got["q"][r], want[r]))
        return got["q"]

    def run(self, col, fresh=True, per=0, small_off=False, legacy=False):
        """steps 2 to 8 of the common body -> (q, info)"""
        if fresh:
            self.stages()
        self.write(col)
        self.ctx.bh(col.N)
        what = (col.name, self.n, "per=%d" % per)
        q = self.check(col, what)
        info = self.ctx.k3_pass_info()
        want = kc.predict(col.p, col.N, self.last, prefilled=fresh and self.stage_runs >= 2, per=per, small_off=small_off, legacy=legacy)
        print(what, "info", info, "predicted", want)
        for slot, (g, w) in enumerate(zip(info, want)):
            assert g == w, (what, "k3_pass_info[%d]" % slot, g, w)
        self.last = (self.n, info[1])
        return q, info


@pytest.mark.parametrize("case", kc.size_cases(), ids=[c[0] for c in kc.size_cases()])
def test_sizes_and_generators(case):
    col = kc.make(case)
    with Pass(case[1]) as P:
        q, info = P.run(col)                                  # a context's first pass ...
        assert info[6] == 0
        q2, info = P.run(col)                                 # ... and a later one: only NaN rows are stored outside the survivors
        assert info[6] == 1 and _same(q, q2)


@pytest.mark.parametrize("col", kc.strip_columns(), ids=[c.name for c in kc.strip_columns()])
def test_strip_with_several_tiles_per_workgroup(col):
    from fithic_amd import _capi
    pers = [4, 2, 3, 1] if col.name == "strip_fourth_does_not_fit" else [4, 1]
    with Pass(len(col.p)) as P:
        qs = []
        for per in pers:
            P.ctx.debug_k3_tiles_per_group(per)
            q, info = P.run(col, per=per)
            assert info[3] == per
            qs.append(q)
        assert all(bits_equal(np.nan_to_num(q, nan=-1.0), np.nan_to_num(qs[0], nan=-1.0)) for q in qs)
        P.ctx.debug_k3_tiles_per_group(0)
        _, info = P.run(col)
        assert info[3] == 1                                   # the library's own choice at these sizes
        for bad in (-1, 5):
            with pytest.raises(_capi.FhxError) as e:
                P.ctx.debug_k3_tiles_per_group(bad)
            assert e.value.code == _capi.FHX_ERR_ARG


@pytest.mark.parametrize("n", [kc.TILE + 1025, 3 * kc.TILE + 128])
def test_q_column_prefilled_and_not(n):
    """the first bh behind a pass_stats that filled the q column with 1.0 stores only NaN rows outside the survivors; every later one
    stores every row - over whatever the bh before it left there"""
    a, b = kc.threshold(n, 801, 0), kc.nan_chunk(n, 802, 0.05)
    with Pass(n) as P:
        q0, info = P.run(a)
        assert info[6] == 0
        q1, info = P.run(a)
        assert info[6] == 1 and _same(q0, q1)
        _, info = P.run(a, fresh=False)
        assert info[6] == 0
        _, info = P.run(b, fresh=False)                      # NaN and small q where column a has 1.0 ...
        assert info[6] == 0
        q4, info = P.run(a, fresh=False)                     # ... which must all be written over
        assert info[6] == 0 and _same(q4, q1)
        s = kc.sparse(n, 803)
        _, info = P.run(s)
        assert info[6] == 1
        _, info = P.run(s, fresh=False)
        assert info[6] == 0 and info[5] == 1


def test_far_below_is_carried_from_one_bh_to_the_next():
    seq = kc.far_below_sequence()
    with Pass(kc.FAR_BELOW_ROWS) as P:
        infos = [P.run(col, fresh=k == 0)[1] for k, col in enumerate(seq)]
    # sparse, all survive, sparse, all survive, all survive
    assert [(i[5], i[0]) for i in infos] == [(0, 1), (1, 0), (0, 1), (1, 0), (0, 2)]


@pytest.mark.parametrize("n_small,env,seed", kc.LARGE_CASES, ids=["%d%s" % (k, "".join("-%s=%s" % kv for kv in e.items())) for k, e, _ in kc.LARGE_CASES])
def test_large_sorts_in_the_pass(n_small, env, seed, monkeypatch):
    col = kc.large_column(n_small, seed)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with Pass(kc.LARGE_ROWS) as P:
        _, info = P.run(col, small_off=env.get("FHX_K3_SMALL") == "0", legacy=env.get("FHX_K3_SORT") == "legacy")
        st = P.ctx.bh_sort_stats()
    assert info[1] == info[2] == n_small
    if info[4] == kc.SORT_ONESWEEP:
        assert st["passes"] == 5
    elif info[4] == kc.SORT_TILES:
        assert st["passes"] == 0


@pytest.mark.parametrize("n", [kc.TILE + 1, kc.TILE + 1023, 3 * kc.TILE + 129])
def test_sharded_sequence_on_written_columns(n):
    """top_hist -> set_cutoff -> local_sort -> apply_sorted -> scatter on one rank: the compaction's counter is zeroed by a fill, not by
    k3_cutoff, and the survivors' number is read back from it"""
    import torch
    with Pass(n) as P:
        ctx = P.ctx
        for col in (kc.sparse(n, 901), kc.threshold(n, 902, -1), kc.zeros(n, 903, 0.4), kc.nan_pairs(n, 904, 0.05, 0)):
            kept_want = kc.cutoff(col.p, col.N)[1]
            qs = []
            for per in (0, 4):
                P.stages()
                P.write(col)
                ctx.debug_k3_tiles_per_group(per)
                ctx.bh_set_cutoff(ctx.bh_top_hist(), col.N)
                ctx.bh_local_sort()
                kept = ctx.n_sorted()
                assert kept == kept_want, (col.name, per)
                q_sorted = torch.empty(kept, dtype=torch.float64, device="cuda:0")
                ctx.bh_apply_sorted(ctx.device_ptr(2), kept, 0, 0.0, col.N, q_sorted.data_ptr())
                ctx.bh_scatter(q_sorted.data_ptr())
                qs.append(P.check(col, (col.name, n, "sharded", per)))
            assert _same(qs[0], qs[1])
        ctx.debug_k3_tiles_per_group(0)


def test_two_contexts_give_the_same_bits():
    n = 3 * kc.TILE + 127
    cols = [kc.threshold(n, 951, 0), kc.ties(n, 952, 0.45), kc.sparse(n, 953), kc.nothing_saturates(n, 954)]
    with Pass(n) as A, Pass(n) as B:
        for col in cols:
            qa, ia = A.run(col)
            qb, ib = B.run(col)
            assert ia == ib and bits_equal(np.nan_to_num(qa, nan=-1.0), np.nan_to_num(qb, nan=-1.0)), col.name


def test_pass_info_needs_a_bh_first():
    from fithic_amd import _capi
    with Pass(kc.TILE - 1) as P:
        with pytest.raises(_capi.FhxError) as e:
            P.ctx.k3_pass_info()
        assert e.value.code == _capi.FHX_ERR_ARG
