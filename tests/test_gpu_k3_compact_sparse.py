"""k3_compact_sparse - the compaction of a pass whose q column holds 1.0 already and whose survivors are few: waves that work alone,
no block barrier in the tile loop, an LDS strip per workgroup - on p columns the test writes (tests/k3_columns.py), as
tests/test_gpu_k3_pass.py runs them: fhx_bh on the engine's own column, q of every row held bit for bit to the oracle's
Benjamini-Hochberg, fhx_n_sorted to the model's number of rows below the cutoff, and the variant the device chose read back
(Context.k3_pass_info()[8], fhx_k3_compact_variant: 0 not enqueued, 1 k3_compact<false> ran, 2 the sparse kernel ran).

Columns of 2 * 16 384 * per + 5 rows (per = tiles per workgroup, forced with fhx_debug_k3_tiles_per_group): whole groups of tiles
and a last group that is one partial tile of one partial wave; the row count is odd.  The device takes the sparse kernel when the
rows below the cutoff number at most groups * 1024 - half a strip per workgroup."""
import numpy as np
import pytest

import k3_columns as kc
from test_gpu_k3_pass import Pass, _same

pytestmark = pytest.mark.gpu

PERS = (2, 4)
NOT_ENQUEUED, PRESENT, SPARSE = 0, 1, 2


def rows_for(per):
    return 2 * kc.TILE * per + 5


def sparse_max(n, per):
    tiles = (n + kc.TILE - 1) // kc.TILE
    return (tiles + per - 1) // per * (kc.STRIP // 2)


def column(name, n, rows, seed, nan_rows=()):
    """small values at `rows`, NaN at `nan_rows`, every other row 1.0 or in [0.3, 1)"""
    rng = np.random.default_rng(seed)
    p = kc._big(rng, n)
    rows = np.asarray(rows, np.int64)
    p[rows] = kc._small(rng, len(rows))
    p[np.asarray(nan_rows, np.int64)] = np.nan
    col = kc.Column(name, p, kc.tests_for(n))
    assert kc.cutoff(col.p, col.N)[1] == len(np.setdiff1d(rows, nan_rows)), name
    return col


def columns(per):
    n = rows_for(per)
    group = kc.TILE * per
    rng = np.random.default_rng(77 + per)
    out = [column("no_survivor", n, [], 1),
           column("one_in_the_last_partial_wave", n, [n - 2], 2),
           column("last_row_alone", n, [n - 1], 3),
           column("one_full_wave", n, np.arange(5 * kc.CHUNK, 6 * kc.CHUNK), 4)]
    # CP_STRIP + 1 survivors in the first workgroup's tiles: one wave with 700, the rest scattered; a few in the other groups
    first = np.concatenate([np.arange(2 * kc.CHUNK + 100, 2 * kc.CHUNK + 800), rng.choice(np.arange(3 * kc.CHUNK, group), kc.STRIP + 1 - 700, replace=False)])
    others = np.concatenate([group + rng.choice(group, 40, replace=False), [n - 5, n - 1]])
    out.append(column("strip_plus_one_in_a_workgroup", n, np.concatenate([first, others]), 5))
    out.append(column("strip_exactly_full_in_a_workgroup", n, np.concatenate([first[:-1], others]), 6))
    # NaN beside kept and beside unkept rows, both members of a pair; a whole chunk of NaN; the last row of the odd count
    kept = rng.choice(n - 1, 300, replace=False)
    pair = kept ^ 1
    nan = np.concatenate([pair[:100], rng.choice(np.setdiff1d(np.arange(n), np.concatenate([kept, pair])), 200, replace=False),
                          np.arange(7 * kc.CHUNK, 8 * kc.CHUNK), [n - 1]])
    out.append(column("nan_among_kept_and_unkept", n, kept, 7, nan_rows=np.setdiff1d(nan, kept)))
    m = sparse_max(n, per)
    out.append(column("fraction_just_under", n, rng.choice(n, m, replace=False), 8))
    out.append(column("fraction_just_over", n, rng.choice(n, m + 1, replace=False), 9))
    return out


NAMES = [c.name for c in columns(PERS[0])]


@pytest.fixture(scope="module", params=PERS)
def setup(request):
    per = request.param
    with Pass(rows_for(per)) as P:
        P.ctx.debug_k3_tiles_per_group(per)
        P.stages()                                   # the context's first pass_stats does not fill q yet: every later one does
        yield per, P, {c.name: c for c in columns(per)}


def run(P, col, fresh=True):
    if fresh:
        P.stages()
    P.write(col)
    P.ctx.bh(col.N)
    q = P.check(col, (col.name, P.n, "prefilled" if fresh else "not prefilled"))
    info = P.ctx.k3_pass_info()
    print(col.name, P.n, "k3_pass_info", info)
    kept = kc.cutoff(col.p, col.N)[1]
    assert P.ctx.n_sorted() == kept and info[1] == kept and info[2] == kept, (col.name, info, kept)
    P.last = (P.n, info[1])
    return q, info


@pytest.mark.parametrize("name", NAMES)
def test_sparse_compaction_on_written_columns(setup, name):
    per, P, cols = setup
    col = cols[name]
    assert len(col.p) == 2 * kc.TILE * per + 5 and len(col.p) & 1
    q, info = run(P, col)
    kept = kc.cutoff(col.p, col.N)[1]
    assert info[3] == per and info[6] == 1 and info[0] in (0, 1)
    assert info[8] == (SPARSE if kept <= sparse_max(P.n, per) else PRESENT), (name, per, info)
    assert info[8] == (PRESENT if name == "fraction_just_over" else SPARSE)
    # the same column once more on a q column that is not prefilled (it holds the q just written): the kernel there was runs alone
    q2, info = run(P, col, fresh=False)
    assert info[6] == 0 and info[8] == NOT_ENQUEUED and _same(q, q2)
