"""K2's division by a tabulated reciprocal (fhx_bdtrc.hpp: div_table_build, lean_quot), through the fhx_debug_table_div hook: a
workgroup builds the LDS table of refined reciprocals by integer j as the class kernels do and divides with the statement their
loops use.  Every j the two tables hold - j (j + 1) for the continued fractions, j for the power series - times 4096 numerators
must equal numpy's float64 division BIT FOR BIT, zeros and their signs included: every numerator is 0 or inside lean_div's window
[1e-200, 1e200], so no case is left out."""
import numpy as np
import pytest

from conftest import bits_equal

pytestmark = pytest.mark.gpu

M = 4096


@pytest.fixture(scope="module")
def ctx():
    from fithic_amd import _capi
    c = _capi.Context(0)
    yield c
    c.close()


def near_ties(divisor_of, table_len, m, rng):
    """numerators whose quotient by some divisor of the table lies next to a rounding tie: the double nearest to D (q + ulp / 2)
    for a representable q in [1, 2) - the exact tie is not a quotient of two doubles, its neighbours are"""
    out = np.empty(m, np.float64)
    for i in range(m):
        d = divisor_of(int(rng.integers(1, table_len)))
        k = int(rng.integers(0, 1 << 52))
        out[i] = float(d * ((1 << 53) + 2 * k + 1)) * 2.0 ** -53 * 2.0 ** int(rng.integers(-600, 600))
    return out


def numerators(divisor_of, table_len, seed):
    rng = np.random.default_rng(seed)
    parts = [
        np.array([0.0, -0.0, 1.0, -1.0, 1e-200, -1e-200, 1e200, -1e200]),
        2.0 ** np.arange(-664, 665, 8),                                                # powers of two inside the window
        -(2.0 ** np.arange(-660, 665, 8)),
        near_ties(divisor_of, table_len, 1024, rng),
        -near_ties(divisor_of, table_len, 512, rng),
    ]
    have = sum(len(p) for p in parts)
    rnd = 10.0 ** rng.uniform(-200, 200, M - have) * rng.choice([-1.0, 1.0], M - have)
    num = np.concatenate(parts + [rnd])
    assert len(num) == M and (((np.abs(num) >= 1e-200) & (np.abs(num) <= 1e200)) | (num == 0)).all()
    return num


@pytest.mark.parametrize("kind,divisor_of", [(0, lambda j: j * (j + 1)), (1, lambda j: j)], ids=["j_times_j_plus_1", "j"])
def test_table_division_is_ieee_division(ctx, kind, divisor_of):
    table_len = ctx.debug_table_div(kind, np.empty(0)).shape[0] + 1
    assert table_len >= 256                                      # the tables of fhx_bdtrc.hpp: kCfTabJ, kPsTabJ
    num = numerators(divisor_of, table_len, 77 + kind)
    got = ctx.debug_table_div(kind, num)
    j = np.arange(1, table_len, dtype=np.float64)
    d = j * (j + 1.0) if kind == 0 else j
    want = num[None, :] / d[:, None]
    assert got.shape == want.shape == (table_len - 1, M)
    assert np.isfinite(want).all() and (np.abs(want[want != 0]) > 1e-300).all()          # nothing near underflow by construction
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert len(bad) == 0, (len(bad), [(int(r) + 1, float(num[c]), float(got[r, c]), float(want[r, c])) for r, c in bad[:5]])
    assert bits_equal(got, want)
