"""A relative bar for p-values: faithfulness to the oracle, row by row, sized by what the oracle's own arithmetic lets a
different libm change (oracle/cephes_libm_nudge.c: Cephes' bdtrc with log, exp and pow one ulp high / one ulp low).

    bar = 2 S + 4 * 2^-52 * |o| + u

o   the oracle's value (bit for bit scipy.special.bdtrc, tests/test_p_relative_inputs.py),
S   max(|up - o|, |down - o|) of the two nudged builds (oracle.fithic_oracle.bdtrc_libm_spread),
2   two libms that are each within one ulp of the true function value lie within two ulp of each other; the nudge measures one,
4   ulp of o for second-order effects in the few IEEE operations that follow the last libm call,
u   2 * 2^-1074 where o, o - S or o + S is subnormal or zero (there an ulp of o says nothing), 0 elsewhere.

None of the numbers comes from a device.  The exact binomial tail is NOT the yardstick: Cephes itself is up to 3e-6 relative away
from it at Hi-C sized totals (tests/golden/f16_bdtrc_tail.json keeps that record).  Not a conftest; no GPU here."""
import numpy as np

import k2_rows as kr

ULP = 2.0 ** -52
MIN_NORMAL = 2.2250738585072014e-308
TINY_U = 2.0 * 5e-324
BAND_NAMES = (">=1e-10", "1e-40..1e-10", "1e-150..1e-40", "normal<1e-150", "subnormal", "zero")
TIGHT = 1e-9                                    # "a bar with teeth": the share of rows whose bar is at most this, relative


def band_of(v):
    """band of a p-value by its size (NaN: -1)"""
    v = np.abs(np.asarray(v, np.float64))
    with np.errstate(invalid="ignore"):
        b = np.select([v >= 1e-10, v >= 1e-40, v >= 1e-150, v >= MIN_NORMAL, v > 0.0, v == 0.0], [0, 1, 2, 3, 4, 5], -1)
    return b.astype(np.int32)


# ---- the fixture of chosen rows, tests/golden/f16_bdtrc_tail.npz (made by tests/golden/make_golden_bdtrc_tail.py) -------------
FIXTURE_TOTALS = (170.0, 171.0, 5000.0, 1.0e6, 645040870.0, 7150761687.0)        # the last one in the wide mode only
FIXTURE_OUTCOMES = (kr.PSERIES, kr.CF_BCF, kr.CF_BD, kr.CF_SWAPPED, kr.CLOSED_POW, kr.CLOSED_LOCAL)
FIXTURE_BANDS = ("1e-10..1", "1e-40..1e-10", "1e-150..1e-40", "1e-300..1e-150", "subnormal", "below1e-330")
FIXTURE_PER_CELL = 16
LOG10_MIN_NORMAL, LOG10_MIN_SUBNORMAL = -307.6526555685888, -323.3062153431158       # 2^-1022, 2^-1074


def fixture_band(exact_log10):
    """band of the EXACT tail by its log10 (-1: between the bands, e.g. a normal value below 1e-300)"""
    v = np.asarray(exact_log10, np.float64)
    with np.errstate(invalid="ignore"):
        b = np.select([v >= -10.0, v >= -40.0, v >= -150.0, v >= -300.0, (v >= LOG10_MIN_SUBNORMAL) & (v < LOG10_MIN_NORMAL), v < -330.0],
                      [0, 1, 2, 3, 4, 5], -1)
    return b.astype(np.int32)


def fixture_totals_mode(total):
    return "wide" if total >= 2.0 ** 31 else "reference"


def cell_name(total, outcome, band):
    return "%d/%s/%s" % (int(total), kr.OUTCOME_NAMES[int(outcome)], FIXTURE_BANDS[int(band)])


def load_fixture():
    """(columns, meta) of f16_bdtrc_tail: count, total, prior, exact, exact_log10, scipy per row"""
    import json
    import os
    g = np.load(os.path.join(kr.GOLDEN, "f16_bdtrc_tail.npz"))
    with open(os.path.join(kr.GOLDEN, "f16_bdtrc_tail.json")) as f:
        meta = json.load(f)
    return {k: g[k] for k in g.files}, meta


def fixture_cells(cols):
    """{cell name: row indices} of the rows of the six outcomes"""
    out = {}
    oc = kr.outcome(cols["count"], cols["total"], cols["prior"])
    band = fixture_band(cols["exact_log10"])
    for i in np.flatnonzero((oc != kr.TRIVIAL) & (band >= 0)):
        out.setdefault(cell_name(cols["total"][i], oc[i], band[i]), []).append(int(i))
    return {k: np.array(v) for k, v in out.items()}


def cell_record(o, S, exact):
    """what the JSON keeps per cell: the reference's own error against the exact tail (a record, not a bar) and the bar's spread"""
    bar = bar_of(o, S)
    normal = np.abs(exact) >= MIN_NORMAL
    rec = {"rows": int(len(o)), "ref_abs_err_max": float(np.max(np.abs(o - exact))), "ref_rel_err_max": None, "bar_rel": None,
           "bar_abs_max": float(bar.max())}
    if normal.any():
        rec["ref_rel_err_max"] = float(np.max(np.abs(o[normal] - exact[normal]) / np.abs(exact[normal])))
    onorm = np.abs(o) >= MIN_NORMAL
    if onorm.any():
        rel = bar[onorm] / np.abs(o[onorm])
        rec["bar_rel"] = {"median": float(np.median(rel)), "p99": float(np.percentile(rel, 99)), "max": float(rel.max())}
    return rec


def bar_of(o, S):
    """the bar per row (NaN where o is NaN)"""
    o = np.asarray(o, np.float64)
    S = np.asarray(S, np.float64)
    a = np.abs(o)
    with np.errstate(invalid="ignore"):
        tiny = (a < MIN_NORMAL) | (np.abs(o - S) < MIN_NORMAL) | (np.abs(o + S) < MIN_NORMAL)
    return 2.0 * S + 4.0 * ULP * a + np.where(tiny, TINY_U, 0.0)


def reference(count, total, prior, totals="reference"):
    """(o, S, bar) for integer counts: bdtrc(count - 1, total, prior) of the oracle and of its nudged builds"""
    from oracle import fithic_oracle as fo
    count = np.asarray(count)
    prior = np.ascontiguousarray(prior, np.float64)
    total = np.ascontiguousarray(np.broadcast_to(np.asarray(total, np.float64), prior.shape))
    o, S = fo.bdtrc_libm_spread(count.astype(np.float64) - 1.0, total, prior, totals)
    return o, S, bar_of(o, S)


def _effective_total(total, totals):
    """the total as bdtrc's arithmetic sees it (k2_rows.outcome takes that one): narrowed to a C int in reference mode"""
    if totals != "reference":
        return total
    t = np.asarray(total, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(t) < 2.0 ** 52, np.mod(t + 2.0 ** 31, 2.0 ** 32) - 2.0 ** 31, t)      # fithic_oracle.int_narrowed, exact in doubles


class Table:
    """per (K2 outcome, band of the oracle's p): rows, share bit-identical, largest |got - o| / bar"""

    def __init__(self, cells, n_rows, n_same, worst):
        self.cells, self.n_rows, self.n_same, self.worst = cells, n_rows, n_same, worst

    def per_outcome(self):
        out = {}
        for (oc, _), (n, same, w) in self.cells.items():
            a = out.setdefault(oc, [0, 0, 0.0])
            a[0], a[1], a[2] = a[0] + n, a[1] + same, max(a[2], w)
        return {k: (v[0], v[1] / v[0], v[2]) for k, v in out.items()}

    def __str__(self):
        lines = ["%-13s %-15s %7s %14s %18s" % ("outcome", "band of p", "rows", "bit-identical", "max |got-o|/bar")]
        for (oc, b), (n, same, w) in sorted(self.cells.items(), key=lambda kv: (kr.OUTCOME_NAMES.index(kv[0][0]), BAND_NAMES.index(kv[0][1]))):
            lines.append("%-13s %-15s %7d %13.2f%% %18.3g" % (oc, b, n, 100.0 * same / n, w))
        for oc, (n, share, w) in sorted(self.per_outcome().items(), key=lambda kv: kr.OUTCOME_NAMES.index(kv[0])):
            lines.append("%-13s %-15s %7d %13.2f%% %18.3g" % (oc, "all", n, 100.0 * share, w))
        lines.append("%-13s %-15s %7d %13.2f%% %18.3g" % ("all", "all", self.n_rows, 100.0 * self.n_same / max(self.n_rows, 1), self.worst))
        return "\n".join(lines)


def check_p_faithful(got, count, total, prior, totals="reference"):
    """(message or None, Table): what assert_p_faithful asserts, without raising"""
    got = np.ascontiguousarray(got, np.float64)
    count = np.ascontiguousarray(count)
    prior = np.ascontiguousarray(prior, np.float64)
    total = np.ascontiguousarray(np.broadcast_to(np.asarray(total, np.float64), prior.shape))
    assert got.shape == count.shape == prior.shape and got.ndim == 1
    o, S, bar = reference(count, total, prior, totals)
    outcome = kr.outcome(count, _effective_total(total, totals), prior)

    def row(i):
        return "count %d prior %r total %r: got %r, oracle %r, S %.3g, bar %.3g, %s" % (
            int(count[i]), float(prior[i]), float(total[i]), float(got[i]), float(o[i]), float(S[i]), float(bar[i]), kr.OUTCOME_NAMES[int(outcome[i])])

    msg = None
    nan_differs = np.flatnonzero(np.isnan(got) != np.isnan(o))
    if len(nan_differs):
        msg = "NaN pattern differs from the oracle's on %d rows:\n  %s" % (len(nan_differs), "\n  ".join(row(i) for i in nan_differs[:5]))
    live = ~np.isnan(o) & ~np.isnan(got)
    with np.errstate(invalid="ignore", over="ignore"):
        ratio = np.where(live, np.abs(got - o) / bar, 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)               # an infinite got
    over = np.flatnonzero(ratio > 1.0)
    if msg is None and len(over):
        worst = over[np.argsort(-ratio[over], kind="stable")[:5]]
        msg = "%d of %d rows are further from the oracle than 2 S + 4 ulp + u; the worst:\n  %s" % (
            len(over), int(live.sum()), "\n  ".join("%s, |got - o| / bar %.3g" % (row(i), ratio[i]) for i in worst))
    same = live & (got.view(np.int64) == o.view(np.int64))
    cells = {}
    bands = band_of(o)
    for oc in np.unique(outcome[live]):
        for b in np.unique(bands[live & (outcome == oc)]):
            m = live & (outcome == oc) & (bands == b)
            cells[(kr.OUTCOME_NAMES[int(oc)], BAND_NAMES[int(b)])] = (int(m.sum()), int(same[m].sum()), float(ratio[m].max()))
    return msg, Table(cells, int(live.sum()), int(same.sum()), float(ratio.max()) if len(ratio) else 0.0)


def assert_p_faithful(got, count, total, prior, totals="reference", what=""):
    """got against the oracle's bdtrc(count - 1, total, prior), row by row: the NaN pattern equals the oracle's, and every other
    row lies within 2 S + 4 * 2^-52 |o| + u of it (module docstring).  total: one number or one per row.  On failure the five
    worst rows are reported with count, prior, total, got, o, S and the K2 outcome (k2_rows.outcome).  Returns the Table."""
    msg, table = check_p_faithful(got, count, total, prior, totals)
    assert msg is None, "%s: %s" % (what, msg) if what != "" else msg
    return table


def assert_pass_p_faithful(got, count, r, totals="reference", what=""):
    """a whole pass of the oracle (PassResult r): rows that reach bdtrc carry the bar through r.prior / r.bdtrc_n, the others keep
    the reference's p = 1 exactly"""
    got = np.ascontiguousarray(got, np.float64)
    reach = ~np.isnan(r.bdtrc_n)
    assert np.array_equal(got[~reach], r.p[~reach]) and (r.p[~reach] == 1.0).all(), what
    return assert_p_faithful(got[reach], np.asarray(count)[reach], r.bdtrc_n[reach], r.prior[reach], totals, what)
