"""Writes tests/golden/f16_bdtrc_tail.npz and .json: chosen (count, total, prior) rows for the relative bar on p-values
(tests/p_relative.py) - for each total, each outcome of k2_rows.outcome and each band of the EXACT binomial tail down to the
subnormal range and below it, at least 16 rows wherever the cell can be reached.  CPU only; needs mpmath (1.3.0) and scipy (1.15.3).

    python tests/golden/make_golden_bdtrc_tail.py

Columns: count, total, prior; exact (the tail by direct summation in 60-digit arithmetic, as a double) and exact_log10 (for values
below the double range; -inf for 0); scipy = scipy.special.bdtrc(count - 1, int(total), prior), live - NaN for the rows of the
wide total 7150761687, which scipy would narrow to a negative C int: there the oracle's wide mode takes scipy's place.

The JSON lists the cells no candidate reaches, and per cell the reference's own error against `exact` (a record, not a bar: the
truncated continued fraction is the answer) and the spread of the bar."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository root (oracle/)

import mpmath as mp                                           # noqa: E402
import scipy.special                                          # noqa: E402

import k2_rows as kr                                          # noqa: E402
import p_relative as pr                                       # noqa: E402

mp.mp.dps = 60
PER_CELL = 18                  # rows kept per cell (the tests ask for pr.FIXTURE_PER_CELL = 16)
LOOSE_PER_CELL = 2             # of which at most this many with a bar above pr.TIGHT relative (counts above total / 1e6 at the large totals)
CANDIDATES = 60                # candidates per cell that get the exact sum
COUNTS = (1, 2, 3, 4, 5, 8, 13, 21, 34, 55, 89, 126, 127, 128, 129, 144, 150, 160, 168, 169, 170, 171, 233, 377, 610, 800, 1022, 1023,
          1024, 1500, 2000, 3000, 4000, 5000)


def exact_tail(count, total, prior):
    """P(X >= count) for X ~ Binomial(total, prior): (value as mpf, log10 or -inf).  Terms from loggamma, then the ratio recurrence
    term(j + 1) / term(j) = (n - j) / (j + 1) * x / (1 - x): upward from `count` when count >= n x, else the complement downward."""
    k, n, x = int(count), int(total), mp.mpf(float(prior))
    if k <= 0 or x == 1:
        return mp.mpf(1), 0.0
    if x == 0:
        return mp.mpf(0), -np.inf
    if k == 1:
        p = -mp.expm1(n * mp.log1p(-x))
    else:
        q = 1 - x
        odds = x / q

        def term(j):
            return mp.exp(mp.loggamma(n + 1) - mp.loggamma(j + 1) - mp.loggamma(n - j + 1) + j * mp.log(x) + (n - j) * mp.log(q))

        if k >= n * x:
            t = term(k)
            s, j = t, k
            while j < n:
                t = t * (n - j) / (j + 1) * odds
                s += t
                j += 1
                if t < s * mp.mpf(10) ** -70:
                    break
            p = s
        else:
            j = k - 1
            t = term(j)
            s = t
            while j > 0:
                t = t * j / (n - j + 1) / odds
                s += t
                j -= 1
                if t < s * mp.mpf(10) ** -70:
                    break
            p = 1 - s
    return p, (float(mp.log10(p)) if p > 0 else -np.inf)


def candidates(total, rng):
    """(count, prior) over every outcome of the total and, for the power series, incbcf and the local closed form, down the tail"""
    n = float(total)
    cs, ps = [], []

    def add(c, pri):
        pri = np.asarray(pri, np.float64)
        pri = pri[(pri > 0.0) & (pri < 1.0)]
        cs.extend([c] * len(pri))
        ps.extend(pri.tolist())

    spread = np.unique(np.clip(np.floor(10.0 ** rng.uniform(0.3, np.log10(5000.0), 40)), 2, 5000)).astype(int)
    for c in sorted(set(COUNTS) | set(spread.tolist())):
        if c > n:
            continue
        if c == 1:
            add(1, 10.0 ** -rng.uniform(2.0, 323.0, 700))                   # local closed form: p ~ n * prior, every band
            add(1, 10.0 ** -rng.uniform(300.0, 323.3, 300))                 # ... densely where n * prior is subnormal
            add(1, np.concatenate([rng.uniform(0.01, 0.999, 60), 1.0 - 10.0 ** -rng.uniform(1, 12, 20), [0.01, 0.5]]))
            continue
        base = c / n
        deep = min(340.0 / c + 1.0, 322.0)
        add(c, base * 10.0 ** -rng.uniform(0.0, deep, 260))                  # observed > expected: down the tail (incbcf, power series)
        add(c, 10.0 ** -rng.uniform(np.log10(max(n, 10.0)), 322.0, 120))     # bb * x <= 1: the power series, any depth
        add(c, base * 10.0 ** rng.uniform(0.0, 3.0, 24))                     # observed < expected: the swapped classes
        add(c, 1.0 - 10.0 ** -rng.uniform(0.3, 12.0, 12))
        add(c, (c - 1.0 + rng.uniform(0.02, 0.98, 40)) / n)                  # between (k - 1) / (n - 1) and k / (n + 1): incbd
    return np.array(cs, np.int32), np.array(ps, np.float64)


def pre_band(o):
    """where the reference's value puts a candidate (it is within 1e-5 of the exact tail; 0 below 5e-324)"""
    with np.errstate(divide="ignore"):
        return pr.fixture_band(np.where(o > 0.0, np.log10(np.where(o > 0.0, o, 1.0)), -np.inf))


def choose(total, rng):
    mode = pr.fixture_totals_mode(total)
    cnt, pri = candidates(total, rng)
    order = rng.permutation(len(cnt))
    cnt, pri = cnt[order], pri[order]
    o, S, bar = pr.reference(cnt, total, pri, mode)
    oc = kr.outcome(cnt, total, pri)
    pb = pre_band(o)
    with np.errstate(invalid="ignore", divide="ignore"):
        loose = (np.abs(o) >= pr.MIN_NORMAL) & (bar / np.abs(o) > pr.TIGHT)
    rows, unreachable = [], []
    for w in pr.FIXTURE_OUTCOMES:
        for b in range(len(pr.FIXTURE_BANDS)):
            idx = np.flatnonzero((oc == w) & (pb == b) & ~np.isnan(o))
            # round robin over the counts, so that a cell is not sixteen rows of one count
            nth = np.zeros(len(idx), np.int64)
            seen = {}
            for j, i in enumerate(idx):
                nth[j] = seen.get(int(cnt[i]), 0)
                seen[int(cnt[i])] = nth[j] + 1
            idx = idx[np.argsort(nth, kind="stable")][:CANDIDATES]
            kept_tight, kept_loose = [], []
            for i in idx:
                p, lg = exact_tail(cnt[i], total, pri[i])
                if pr.fixture_band(lg) != b:
                    continue
                (kept_loose if loose[i] else kept_tight).append((int(i), float(p), lg))
            kept = kept_tight[:PER_CELL - min(LOOSE_PER_CELL, len(kept_loose))]
            kept += kept_loose[:PER_CELL - len(kept)]
            if len(kept) < pr.FIXTURE_PER_CELL and len(kept_tight) + len(kept_loose) >= pr.FIXTURE_PER_CELL:
                kept = (kept_tight + kept_loose)[:PER_CELL]
            if len(kept) < pr.FIXTURE_PER_CELL:
                unreachable.append(pr.cell_name(total, w, b))
                continue
            rows += [(int(cnt[i]), float(total), float(pri[i]), p, lg) for i, p, lg in kept]
    # rows kept whatever the draw: count 1 under priors so small that n * prior is a small multiple of 2^-53 (1e-12 at 1e6: a "more
    # accurate" formula differs from the reference by 1e-10 relative there), and the counts around K2_TB_COUNTS and K2H_KCAP
    forced = [(1, x) for x in (1e-12, 1e-13, 1e-15, 2.0 ** -40, 2.0 ** -53 / float(total))]
    forced += [(c, c / float(total) / 8.0) for c in (2, 3, 126, 127, 128, 129, 1022, 1023, 1024, 5000) if c <= total]
    have = {(r[0], r[2]) for r in rows}
    for c, x in forced:
        if (c, x) not in have:
            p, lg = exact_tail(c, total, x)
            rows.append((c, float(total), float(x), float(p), lg))
    # rows outside the six outcomes: the NaN pattern and the constants (count 0, count = total + 1, count beyond, prior NaN / above 1)
    t = int(total)
    for c, x, p in ((0, 0.3, 1.0), (t + 1, 0.3, 0.0), (t + 2, 0.3, np.nan), (2, np.nan, np.nan), (2, 1.5, np.nan), (1, np.nan, np.nan),
                    (3, 0.0, 0.0), (3, 1.0, 1.0)):
        if c <= 2 ** 20:
            rows.append((c, float(total), x, p, float(np.log10(p)) if p > 0 else (-np.inf if p == 0 else np.nan)))
    return rows, unreachable


def main():
    rng = np.random.default_rng(16)
    rows, unreachable = [], []
    for total in pr.FIXTURE_TOTALS:
        r, u = choose(total, rng)
        rows += r
        unreachable += u
        print("total %d: %d rows, %d cells not reached" % (total, len(r), len(u)))
    cols = dict(count=np.array([r[0] for r in rows], np.int32), total=np.array([r[1] for r in rows], np.float64),
                prior=np.array([r[2] for r in rows], np.float64), exact=np.array([r[3] for r in rows], np.float64),
                exact_log10=np.array([r[4] for r in rows], np.float64))
    ref_mode = cols["total"] < 2.0 ** 31
    sp = np.full(len(rows), np.nan)
    sp[ref_mode] = scipy.special.bdtrc(cols["count"][ref_mode] - 1.0, cols["total"][ref_mode].astype(np.int64), cols["prior"][ref_mode])
    cols["scipy"] = sp

    # cross-check of the summation: 50 rows of the small totals against the regularised incomplete beta function
    small = np.flatnonzero((cols["total"] <= 5000.0) & (cols["count"] >= 2) & (cols["count"] <= cols["total"]) & (cols["exact"] > 0) & (cols["exact"] < 1))
    for i in rng.choice(small, 50, replace=False):
        k, n, x = int(cols["count"][i]), int(cols["total"][i]), mp.mpf(float(cols["prior"][i]))
        want = mp.betainc(k, n - k + 1, 0, x, regularized=True)
        got, _ = exact_tail(k, n, float(x))
        assert abs(got - want) <= abs(want) * mp.mpf(10) ** -40, (k, n, float(x), got, want)

    o = np.empty(len(rows))
    S = np.empty(len(rows))
    for mode, sel in (("reference", ref_mode), ("wide", ~ref_mode)):
        o[sel], S[sel], _ = pr.reference(cols["count"][sel], cols["total"][sel], cols["prior"][sel], mode)
    same = (o.view(np.int64) == sp.view(np.int64)) | (np.isnan(o) & np.isnan(sp))
    assert same[ref_mode].all(), "the oracle must reproduce scipy bit for bit"
    cells = pr.fixture_cells(cols)
    record = {name: pr.cell_record(o[idx], S[idx], cols["exact"][idx]) for name, idx in sorted(cells.items())}
    in_cells = np.concatenate(list(cells.values()))
    normal = in_cells[np.abs(o[in_cells]) >= pr.MIN_NORMAL]
    rel = pr.bar_of(o, S)[normal] / np.abs(o[normal])
    meta = {"rows": len(rows), "rows_in_cells": int(len(in_cells)), "per_cell_min": pr.FIXTURE_PER_CELL, "unreachable": sorted(unreachable),
            "normal_rows": int(len(normal)), "share_bar_le_1e-9": float((rel <= pr.TIGHT).mean()),
            "share_bar_le_1e-9_below_1e-10": float((rel[o[normal] < 1e-10] <= pr.TIGHT).mean()),
            "share_p_below_1e-10": float((o[normal] < 1e-10).mean()), "cells": record}
    np.savez_compressed(os.path.join(HERE, "f16_bdtrc_tail.npz"), **cols)
    with open(os.path.join(HERE, "f16_bdtrc_tail.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d rows in %d cells, %d cells not reached; bar <= 1e-9 on %.4f of %d normal rows; reference vs exact: up to %.3g relative" % (
        len(rows), len(cells), len(unreachable), meta["share_bar_le_1e-9"], len(normal),
        max(v["ref_rel_err_max"] or 0.0 for v in record.values())))


if __name__ == "__main__":
    main()
