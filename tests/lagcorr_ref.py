"""Exact numpy checker for crosscorrelate / autocorrelate (gdsp_genome_lag_correlation, include/genodsp_hip.h): the
figures of the sample where x and y are both finite from correlate_ref.figures, the lagged products with numpy (the two
centrings and the product, one IEEE operation each), their sums as Python ints (xsum_ref.exact_int) rounded once by
round_ratio, and the correlation derived as correlate_ref.derived spells it.  A genome is a list of (x, y) pairs of whole
chromosome vectors."""
import math

import numpy as np

import correlate_ref as cref
import xsum_ref as ref
from xsum_ref import SCALE, exact_int, round_ratio, same          # noqa: F401  (same: for the tests)

FIGURES = cref.FIGURES
WORDS = 72


def figures(pairs):
    """the 13 figures of the bases where x and y are both finite (window 1, no limits)"""
    return cref.genome([(np.asarray(x, np.float64), np.asarray(y, np.float64)) for x, y in pairs])


def sums(pairs, lag_lo, nlags, meanx, meany):
    """per lag lag_lo + k: (products taken, the exact sum of the finite ones times 2^1074 as an int, those not finite)"""
    prepared = []
    with np.errstate(all="ignore"):
        for x, y in pairs:
            x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
            assert x.size == y.size
            prepared.append((x - np.float64(meanx), y - np.float64(meany), np.isfinite(x), np.isfinite(y)))
    out = []
    for k in range(int(nlags)):
        d = int(lag_lo) + k
        taken, bad, finite = 0, 0, []
        for dx, dy, fx, fy in prepared:
            L = dx.size
            i0, i1 = max(0, -d), min(L, L - d)                  # 0 <= i < L and 0 <= i + d < L
            if i1 <= i0:
                continue
            both = fx[i0:i1] & fy[i0 + d:i1 + d]
            with np.errstate(all="ignore"):
                p = (dx[i0:i1] * dy[i0 + d:i1 + d])[both]
            fin = np.isfinite(p)
            taken += int(p.size)
            bad += int((~fin).sum())
            finite.append(p[fin])
        out.append((taken, exact_int(np.concatenate(finite)) if finite else 0, bad))
    return out


def words_of(M, count=0, bad=0):
    """the canonical image of the exact sum M 2^-1074 (as xsum_ref.image), with its count and INF words"""
    w = np.zeros(WORDS, np.uint64)
    for k in range(67):
        w[k] = (M >> (32 * k)) & 0xFFFFFFFF
    w[67] = np.uint64((M >> (32 * 67)) & 0xFFFFFFFFFFFFFFFF)
    w[68], w[69] = count, bad
    return w


def images(pairs, lag_lo, nlags, meanx, meany):
    """what gdsp_lag_products_batch leaves: np.uint64[nlags, 72] (words 70 and 71 are not the checker's to say)"""
    return np.stack([words_of(M, n, bad) for n, M, bad in sums(pairs, lag_lo, nlags, meanx, meany)])


def curve(pairs, lag_lo, nlags):
    """(figures, pairs per lag, covariance per lag, correlation per lag)"""
    fig = figures(pairs)
    f = dict(zip(FIGURES, fig))
    N = int(f["count"])
    nlags = int(nlags)
    if N == 0:
        return fig, [0] * nlags, [math.nan] * nlags, [math.nan] * nlags
    counts, cov, corr = [], [], []
    for n, M, bad in sums(pairs, lag_lo, nlags, f["meanx"], f["meany"]):
        c = math.nan if bad else round_ratio(M, N << SCALE)
        counts.append(n)
        cov.append(c)
        corr.append(cref.derived(c, f["varx"], f["vary"], f["sdx"], f["sdy"], f["meanx"], f["meany"])[0])
    return fig, counts, cov, corr


def best(lags, corr):
    """(bestlag, bestcorrelation, mincorrelation): the lag of the largest correlation that is not NaN, ties to the
    smaller |lag|, then the smaller lag; None when every correlation is NaN"""
    seen = [(c, d) for d, c in zip(lags, corr) if not math.isnan(c)]
    if not seen:
        return None
    top = max(c for c, _ in seen)
    d = min((abs(d), d) for c, d in seen if c == top)[1]
    return d, top, min(c for c, _ in seen)
