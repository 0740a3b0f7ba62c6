"""Exact numpy checker for correlate (gdsp_genome_correlation, include/genodsp_hip.h): the pair sample's sums, means,
variances and covariance computed exactly and rounded once -- numpy for the per-pair roundings (fl(x - meanx) and the
three products, each one IEEE operation), Python ints for the sums (xsum_ref.exact_int) -- and the correlation, slope
and intercept derived from them in plain double, operation by operation as the header spells them."""
import math

import numpy as np

import xsum_ref as ref
from xsum_ref import DBL_MAX, SCALE, exact_int, round_ratio, same          # noqa: F401  (same: for the tests)

FIGURES = ("count", "sumx", "sumy", "meanx", "meany", "varx", "vary", "sdx", "sdy", "covariance", "correlation", "slope",
           "intercept")


def pair_sample(x, y, window=1, lo=-DBL_MAX, hi=DBL_MAX, ylo=-DBL_MAX, yhi=DBL_MAX, first=0):
    """The pairs correlate looks at: every window-th base counted from the chromosome's first (x[0] is base `first`)
    whose x is within lo, hi and whose y is within ylo, yhi, neither NaN nor +-inf."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    assert x.size == y.size
    idx = np.arange(x.size, dtype=np.int64) + int(first)
    keep = (idx % int(window) == 0) & ~(x < lo) & ~(x > hi) & np.isfinite(x) & ~(y < ylo) & ~(y > yhi) & np.isfinite(y)
    return x[keep], y[keep]


def products(x, y, meanx, meany):
    """qxx, qyy, qxy of an already sampled pair of arrays: each two or three roundings, no fma"""
    with np.errstate(all="ignore"):
        dx, dy = x - np.float64(meanx), y - np.float64(meany)
        return dx * dx, dy * dy, dx * dy


def derived(cov, varx, vary, sdx, sdy, meanx, meany):
    """(correlation, slope, intercept) from the once-rounded figures"""
    f = np.float64
    xok = varx > 0 and math.isfinite(varx)
    yok = vary > 0 and math.isfinite(vary)
    cok = not math.isnan(cov)
    r = slope = intercept = math.nan
    with np.errstate(all="ignore"):
        if xok and yok and cok:
            mx, ex = math.frexp(sdx)
            my, ey = math.frexp(sdy)
            r = float(f(math.ldexp(cov, -(ex + ey))) / (f(mx) * f(my)))
            r = max(-1.0, min(1.0, r))
        if xok and cok:
            slope = float(f(cov) / f(varx))
            intercept = float(f(meany) - f(slope) * f(meanx))
    return r, slope, intercept


def figures(x, y):
    """The 13 figures, in FIGURES' order, of an already sampled pair of arrays."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = int(x.size)
    Mx, My = exact_int(x), exact_int(y)
    out = [float(n), round_ratio(Mx, 1 << SCALE), round_ratio(My, 1 << SCALE)] + [math.nan] * 10
    if n == 0:
        return tuple(out)
    meanx, meany = round_ratio(Mx, n << SCALE), round_ratio(My, n << SCALE)
    qxx, qyy, qxy = products(x, y, meanx, meany)
    varx = math.inf if not np.isfinite(qxx).all() else round_ratio(exact_int(qxx), n << SCALE)
    vary = math.inf if not np.isfinite(qyy).all() else round_ratio(exact_int(qyy), n << SCALE)
    cov = math.nan if not np.isfinite(qxy).all() else round_ratio(exact_int(qxy), n << SCALE)
    sdx, sdy = math.sqrt(varx), math.sqrt(vary)
    out[3:10] = [meanx, meany, varx, vary, sdx, sdy, cov]
    out[10:13] = derived(cov, varx, vary, sdx, sdy, meanx, meany)
    return tuple(out)


def genome(pairs, window=1, lo=-DBL_MAX, hi=DBL_MAX, ylo=-DBL_MAX, yhi=DBL_MAX):
    """figures of a genome given as (x, y) pairs of whole chromosome vectors"""
    s = [pair_sample(x, y, window, lo, hi, ylo, yhi) for x, y in pairs]
    return figures(np.concatenate([a for a, _ in s] or [np.empty(0)]), np.concatenate([b for _, b in s] or [np.empty(0)]))


def images(x, y, means=None):
    """the canonical images of one pass over an already sampled pair of arrays (np.uint64[k, 72], k = 2 or 3): what
    gdsp_xsum_fold leaves of each, with the q that are not finite counted in word 69 and left out"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    terms = (x, y) if means is None else products(x, y, means[0], means[1])
    out = []
    for t in terms:
        fin = np.isfinite(t)
        w = ref.image(t[fin])
        w[68] = x.size
        w[69] = int((~fin).sum())
        out.append(w)
    return np.stack(out)
