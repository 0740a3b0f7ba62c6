"""Run-length arithmetic for piecewise-constant signals: what the genome-wide reductions (percentile, stats, histogram,
correlate, crosscorrelate) must return for a signal given as runs [(length, value), ...], without ever building the
vector -- so that the answer for 2^32 - 1 bases costs a handful of Fractions.  Every figure follows the definition in
include/genodsp_hip.h operation by operation: the per-base roundings (fl(v - mean), the products) are single numpy
float64 operations on the run's value, the sums are exact rationals (a run of L bases adds L times its term), and each
result is rounded once.  tests/test_stepsignal_ref.py holds every function here to the array checkers (xsum_ref,
histogram_ref, correlate_ref, lagcorr_ref, sliding_percentile_ref.rank) on short vectors.  Standard library and numpy."""
import math
from fractions import Fraction

import numpy as np

import correlate_ref as cref
from sliding_percentile_ref import rank
from xsum_ref import round_ratio

f64 = np.float64


def from_intervals(n, intervals):
    """runs of the vector of n zeros after apply_intervals has added val over each [start, end): [(length, value), ...].
    The values are added in the order given, as the operator adds them (exact for the dyadic values the tests plant)"""
    cuts = sorted(set([0, n] + [p for a, z, _ in intervals for p in (a, z) if 0 <= p <= n]))
    runs = []
    for a, z in zip(cuts[:-1], cuts[1:]):
        v = f64(0.0)
        for s, e, x in intervals:
            if s <= a and z <= e:
                v = v + f64(x)
        runs.append((z - a, float(v)))
    return merge(runs)


def merge(runs):
    out = []
    for length, v in runs:
        if length <= 0:
            continue
        if out and out[-1][1] == v:
            out[-1] = (out[-1][0] + length, v)
        else:
            out.append((length, v))
    return out


def length(runs):
    return sum(length for length, _ in runs)


def to_array(runs):
    return np.concatenate([np.full(length, v, np.float64) for length, v in runs])


def multiset(runs):
    """sorted [(value, count)]"""
    counts = {}
    for length, v in runs:
        counts[v] = counts.get(v, 0) + length
    return sorted(counts.items())


def percentile(runs, p_thousandths):
    """the value of rank gdsp_percentile_rank(n, p) among the n values, ascending"""
    k = rank(length(runs), p_thousandths)
    for v, c in multiset(runs):
        if k < c:
            return v
        k -= c
    raise AssertionError("rank beyond the multiset")


def minmax(runs):
    ms = multiset(runs)
    return ms[0][0], ms[-1][0]


def _round(q):
    """a Fraction rounded once"""
    return round_ratio(q.numerator, q.denominator)


def stats(runs):
    """(count, sum, mean, variance, stddev) as gdsp_genome_stats defines them"""
    n = length(runs)
    total = sum(Fraction(v) * c for v, c in multiset(runs))
    mean = _round(total / n)
    sq = Fraction(0)
    for v, c in multiset(runs):
        d = f64(v) - f64(mean)                                           # fl(v - mean), then fl(d d)
        sq += Fraction(float(d * d)) * c
    var = _round(sq / n)
    return float(n), _round(total), mean, var, math.sqrt(var)


def histogram_words(runs, edges):
    """bins, below, above, n: as histogram_ref.words_of_sample"""
    e = np.asarray(edges, np.float64)
    B = e.size - 1
    w = [0] * (B + 3)
    for v, c in multiset(runs):
        k = int(np.searchsorted(e, v, side="right")) - 1
        w[B if k < 0 else (B + 1 if k >= B else k)] += c
    w[B + 2] = length(runs)
    return w


def at_least(words):
    """the table's `atleast` column as counts: the values at or above each bin's lower edge (histogram_ref.table_text)"""
    B = len(words) - 3
    out, left = [], words[B + 2] - words[B]
    for k in range(B):
        out.append(left)
        left -= words[k]
    return out


def pairs_of(xruns, yruns, shift=0):
    """[(count, x value, y value)] over the bases i where x[i] and y[i + shift] both exist"""
    n = length(xruns)
    assert length(yruns) == n

    def cuts(runs, move):
        out, at = [], 0
        for length_, v in runs:
            out.append((at - move, at + length_ - move, v))                 # the run covers x positions [a, z)
            at += length_
        return out

    lo, hi = max(0, -shift), min(n, n - shift)
    xs, ys = cuts(xruns, 0), cuts(yruns, shift)
    out, i, j = [], 0, 0
    while i < len(xs) and j < len(ys):
        a, z = max(xs[i][0], ys[j][0], lo), min(xs[i][1], ys[j][1], hi)
        if z > a:
            out.append((z - a, xs[i][2], ys[j][2]))
        if xs[i][1] <= ys[j][1]:
            i += 1
        else:
            j += 1
    return out


def correlation(xruns, yruns):
    """the 13 figures of correlate_ref.FIGURES"""
    pairs = pairs_of(xruns, yruns)
    n = sum(c for c, _, _ in pairs)
    sx = sum(Fraction(x) * c for c, x, _ in pairs)
    sy = sum(Fraction(y) * c for c, _, y in pairs)
    meanx, meany = _round(sx / n), _round(sy / n)
    qxx = qyy = qxy = Fraction(0)
    for c, x, y in pairs:
        dx, dy = f64(x) - f64(meanx), f64(y) - f64(meany)
        qxx += Fraction(float(dx * dx)) * c
        qyy += Fraction(float(dy * dy)) * c
        qxy += Fraction(float(dx * dy)) * c
    varx, vary, cov = _round(qxx / n), _round(qyy / n), _round(qxy / n)
    sdx, sdy = math.sqrt(varx), math.sqrt(vary)
    return (float(n), _round(sx), _round(sy), meanx, meany, varx, vary, sdx, sdy, cov) + \
        tuple(cref.derived(cov, varx, vary, sdx, sdy, meanx, meany))


def lag_curve(xruns, yruns, lag_lo, nlags):
    """(figures, pairs per lag, covariance per lag, correlation per lag) as lagcorr_ref.curve: per lag d the sum of
    fl(fl(x[i] - meanx) * fl(y[i + d] - meany)), exact, over N (the count of the figures) and rounded once"""
    fig = correlation(xruns, yruns)
    f = dict(zip(cref.FIGURES, fig))
    n = int(f["count"])
    counts, cov, corr = [], [], []
    for k in range(int(nlags)):
        pairs = pairs_of(xruns, yruns, int(lag_lo) + k)
        total = Fraction(0)
        for c, x, y in pairs:
            total += Fraction(float((f64(x) - f64(f["meanx"])) * (f64(y) - f64(f["meany"])))) * c
        counts.append(sum(c for c, _, _ in pairs))
        cov.append(_round(total / n))
        corr.append(cref.derived(cov[-1], f["varx"], f["vary"], f["sdx"], f["sdy"], f["meanx"], f["meany"])[0])
    return fig, counts, cov, corr


# ---------------------------------------------------------------------------------- the signals the tests share ----

def step_intervals(n, q1, q2, q3, extremes):
    """four levels with steps at q1 < q2 < q3, and single bases planted on top: the intervals to hand apply_intervals"""
    levels = [(0, q1, 1.5), (q1, q2, -2.25), (q2, q3, 7.0), (q3, n, 0.5)]
    return levels + [(p, p + 1, x) for p, x in extremes]


def halves_intervals(n, h, extremes):
    return [(0, h, 3.0), (h, n, -1.25)] + [(p, p + 1, x) for p, x in extremes]


def interval_figures(runs, a, z):
    """statsover's figures of the bases [a, z): (count, sum, mean, min, max, maxpos), maxpos the first base of the maximum"""
    at, total, count, lo, hi, where = 0, Fraction(0), 0, None, None, -1
    for length_, v in runs:
        s, e = max(at, a), min(at + length_, z)
        if s < e:
            total += Fraction(v) * (e - s)
            count += e - s
            lo = v if lo is None or v < lo else lo
            if hi is None or v > hi:
                hi, where = v, s
        at += length_
    return count, _round(total), _round(total / count), lo + 0.0, hi + 0.0, where
