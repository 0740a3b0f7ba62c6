"""The per-interval checker of correlateover (tests/correlateover_ref.py) held to a literal fractions.Fraction loop on tiny
intervals, to correlate's checker on an interval that is the whole vector, and to planted answers.  No GPU."""
import math
from fractions import Fraction

import numpy as np

import correlate_ref as cref
import correlateover_ref as ref

DBL_MAX = ref.DBL_MAX


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))


def literal(x, y, s, e, lo, hi, ylo, yhi):
    """the definition, base by base: Fractions for the sums, Python floats (one IEEE operation each) for the rest"""
    pairs = [(float(a), float(b)) for a, b in zip(x[s:e], y[s:e])
             if not a < lo and not a > hi and math.isfinite(a) and not b < ylo and not b > yhi and math.isfinite(b)]
    n = len(pairs)
    if n == 0:
        return (0,) + (math.nan,) * 8
    meanx = float(sum(Fraction(a) for a, _ in pairs) / n)
    meany = float(sum(Fraction(b) for _, b in pairs) / n)
    sxx = sxy = syy = Fraction(0)
    for a, b in pairs:
        dx, dy = a - meanx, b - meany
        sxx += Fraction(dx * dx)
        syy += Fraction(dy * dy)
        sxy += Fraction(dx * dy)
    varx, vary, cov = float(sxx / n), float(syy / n), float(sxy / n)
    sdx, sdy = math.sqrt(varx), math.sqrt(vary)
    r = slope = intercept = math.nan
    if varx > 0 and vary > 0:
        (mx, ex), (my, ey) = math.frexp(sdx), math.frexp(sdy)
        r = max(-1.0, min(1.0, math.ldexp(cov, -(ex + ey)) / (mx * my)))
    if varx > 0:
        slope = cov / varx
        intercept = meany - slope * meanx
    return (n, meanx, meany, sdx, sdy, cov, r, slope, intercept)


def test_the_checker_is_the_literal_definition_on_tiny_intervals():
    rng = np.random.default_rng(5)
    n = 60
    kinds = {"depth": (rng.integers(0, 9, n).astype(np.float64), rng.integers(0, 5, n).astype(np.float64)),
             "real": (rng.standard_normal(n) * 10 + 2, rng.standard_normal(n) * 3 - 1),
             "wide": (rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n), rng.standard_normal(n) * 10.0 ** rng.integers(-9, 9, n))}
    checked = 0
    for name, (x, y) in kinds.items():
        x, y = x.copy(), y.copy()
        x[7], y[11], x[30], y[31] = math.nan, math.inf, -math.inf, math.nan
        for lo, hi, ylo, yhi in ((-DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX), (0.5, 7.0, -DBL_MAX, 3.0), (-DBL_MAX, DBL_MAX, 0.25, DBL_MAX)):
            for _ in range(14):
                s = int(rng.integers(0, n - 1))
                e = min(n, s + 1 + int(rng.integers(0, 12)))
                want = literal(x, y, s, e, lo, hi, ylo, yhi)
                got = ref.interval(x, y, s, e, lo, hi, ylo, yhi)
                assert got[0] == want[0] and all(same(a, b) for a, b in zip(got[1:], want[1:])), (name, s, e, got, want)
                checked += 1
    assert checked > 100
    assert len(ref.FIGURES) == 9 and ref.interval(x, y, 7, 8)[0] == 0           # x[7] is NaN: an empty sample


def test_a_whole_vector_interval_is_correlates_genome():
    rng = np.random.default_rng(8)
    x, y = rng.standard_normal(5000) * 4 + 1, rng.standard_normal(5000)
    y += 0.5 * x
    x[100], y[200] = math.nan, math.inf
    for kw in ({}, {"lo": 0.0, "hi": 6.0}, {"ylo": -0.5}):
        whole = dict(zip(cref.FIGURES, cref.genome([(x, y)], 1, **kw)))
        got = dict(zip(ref.FIGURES, ref.interval(x, y, 0, x.size, **kw)))
        for mine, theirs in zip(ref.FIGURES, ref._FROM):
            assert same(float(got[mine]), float(whole[theirs])), (kw, mine)
        assert 0.5 < got["correlation"] < 1.0
    out = ref.interval_correlation(x, y, [0, 10], [x.size, 20])
    assert out["count"].dtype == np.uint32 and out["count"].tolist() == [4998, 10] and same(out["slope"][0], ref.interval(x, y, 0, x.size)[7])


def test_planted_answers():
    x = np.arange(1, 41, dtype=np.float64)
    fig = dict(zip(ref.FIGURES, ref.interval(x, 2 * x + 3, 5, 30)))
    assert fig["count"] == 25 and fig["correlation"] == 1.0 and fig["slope"] == 2.0 and fig["intercept"] == 3.0
    assert fig["mean"] == 18.0 and fig["filemean"] == 39.0 and fig["filestddev"] == 2 * fig["stddev"]
    fig = dict(zip(ref.FIGURES, ref.interval(x, -x, 0, 40)))
    assert fig["correlation"] == -1.0 and fig["slope"] == -1.0 and fig["intercept"] == 0.0
    # a constant track: its variance is 0, so there is no correlation; the regression on x is the flat line
    fig = dict(zip(ref.FIGURES, ref.interval(x, np.full(40, 7.0), 3, 9)))
    assert fig["filestddev"] == 0.0 and fig["covariance"] == 0.0 and math.isnan(fig["correlation"]) and fig["slope"] == 0.0 and fig["intercept"] == 7.0
    # a constant signal: nothing to regress on
    fig = dict(zip(ref.FIGURES, ref.interval(np.full(40, 7.0), x, 3, 9)))
    assert fig["stddev"] == 0.0 and all(math.isnan(fig[k]) for k in ("correlation", "slope", "intercept"))
    # products that overflow: a variance of +inf and, where a crossed product is not finite, no covariance
    big = np.array([1e200, -1e200, 1e200, -1e200])
    fig = dict(zip(ref.FIGURES, ref.interval(big, big, 0, 4)))
    assert fig["stddev"] == math.inf and fig["filestddev"] == math.inf and math.isnan(fig["covariance"]) and math.isnan(fig["correlation"])
    # the table's text
    text = ref.table([("chr1", 5, 9, (0,) + (math.nan,) * 8), ("chr2", 0, 4, (4, 2.0, 0.5, 1e-3, math.inf, -0.25, 1.0, 2.0, 3.0))], None)
    assert text.splitlines()[0] == ref.HEADER and text.splitlines()[1] == "chr1\t5\t9\t0" + "\tNA" * 8
    assert text.splitlines()[2] == "chr2\t0\t4\t4\t2\t0.5\t0.001\tinf\t-0.25\t1\t2\t3"
    assert ref.table([("c", 1, 2, (1, 2.0, 0.5, 0.0, 0.0, 0.0, math.nan, math.nan, math.nan))], 2).splitlines()[1] == "c\t1\t2\t1\t2.00\t0.50\t0.00\t0.00\t0.00\tNA\tNA\tNA"
