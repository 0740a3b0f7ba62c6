"""CPU: the checker of breadthover (tests/breadthover_ref.py) held to a literal loop of the definition in
include/genodsp_hip.h on the data kinds of the library's tests, and to what the definition says about planted NaN,
infinities and out-of-limit bases, about strict against nextafter, and about the two zeros."""
import math

import numpy as np
import pytest

import breadthover_ref as ref
from test_percentilesover import data

DBL_MAX = ref.DBL_MAX
KINDS = ["depth", "equal", "real", "small", "sprinkled"]


def literal(v, s, e, ts, strict, lo=-DBL_MAX, hi=DBL_MAX):
    """the definition, one base at a time"""
    m, cols = 0, [0] * len(ts)
    for i in range(s, e):
        x = float(v[i])
        if (x < lo) or (x > hi) or not math.isfinite(x):
            continue
        m += 1
        for j, t in enumerate(ts):
            if (x > t) if strict else (x >= t):
                cols[j] += 1
    return m, cols


def thresholds_of(x):
    fin = x[np.isfinite(x)]
    return [float(fin[3]), float(np.median(fin)), 0.0, -0.0, math.inf, -math.inf, DBL_MAX, -DBL_MAX, float(fin[3]), 7.0, 1.0]


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_the_checker_is_the_literal_definition(kind, strict):
    x = data(kind, 700, seed=len(kind))
    ts = thresholds_of(x)
    rng = np.random.default_rng(5)
    start = np.concatenate([[0, 0, 699, 100], rng.integers(0, 650, 30)]).astype(np.uint32)
    end = np.concatenate([[700, 1, 700, 101], start[4:] + 1 + rng.integers(0, 50, 30)]).astype(np.uint32)
    for lo, hi in ((-DBL_MAX, DBL_MAX), (-1e299, 1e299), (0.0, 10.0), (-0.0, 0.0)):
        count, atleast = ref.interval_breadth(x, start, end, ts, strict, lo, hi)
        assert count.dtype == np.uint32 and atleast.dtype == np.uint32 and atleast.shape == (start.size, len(ts))
        for i in range(start.size):
            m, cols = literal(x, int(start[i]), int(end[i]), ts, strict, lo, hi)
            assert (int(count[i]), atleast[i].tolist()) == (m, cols), (kind, strict, lo, hi, i)


@pytest.mark.parametrize("strict", [False, True])
def test_planted_bases_count_in_no_column(strict):
    """NaN, infinities and values beyond the limits are not in the sample: an interval of them is 0 in every column, and
    planting them among others changes nothing but the count of what is left"""
    ts = [-math.inf, -1e300, 0.0, 5.0, 1e300, math.inf]
    bad = np.array([np.nan, -np.nan, np.inf, -np.inf, 1e300, -1e300] * 5)
    count, atleast = ref.interval_breadth(bad, [0, 3], [bad.size, 4], ts, strict, -1e299, 1e299)
    assert count.tolist() == [0, 0] and not atleast.any()
    good = np.arange(-10.0, 20.0)
    mixed = np.empty(good.size + bad.size)
    mixed[::2], mixed[1::2] = good, bad
    c0, a0 = ref.interval_breadth(good, [0], [good.size], ts, strict, -1e299, 1e299)
    c1, a1 = ref.interval_breadth(mixed, [0], [mixed.size], ts, strict, -1e299, 1e299)
    assert int(c0[0]) == int(c1[0]) == good.size and np.array_equal(a0, a1)
    assert int(a0[0, 0]) == good.size and int(a0[0, -1]) == 0                    # T = -inf: the sample; T = +inf: nothing
    # without limits +-1e300 are sampled, the infinities and NaN still are not
    c2, a2 = ref.interval_breadth(bad, [0], [bad.size], ts, strict)
    assert int(c2[0]) == 10 and a2[0].tolist() == ([10, 5, 5, 5, 0, 0] if strict else [10, 10, 5, 5, 5, 0])


@pytest.mark.parametrize("kind", KINDS)
def test_strict_is_the_next_double(kind):
    """v > T is v >= nextafter(T, +inf) for finite T"""
    x = data(kind, 500, seed=2)
    fin = x[np.isfinite(x)]
    ts = [float(fin[0]), float(fin[1]), 0.0, -0.0, 5e-324, -5e-324, 7.0, -DBL_MAX, 1.0]
    up = [float(np.nextafter(t, np.inf)) for t in ts]
    start, end = np.array([0, 17, 250], np.uint32), np.array([500, 400, 251], np.uint32)
    c0, a0 = ref.interval_breadth(x, start, end, ts, True)
    c1, a1 = ref.interval_breadth(x, start, end, up, False)
    assert np.array_equal(c0, c1) and np.array_equal(a0, a1)
    assert up[2] == up[3] == 5e-324                                              # the two zeros are one threshold


def test_the_two_zeros_are_equal():
    x = np.array([-0.0, 0.0, -5e-324, 5e-324, -0.0, 1.0, -1.0])
    count, atleast = ref.interval_breadth(x, [0], [x.size], [0.0, -0.0], False)
    assert int(count[0]) == 7 and atleast[0].tolist() == [5, 5]                  # -0.0 >= 0.0
    count, atleast = ref.interval_breadth(x, [0], [x.size], [0.0, -0.0], True)
    assert atleast[0].tolist() == [2, 2]                                         # and neither zero is above the other


def test_the_table():
    rows = [("chrA", 5, 50, 45, [45, 9, 0]), ("chrB", 0, 7, 0, [0, 0, 0]), ("chrA", 1, 4, 3, [3, 1, 1])]
    assert ref.table(rows, ["1", "1e1", "mean"]) == ("#chrom\tstart\tend\tcount\tge1\tge1e1\tgemean\nchrA\t5\t50\t45\t45\t9\t0\n"
                                                      "chrB\t0\t7\t0\t0\t0\t0\nchrA\t1\t4\t3\t3\t1\t1\n")
    got = ref.table(rows, ["1", "1e1", "mean"], strict=True, fraction=True)
    assert got == ("#chrom\tstart\tend\tcount\tgt1\tgt1e1\tgtmean\nchrA\t5\t50\t45\t1\t0.20000000000000001\t0\n"
                   "chrB\t0\t7\t0\tNA\tNA\tNA\nchrA\t1\t4\t3\t1\t0.33333333333333331\t0.33333333333333331\n")
    assert ref.table(rows[:1], ["1", "1e1", "mean"], fraction=True, precision=3).endswith("\t45\t1.000\t0.200\t0.000\n")
