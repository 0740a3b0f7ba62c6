"""Exact numpy checker for stats / normalize (gdsp_genome_stats, include/genodsp_hip.h): the sample's sum, mean and
variance computed exactly, each rounded once, without np.sum.

Every finite double is m * 2^e with an integer m < 2^53.  The mantissas are cut into halves of 26 and 27 bits and added
in int64 per exponent (np.add.reduceat over the values sorted by exponent), and the per-exponent totals are combined as
Python ints: the exact sum is an int M times 2^-1074.  Python's int / int true division is correctly rounded, so
M / 2^1074 and M / (n 2^1074) are the sum and the mean rounded once; an OverflowError there means the rounded value is
beyond DBL_MAX, which is checked against the rounding threshold 2^1024 - 2^970 before it is read as +-inf."""
import math

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
SCALE = 1074                                   # the exact sum is an integer times 2^-1074
HALF = 26


def sample(v, window=1, lo=-DBL_MAX, hi=DBL_MAX, first=0):
    """The values stats looks at: every window-th base counted from the chromosome's first (v[0] is base `first`) with
    lo <= x <= hi, never NaN or +-inf."""
    v = np.asarray(v, np.float64)
    idx = np.arange(v.size, dtype=np.int64) + int(first)
    keep = (idx % int(window) == 0) & ~(v < lo) & ~(v > hi) & np.isfinite(v)
    return v[keep]


def exact_int(x):
    """sum(x) * 2^1074 exactly, as a Python int (x finite)."""
    x = np.asarray(x, np.float64)
    if x.size == 0:
        return 0
    m, e = np.frexp(x)                                   # x = m 2^e, 0.5 <= |m| < 1
    mi = np.ldexp(m, 53).astype(np.int64)                # exact: |mi| < 2^53
    ex = e.astype(np.int64) - 53 + SCALE                 # x = mi 2^(ex - 1074), ex >= 0
    low = ex < 0                                         # subnormals: mi has as many trailing zeros
    mi[low] >>= -ex[low]
    ex[low] = 0
    order = np.argsort(ex, kind="stable")
    mi, ex = mi[order], ex[order]
    hi = mi >> HALF                                      # floor: mi = hi 2^26 + lo, 0 <= lo < 2^26
    lo = mi - (hi << HALF)
    starts = np.flatnonzero(np.concatenate(([True], ex[1:] != ex[:-1])))
    shi = np.add.reduceat(hi, starts)                    # |hi| < 2^27: 2^36 of them still fit
    slo = np.add.reduceat(lo, starts)
    total = 0
    for s_hi, s_lo, k in zip(shi.tolist(), slo.tolist(), ex[starts].tolist()):
        total += ((s_hi << HALF) + s_lo) << k
    return total


def round_ratio(num, den):
    """num / den rounded once to nearest-even (den > 0), +-inf beyond DBL_MAX, -0.0 for a negative value that rounds
    to zero, +0.0 for an exact zero."""
    if num == 0:
        return 0.0
    try:
        return num / den
    except OverflowError:
        # the rounded value is beyond DBL_MAX: |num / den| >= DBL_MAX + half an ulp = 2^1024 - 2^970
        assert abs(num) >= ((1 << 1024) - (1 << 970)) * den
        return math.inf if num > 0 else -math.inf


def stats(x):
    """(count, sum, mean, variance, stddev) of an already sampled array, as gdsp_genome_stats defines them."""
    x = np.asarray(x, np.float64)
    n = int(x.size)
    M = exact_int(x)
    total = round_ratio(M, 1 << SCALE)
    if n == 0:
        return (0.0, total, math.nan, math.nan, math.nan)
    mean = round_ratio(M, n << SCALE)
    with np.errstate(over="ignore", invalid="ignore"):
        d = x - mean                                     # fl(v - mean), then fl(d * d): two roundings, no fma
        q = d * d
    if np.isposinf(q).any():
        var = math.inf
    else:
        var = round_ratio(exact_int(q), n << SCALE)
    return (float(n), total, mean, var, math.sqrt(var))


def genome(vectors, window=1, lo=-DBL_MAX, hi=DBL_MAX):
    """stats of a genome given as whole chromosome vectors"""
    return stats(np.concatenate([sample(v, window, lo, hi) for v in vectors] or [np.empty(0)]))


def same(a, b):
    """bit for bit, NaN equal to NaN"""
    a, b = float(a), float(b)
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def image(x):
    """the canonical accumulator image of a sample (GDSP_XSUM_WORDS words: 68 digits of 32 bits, the top one signed;
    count) -- what gdsp_xsum_fold leaves, as np.uint64"""
    M = exact_int(x)
    words = np.zeros(72, np.uint64)
    for k in range(67):
        words[k] = (M >> (32 * k)) & 0xFFFFFFFF
    words[67] = np.uint64((M >> (32 * 67)) & 0xFFFFFFFFFFFFFFFF)
    words[68] = np.asarray(x).size
    return words
