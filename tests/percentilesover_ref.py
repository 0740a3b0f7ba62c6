"""CPU checker for percentilesover / medianover (numpy only): the definition of gdsp_interval_percentiles, computed
exactly.  Keys, their inverse and the rank rule are sliding_percentile_ref's (gdsp_key_of, gdsp_value_of,
gdsp_percentile_rank); an interval's sample is statsover's -- inside the limits and finite -- and its keys are sorted
with np.sort.  Also the Python formatter of the driver's table."""
import math

import numpy as np

from sliding_percentile_ref import key_of, rank, value_of

DBL_MAX = float(np.finfo(np.float64).max)


def sample_keys(v, s, e, lo=-DBL_MAX, hi=DBL_MAX):
    """the sorted keys of the sample of interval [s, e) of v"""
    x = np.ascontiguousarray(v[s:e], np.float64)
    with np.errstate(invalid="ignore"):
        keep = ~(x < lo) & ~(x > hi) & np.isfinite(x)
    return np.sort(key_of(x[keep]))


def interval_percentiles(v, start, end, ps, lo=-DBL_MAX, hi=DBL_MAX):
    """-> (count uint32[n], values float64[n, len(ps)]) for the intervals [start[i], end[i]) of v"""
    n = len(start)
    count = np.zeros(n, np.uint32)
    values = np.full((n, len(ps)), np.nan)
    for i in range(n):
        keys = sample_keys(v, int(start[i]), int(end[i]), lo, hi)
        m = keys.size
        count[i] = m
        if m:
            values[i] = value_of(keys[[rank(m, int(p)) for p in ps]])
    return count, values


def column_name(p):
    """'p' and what the percentile operator puts behind 'percentile' in its variable's name (percentile.c:756-780)"""
    if p % 1000 == 0:
        return "p%d" % (p // 1000)
    pct = float(np.float32(p) / np.float32(1000))
    precision, denom = 1, 100
    while denom >= 1:
        if p % denom == 0:
            return "p%.*f" % (precision, pct)
        precision, denom = precision + 1, denom // 10
    return "p%f" % pct


def format_value(x, precision=None):
    if math.isnan(x):
        return "NA"
    if precision is not None:
        return "%.*f" % (precision, x)
    if abs(x) < 1e15 and x == math.floor(x):
        return "%d" % int(x)
    return "%.17g" % x


def table(rows, ps, precision=None):
    """the driver's table: rows of (chrom, start, end, count, values) as the file names them"""
    lines = ["#chrom\tstart\tend\tcount" + "".join("\t" + column_name(int(p)) for p in ps)]
    for chrom, s, e, m, vals in rows:
        lines.append("\t".join([chrom, str(s), str(e), str(int(m))] + [format_value(float(x), precision) for x in vals]))
    return "".join(line + "\n" for line in lines)
