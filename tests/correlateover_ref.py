"""CPU checker for correlateover (gdsp_interval_correlation, include/genodsp_hip.h): an interval's figures are correlate's
for the interval's pair sample, so this is a thin wrapper around correlate_ref.pair_sample and correlate_ref.figures (exact
sums in Python ints, every figure rounded once or derived operation by operation).  Also the Python formatter of the
driver's table."""
import math

import numpy as np

import correlate_ref as cref
from xsum_ref import DBL_MAX

FIGURES = ("count", "mean", "filemean", "stddev", "filestddev", "covariance", "correlation", "slope", "intercept")
_FROM = ("count", "meanx", "meany", "sdx", "sdy", "covariance", "correlation", "slope", "intercept")      # of correlate_ref.FIGURES
HEADER = "#chrom\tstart\tend\tcount\tmean\tfilemean\tstddev\tfilestddev\tcovariance\tcorrelation\tslope\tintercept"


def interval(x, y, s, e, lo=-DBL_MAX, hi=DBL_MAX, ylo=-DBL_MAX, yhi=DBL_MAX):
    """the nine figures of interval [s, e) of the pair (x, y), in FIGURES' order; count as an int"""
    with np.errstate(invalid="ignore"):
        fig = dict(zip(cref.FIGURES, cref.figures(*cref.pair_sample(x[int(s):int(e)], y[int(s):int(e)], 1, lo, hi, ylo, yhi))))
    return (int(fig["count"]),) + tuple(float(fig[k]) for k in _FROM[1:])


def interval_correlation(x, y, start, end, lo=-DBL_MAX, hi=DBL_MAX, ylo=-DBL_MAX, yhi=DBL_MAX):
    """-> dict of arrays (count uint32, the rest float64) for the intervals [start[i], end[i]) of the pair (x, y)"""
    rows = [interval(x, y, s, e, lo, hi, ylo, yhi) for s, e in zip(start, end)]
    out = {"count": np.array([r[0] for r in rows], np.uint32)}
    for j, name in enumerate(FIGURES[1:], 1):
        out[name] = np.array([r[j] for r in rows], np.float64)
    return out


def format_value(x, precision=None):
    """a figure as the driver prints it"""
    if math.isnan(x):
        return "NA"
    if precision is not None:
        return "%.*f" % (precision, x)
    if abs(x) < 1e15 and x == math.floor(x) and not (x == 0 and math.copysign(1.0, x) < 0):
        return "%d" % int(x)
    return "%.17g" % x


def table(rows, precision=None):
    """the driver's table: rows of (chrom, start, end, figures) as the file names them, figures in FIGURES' order"""
    lines = [HEADER]
    for chrom, s, e, fig in rows:
        lines.append("\t".join([chrom, str(s), str(e), str(int(fig[0]))] + [format_value(float(v), precision) for v in fig[1:]]))
    return "".join(line + "\n" for line in lines)
