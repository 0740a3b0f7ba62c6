"""CPU checker for breadthover (numpy only): the definition of gdsp_interval_breadth by boolean masks per interval.  An
interval's sample is statsover's -- inside the limits and finite --; a column counts the sampled bases with v >= T as IEEE
compares them (v > T when strict).  Also the Python formatter of the driver's table."""
import numpy as np

from percentilesover_ref import format_value

DBL_MAX = float(np.finfo(np.float64).max)


def interval_breadth(v, start, end, thresholds, strict=False, lo=-DBL_MAX, hi=DBL_MAX):
    """-> (count uint32[n], atleast uint32[n, len(thresholds)]) for the intervals [start[i], end[i]) of v"""
    n = len(start)
    ts = [float(t) for t in thresholds]
    count = np.zeros(n, np.uint32)
    atleast = np.zeros((n, len(ts)), np.uint32)
    for i in range(n):
        x = np.ascontiguousarray(v[int(start[i]):int(end[i])], np.float64)
        with np.errstate(invalid="ignore"):
            keep = ~(x < lo) & ~(x > hi) & np.isfinite(x)
            count[i] = int(keep.sum())
            for j, t in enumerate(ts):
                atleast[i, j] = int((keep & ((x > t) if strict else (x >= t))).sum())
    return count, atleast


def table(rows, labels, strict=False, fraction=False, precision=None):
    """the driver's table: rows of (chrom, start, end, count, atleast) as the file names them; labels: the thresholds as
    the user spelled them"""
    lines = ["#chrom\tstart\tend\tcount" + "".join("\t" + ("gt" if strict else "ge") + t for t in labels)]
    for chrom, s, e, m, cols in rows:
        if not fraction:
            figures = [str(int(c)) for c in cols]
        elif int(m) == 0:
            figures = ["NA"] * len(cols)
        else:
            figures = [format_value(float(int(c)) / float(int(m)), precision) for c in cols]
        lines.append("\t".join([chrom, str(s), str(e), str(int(m))] + figures))
    return "".join(line + "\n" for line in lines)
