"""The checker for `histogram` (numpy and the standard library only): the edge table, the words and the driver's table
as include/genodsp_hip.h and genodsp_amd/host/ops_histogram.c define them.  Everything is integers or printed bytes."""
from fractions import Fraction

import numpy as np

import xsum_ref

DBL_MAX = xsum_ref.DBL_MAX


def uniform_edges(lo, width, bins):
    """e[k] = lo + k*width rounded once (a correctly rounded fma: the exact rational turned into a float)"""
    lo, width = Fraction(float(lo)), Fraction(float(width))
    e = []
    for k in range(int(bins) + 1):
        try:
            e.append(float(Fraction(k) * width + lo))
        except OverflowError:
            e.append(float("inf") if Fraction(k) * width + lo > 0 else float("-inf"))
    return np.array(e, np.float64)


def table_ok(edges):
    e = np.asarray(edges, np.float64)
    return bool(2 <= e.size <= 65537 and np.all(np.isfinite(e)) and np.all(e[:-1] < e[1:]))


def words_of_sample(x, edges):
    """the B + 3 words of an already sampled array: bins, below, above, n"""
    e = np.asarray(edges, np.float64)
    B = e.size - 1
    x = np.asarray(x, np.float64)
    k = np.searchsorted(e, x, side="right") - 1               # e[k] <= x < e[k+1]; -1 below, B at or above e[B]
    inside = (k >= 0) & (k < B)
    w = np.zeros(B + 3, np.uint64)
    w[:B] = np.bincount(k[inside], minlength=B).astype(np.uint64)
    w[B] = int((k < 0).sum())
    w[B + 1] = int((k >= B).sum())
    w[B + 2] = x.size
    return w


def words(vectors, edges, window=1, lo=-DBL_MAX, hi=DBL_MAX, firsts=None):
    """the words of a genome given as vectors (vector i starts at chromosome position firsts[i], default 0)"""
    firsts = firsts if firsts is not None else [0] * len(vectors)
    parts = [xsum_ref.sample(v, window, lo, hi, f) for v, f in zip(vectors, firsts)]
    return words_of_sample(np.concatenate(parts or [np.empty(0)]), edges)


def table_text(w, edges, precision=None):
    """what the driver prints for the words w"""
    e = np.asarray(edges, np.float64)
    B = e.size - 1
    below, above, n = int(w[B]), int(w[B + 1]), int(w[B + 2])
    edge = (lambda v: "%.17g" % v) if precision is None else (lambda v: "%.*f" % (precision, v))
    lines = ["# count %d" % n, "# below %d" % below, "# above %d" % above, "#lo\thi\tcount\tfraction\tatleast"]
    at_least = n - below
    for k in range(B):
        c = int(w[k])
        if n == 0:
            lines.append("%s\t%s\t%d\tNA\tNA" % (edge(e[k]), edge(e[k + 1]), c))
        else:
            lines.append("%s\t%s\t%d\t%.17g\t%.17g" % (edge(e[k]), edge(e[k + 1]), c, c / n, at_least / n))
        at_least -= c
    return "\n".join(lines) + "\n"


def mode_of(w, edges):
    """the lower edge of the fullest bin (lowest on ties); None when no bin holds anything"""
    B = len(edges) - 1
    if int(np.asarray(w[:B], np.uint64).sum()) == 0:
        return None
    return float(edges[int(np.argmax(w[:B]))])
