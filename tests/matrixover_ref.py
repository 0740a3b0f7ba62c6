"""Exact checker for matrixover (gdsp_genome_matrix, include/genodsp_hip.h): a literal loop over the cells.  A cell
(anchor, column j) is the bases p + s k, off_lo + j bin <= k < off_lo + (j+1) bin, that lie in the anchor's vector -- one
interval of it; its sample goes through xsum_ref.sample and its count, sum and mean through xsum_ref.stats, which computes
them exactly and rounds each once; min and max come from numpy, a zero made +0.0.

A genome is a list of numpy vectors; anchors are rows (vector index, position, strand +1 / -1), as in profileover_ref.

`figures` gives all five figures of every cell at once (tests share one pass between the figures).  A cell of one base has
nothing to add up, and `figures` does not send it through the exact sum unless literal=True: its figures are the value
itself with a zero made +0.0 (test_matrixover_ref.py holds the two forms together)."""
import math

import numpy as np

import xsum_ref as ref
from anchor_cases import anchors_array

DBL_MAX = ref.DBL_MAX
MAX_OFFSETS = 16384
FIGURES = ("mean", "sum", "count", "min", "max")              # GDSP_MATRIX_MEAN .. GDSP_MATRIX_MAX


def cell_interval(n, p, s, off_lo, bin, j):
    """[start, end) of the bases of column j of the anchor (p, s) in a vector of n; start >= end: none"""
    k_lo = off_lo + j * bin
    k_hi = k_lo + bin - 1
    g_lo, g_hi = (p + k_lo, p + k_hi) if s > 0 else (p - k_hi, p - k_lo)
    return max(g_lo, 0), min(g_hi, n - 1) + 1


def cell_figures(x):
    """(mean, sum, count, min, max) of an already sampled array"""
    f = ref.stats(x)
    if x.size == 0:
        return (math.nan, f[1], 0.0, math.nan, math.nan)
    return (f[2], f[1], f[0], float(np.min(x)) + 0.0, float(np.max(x)) + 0.0)


def figures(vectors, anchors, off_lo, noffsets, bin=1, lo=-DBL_MAX, hi=DBL_MAX, literal=False):
    """-> {figure: float64[nanchors, ncols]}"""
    assert 1 <= noffsets <= MAX_OFFSETS and bin >= 1 and noffsets % bin == 0
    a = anchors_array(anchors)
    ncols = noffsets // bin
    out = {k: np.empty((a.shape[0], ncols), np.float64) for k in FIGURES}
    vectors = [np.asarray(v, np.float64) for v in vectors]
    for i, (c, p, s) in enumerate(a.tolist()):
        v = vectors[c]
        assert 0 <= p < v.size, "an anchor outside its vector"
        row = []
        for j in range(ncols):
            start, end = cell_interval(v.size, p, s, off_lo, bin, j)
            if end - start == 1 and not literal:
                x = float(v[start])
                if math.isfinite(x) and not x < lo and not x > hi:
                    row.append((x + 0.0, x + 0.0, 1.0, x + 0.0, x + 0.0))
                else:
                    row.append((math.nan, 0.0, 0.0, math.nan, math.nan))
            else:
                row.append(cell_figures(ref.sample(v[start:end] if start < end else v[:0], 1, lo, hi)))
        for k, name in enumerate(FIGURES):
            out[name][i] = [f[k] for f in row]
    return out


def matrix(vectors, anchors, off_lo, noffsets, bin=1, what="mean", lo=-DBL_MAX, hi=DBL_MAX):
    """float64[nanchors, noffsets // bin] of one figure"""
    return figures(vectors, anchors, off_lo, noffsets, bin, lo, hi)[what]


def same_bits(a, b):
    """bit for bit, every NaN equal to every NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))
