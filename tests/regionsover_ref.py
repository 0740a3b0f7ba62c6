"""Exact checker for regionsover (gdsp_genome_regions, include/genodsp_hip.h): a literal loop over the cells, in Python
integers.  A row has U // bin + B + D // bin columns in the region's own direction; column j of the region [s, e) of L
bases on the plus strand is
    upstream    [s - U + j bin, s - U + (j+1) bin)
    body k      [s + k L // B, s + (k+1) L // B)
    downstream  [e + j bin, e + (j+1) bin)
and on the minus strand the mirror image about the region: the column that holds the offsets [a, z) from the region's
first base in its own direction is [s + a, s + z) on the plus strand and [e - z, e - a) on the minus strand.  Flank cells
are cut to [0, n); a region is never cut.  Each cell's sample goes through xsum_ref.sample and its count, sum and mean
through xsum_ref.stats, which computes them exactly and rounds each once; min and max come from numpy, a zero made +0.0
-- matrixover_ref.cell_figures.

A genome is a list of numpy vectors; regions are rows (vector index, start, end, strand +1 / -1), zero-based half-open."""
import numpy as np

import matrixover_ref as mref
import xsum_ref as ref

DBL_MAX = ref.DBL_MAX
MAX_COLUMNS = 16384
FIGURES = mref.FIGURES
same_bits = mref.same_bits


def columns(U, B, D, bin):
    assert 1 <= B <= MAX_COLUMNS and 0 <= U <= MAX_COLUMNS and 0 <= D <= MAX_COLUMNS and bin >= 1 and U % bin == 0 and D % bin == 0
    ncols = U // bin + B + D // bin
    assert ncols <= MAX_COLUMNS
    return ncols


def cell_interval(n, s, e, strand, U, B, D, bin, j):
    """[start, end) of the bases of column j of the region [s, e) in a vector of n; start >= end: none"""
    assert 0 <= s < e <= n
    ncols = columns(U, B, D, bin)
    assert 0 <= j < ncols
    L = e - s
    n_up = U // bin
    if j < n_up:                                         # offsets [a, z) from the region's first base, in its direction
        a, z = -U + j * bin, -U + (j + 1) * bin
    elif j < n_up + B:
        k = j - n_up
        a, z = (k * L) // B, ((k + 1) * L) // B
    else:
        k = j - n_up - B
        a, z = L + k * bin, L + (k + 1) * bin
    lo, hi = (s + a, s + z) if strand > 0 else (e - z, e - a)      # minus: the mirror image about the region
    return max(lo, 0), min(hi, n)


def figures(vectors, regions, B, U=0, D=0, bin=1, lo=-DBL_MAX, hi=DBL_MAX):
    """-> {figure: float64[nregions, ncols]}"""
    ncols = columns(U, B, D, bin)
    a = np.asarray(regions, dtype=np.int64).reshape(-1, 4)
    out = {k: np.empty((a.shape[0], ncols), np.float64) for k in FIGURES}
    vectors = [np.asarray(v, np.float64) for v in vectors]
    for i, (c, s, e, strand) in enumerate(a.tolist()):
        v = vectors[c]
        row = []
        for j in range(ncols):
            start, end = cell_interval(v.size, s, e, strand, U, B, D, bin, j)
            row.append(mref.cell_figures(ref.sample(v[start:end] if start < end else v[:0], 1, lo, hi)))
        for k, name in enumerate(FIGURES):
            out[name][i] = [f[k] for f in row]
    return out


def matrix(vectors, regions, B, U=0, D=0, bin=1, what="mean", lo=-DBL_MAX, hi=DBL_MAX):
    """float64[nregions, ncols] of one figure"""
    return figures(vectors, regions, B, U, D, bin, lo, hi)[what]
