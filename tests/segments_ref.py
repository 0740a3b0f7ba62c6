"""Numpy checker for segments (include/genodsp_hip.h; not in the reference), straight from the definition:
predicate -> runs -> join across gaps of at most merge_gap -> filters, and statsover's figures over the finite members
of each kept segment through tests/xsum_ref.py (exact integer sum, each figure rounded once)."""
import math

import numpy as np

import xsum_ref as ref


def members(v, T, ties_above=False):
    """binarize's test; a NaN is never a member"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return (v >= T) if ties_above else (v > T)


def runs(m):
    """the maximal stretches [s, e) of True"""
    m = np.asarray(m, bool)
    d = np.diff(np.concatenate(([0], m.astype(np.int8), [0])))
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1)


def joined(starts, ends, merge_gap):
    """lists of run indices, one list per segment"""
    groups = []
    for k in range(len(starts)):
        if groups and int(starts[k]) - int(ends[groups[-1][-1]]) <= merge_gap:
            groups[-1].append(k)
        else:
            groups.append([k])
    return groups


def figures(v, m, s, e):
    """(count, sum, mean, min, max, maxpos) over the finite members of v[s:e]; maxpos -1 when there are none"""
    if e - s == 1 and np.isfinite(v[s]):                  # (one finite member is every figure of itself)
        x = float(v[s] + 0.0)
        return (1, x, x, x, x, s)
    x = v[s:e]
    keep = m[s:e] & np.isfinite(x)
    smp = x[keep]
    n = int(smp.size)
    M = ref.exact_int(smp)
    total = ref.round_ratio(M, 1 << ref.SCALE)
    if n == 0:
        return (0, total, math.nan, math.nan, math.nan, -1)
    mx = smp.max()
    return (n, total, ref.round_ratio(M, n << ref.SCALE), float(smp.min() + 0.0), float(mx + 0.0),
            s + int(np.flatnonzero(keep & (x == mx))[0]))


def segments(v, T, ties_above=False, merge_gap=0, min_length=1, min_height=None):
    """-> list of (start, end, count, sum, mean, min, max, maxpos) of the kept segments of one vector, in order"""
    v = np.asarray(v, np.float64)
    m = members(v, T, ties_above)
    starts, ends = runs(m)
    out = []
    for group in joined(starts, ends, merge_gap):
        s, e = int(starts[group[0]]), int(ends[group[-1]])
        if e - s < min_length:
            continue
        f = figures(v, m, s, e)
        if min_height is not None and (f[0] == 0 or f[4] < min_height):
            continue
        out.append((s, e) + f)
    return out


def genome(vectors, T, **kw):
    """-> list of (vec, start, end, count, sum, mean, min, max, maxpos) over a list of vectors"""
    return [(k,) + seg for k, v in enumerate(vectors) for seg in segments(v, T, **kw)]


def same_table(got, want):
    """got: the dict of arrays the library's Python face returns; want: genome()'s list.  Bit for bit."""
    assert len(got["start"]) == len(want), (len(got["start"]), len(want))
    for i, w in enumerate(want):
        have = (int(got["vec"][i]), int(got["start"][i]), int(got["end"][i]), int(got["count"][i]))
        assert have == w[:4], (i, have, w)
        for k, name in ((4, "sum"), (5, "mean"), (6, "min"), (7, "max")):
            assert ref.same(got[name][i], w[k]), (i, name, w[:3], got[name][i], w[k])
        assert int(got["maxpos"][i]) == w[8], (i, w[:3], int(got["maxpos"][i]), w[8])
