"""The checker of `fillgaps` (gdsp_fillgaps in include/genodsp_hip.h): the unknown bases of a vector take their values from
the known bases before and behind their gap.  `fill_gaps` is vectorised (running maxima and minima over the known bases'
indices, then the definition's arithmetic on whole arrays, one numpy operation per rounding); `fill_gaps_loop` is the
definition read aloud, base by base, and tests/test_fillgaps_ref.py holds the one to the other.  Plain numpy, no GPU."""
import numpy as np

KNOWN = ("above", "nonzero")
HOW = ("linear", "nearest", "left", "right")
ENDS = ("extend", "keep")


def known_bases(v, T=0.0, ties_above=False, known="above"):
    """above: the test of `segments`, v > T, or v >= T with ties above; nonzero: neither zero nor NaN.  A NaN is never known"""
    assert known in KNOWN
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        if known == "nonzero":
            return (v != 0) & (v == v)
        return (v >= T) if ties_above else (v > T)


def neighbours(m):
    """per base the last True of m at or before it (-1: none) and the first at or behind it (len(m): none)"""
    n = m.size
    idx = np.arange(n, dtype=np.int64)
    L = np.maximum.accumulate(np.where(m, idx, -1))
    R = np.minimum.accumulate(np.where(m, idx, n)[::-1])[::-1]
    return L, R


def fill_gaps(v, T=0.0, ties_above=False, known="above", how="linear", ends="extend", maxgap=None):
    assert how in HOW and ends in ENDS and (maxgap is None or maxgap >= 1)
    v = np.asarray(v, np.float64)
    out = v.copy()
    n = v.size
    m = known_bases(v, T, ties_above, known)
    if not m.any():
        return out                                                              # nothing known: untouched
    idx = np.arange(n, dtype=np.int64)
    L, R = neighbours(m)
    have_l, have_r = L >= 0, R < n
    both = have_l & have_r
    a = v[np.where(have_l, L, 0)]                                               # (whatever, where the side does not exist)
    b = v[np.where(have_r, R, 0)]
    if how == "linear":
        k = (idx - L).astype(np.float64)
        d = (R - L).astype(np.float64)
        with np.errstate(all="ignore"):
            x = a + ((b - a) * k) / d                                           # four operations, each rounded once
            lo, hi = np.where(a < b, a, b), np.where(a < b, b, a)
            x = np.where(x < lo, lo, np.where(x > hi, hi, x))                   # (a NaN passes)
            val = np.where(a == b, a, x)
        wanted = both
    elif how == "nearest":
        val, wanted = np.where(idx - L <= R - idx, a, b), both
    elif how == "left":
        val, wanted = a, have_l
    else:
        val, wanted = b, have_r
    if ends == "extend":                                                        # the side that exists (one does)
        val, wanted = np.where(wanted, val, np.where(have_l, a, b)), have_l | have_r
    fill = ~m & wanted
    if maxgap is not None:
        fill &= (R - L - 1) <= maxgap                                           # the gap's length, the end gaps' too
    out[fill] = val[fill]
    return out


def fill_gaps_loop(v, T=0.0, ties_above=False, known="above", how="linear", ends="extend", maxgap=None):
    """the definition, literally"""
    v = np.asarray(v, np.float64)
    n = len(v)
    out = v.copy()

    def is_known(x):
        if known == "nonzero":
            return x != 0 and x == x
        return (x >= T) if ties_above else (x > T)                              # (False for a NaN either way)

    kn = [bool(is_known(np.float64(v[i]))) for i in range(n)]
    if not any(kn):
        return out
    i = 0
    while i < n:
        if kn[i]:
            i += 1
            continue
        j = i
        while j < n and not kn[j]:
            j += 1                                                              # the gap is [i, j)
        l = i - 1 if i > 0 else None
        r = j if j < n else None
        if maxgap is None or j - i <= maxgap:
            for p in range(i, j):
                if l is not None and r is not None:
                    a, b = v[l], v[r]
                    if how == "linear":
                        if a == b:
                            x = a
                        else:
                            with np.errstate(all="ignore"):
                                s = np.float64(b - a)
                                s = np.float64(s * np.float64(p - l))
                                s = np.float64(s / np.float64(r - l))
                                x = np.float64(a + s)
                            lo, hi = min(a, b), max(a, b)
                            x = lo if x < lo else (hi if x > hi else x)
                    elif how == "nearest":
                        x = a if p - l <= r - p else b
                    else:
                        x = a if how == "left" else b
                    out[p] = x
                else:
                    side = l if l is not None else r                            # an end gap: the one known neighbour
                    needs_other = (how == "left" and l is None) or (how == "right" and r is None) or how in ("linear", "nearest")
                    if not needs_other or ends == "extend":
                        out[p] = v[side]
        i = j
    return out
