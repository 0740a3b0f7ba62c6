"""numpy checker for prominence (gdsp_prominence, include/genodsp_hip.h): -> (prominence, base) of every base.

The walks are found by binary lifting over sparse tables: table k holds the max and the min of every stretch of 2^k
values; from base i a walk takes the stretches 2^K, ..., 2, 1 in turn, each when it lies inside the window and the vector
and holds nothing above v[i], and folds the stretch's min into the walk's minimum.  "Nothing above x" is closed under
taking prefixes, so this reaches exactly where the one-by-one walk stops.  tests/test_prominence_ref.py holds it to a
literal loop of the definition and to scipy.signal.peak_prominences.  A window that holds a NaN gives an unspecified
result, here as in the library."""
import numpy as np


def reach(W):
    left = (W - 1) // 2
    return left, W - 1 - left


def literal(v, W):
    """the definition, word for word"""
    v = np.asarray(v, np.float64)
    n = v.size
    wL, wR = reach(W)
    prom, base = np.zeros(n), np.zeros(n)
    for i in range(n):
        x = v[i]
        mL = x
        j = i - 1
        while j >= max(0, i - wL) and not v[j] > x:
            if v[j] < mL:
                mL = v[j]
            j -= 1
        mR = x
        j = i + 1
        while j <= min(n - 1, i + wR) and not v[j] > x:
            if v[j] < mR:
                mR = v[j]
            j += 1
        b = mL if mL >= mR else mR
        base[i] = b
        prom[i] = 0.0 if x == b else x - b
    return prom, base


def prominence(v, W):
    v = np.ascontiguousarray(v, np.float64)
    n = v.size
    wL, wR = reach(W)
    if n == 0:
        return np.zeros(0), np.zeros(0)
    levels = max(1, int(max(wL, wR)).bit_length())
    tmax, tmin = [v], [v]
    with np.errstate(invalid="ignore"):
        for k in range(1, levels):
            h = 1 << (k - 1)
            a, b = tmax[-1], tmin[-1]
            if a.size <= h:
                break
            tmax.append(np.maximum(a[:-h], a[h:]))
            tmin.append(np.minimum(b[:-h], b[h:]))
        i = np.arange(n)
        lo = np.maximum(0, i - wL)
        hi = np.minimum(n - 1, i + wR)
        mL, mR = v.copy(), v.copy()
        posL, posR = i.copy(), i.copy()                   # the walks have covered [posL, i) and (i, posR]
        for k in range(len(tmax) - 1, -1, -1):
            s = 1 << k
            size = tmax[k].size
            start = np.clip(posL - s, 0, size - 1)
            ok = (posL - s >= lo) & ~(tmax[k][start] > v)
            mL = np.where(ok & (tmin[k][start] < mL), tmin[k][start], mL)
            posL = np.where(ok, posL - s, posL)
            start = np.clip(posR + 1, 0, size - 1)
            ok = (posR + s <= hi) & ~(tmax[k][start] > v)
            mR = np.where(ok & (tmin[k][start] < mR), tmin[k][start], mR)
            posR = np.where(ok, posR + s, posR)
        base = np.where(mL >= mR, mL, mR)
        prom = np.where(v == base, 0.0, v - base)
    return prom, base


def clean(v, W):
    """which bases have no NaN in their window (the others' results are unspecified)"""
    v = np.asarray(v, np.float64)
    wL, wR = reach(W)
    bad = np.flatnonzero(np.isnan(v))
    ok = np.ones(v.size, bool)
    for b in bad:
        ok[max(0, b - wR):b + wL + 1] = False            # base i sees b when i-wL <= b <= i+wR
    return ok
