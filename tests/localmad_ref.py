"""CPU checker for localmad / hampel (numpy only): the definition of gdsp_localmad, computed operation by operation.

Window, centring and rank are slidingpercentile's (sliding_percentile_ref: key_of, value_of, rank, reach).  Bases whose
window lies inside the vector are done a chunk at a time with a sliding_window_view: np.partition of the keys for med,
abs(view - med[:, None]) -- one rounded subtraction per deviation, then the sign cleared -- and np.partition again for
mad; the truncated windows at the two ends one by one.  Then the figures, each step one numpy operation on float64.

The definition holds where every value of a window is finite; what this file gives elsewhere is of no account.
block(win) is the other road to the MAD, the one the kernel takes: the contiguous block of the sorted window that holds
the k+1 smallest deviations, and where it starts."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from sliding_percentile_ref import key_of, value_of, rank, reach

WHAT = ("zscore", "median", "mad", "difference", "clean", "outlier")
SCALE = 1.4826
THRESHOLD = 3.0


def _med_mad_of(win):
    """(med, mad) of one window"""
    k = rank(win.size, 50000)
    med = value_of(np.partition(key_of(win), k)[k:k + 1])[0]
    with np.errstate(over="ignore", invalid="ignore"):
        dev = np.abs(win - med)
    return med, np.partition(dev, k)[k]


def med_mad(v, W):
    """(med, mad) for every base of v: two float64 vectors"""
    v = np.ascontiguousarray(v, np.float64)
    n = v.size
    left, right = reach(W)
    med = np.empty(n, np.float64)
    mad = np.empty(n, np.float64)
    first, last = left, n - 1 - right                  # bases whose window is whole
    if last >= first:
        k = rank(W, 50000)
        kview = sliding_window_view(key_of(v), W)      # view[j] = the window of base j + left
        vview = sliding_window_view(v, W)
        chunk = max(1, (1 << 21) // W)
        for a in range(0, kview.shape[0], chunk):
            m = value_of(np.partition(kview[a:a + chunk], k, axis=1)[:, k])
            with np.errstate(over="ignore", invalid="ignore"):
                dev = np.abs(vview[a:a + chunk] - m[:, None])
            med[a + left:a + left + m.size] = m
            mad[a + left:a + left + m.size] = np.partition(dev, k, axis=1)[:, k]
    for i in range(n):
        if first <= i <= last:
            continue
        med[i], mad[i] = _med_mad_of(v[max(0, i - left):min(n - 1, i + right) + 1])
    return med, mad


def figures(v, W, scale=SCALE, threshold=THRESHOLD, minmad=None, parts=None):
    """{figure: vector} for every figure of WHAT.  parts: (med, mad) from med_mad(v, W), when the caller has them"""
    v = np.ascontiguousarray(v, np.float64)
    med, mad = parts if parts is not None else med_mad(v, W)
    scale, threshold = np.float64(scale), np.float64(threshold)
    madf = mad if minmad is None else np.where(np.float64(minmad) > mad, np.float64(minmad), mad)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        sigma = scale * madf
        diff = np.where(v == med, 0.0, v - med)
        limit = threshold * sigma
        outlier = np.abs(diff) > limit
        safe = np.where(sigma == 0, 1.0, sigma)
        z = np.where(sigma == 0, 0.0, diff / safe)
    return {"zscore": z, "median": med, "mad": np.ascontiguousarray(madf, np.float64), "difference": diff,
            "clean": np.where(outlier, med, v), "outlier": outlier.astype(np.float64)}


def local_mad(v, W, as_="zscore", scale=SCALE, threshold=THRESHOLD, minmad=None):
    return figures(v, W, scale, threshold, minmad)[as_]


def hampel(v, W, as_="clean", scale=SCALE, threshold=THRESHOLD, minmad=None):
    return figures(v, W, scale, threshold, minmad)[as_]


def block(win):
    """(a, mad) of one window by the block rule: with s the sorted window and med = s[k], the k+1 smallest deviations are
    those of s[a .. a+k] for the a of 0 .. min(k, m-1-k) whose larger end deviation is smallest (the first such a)"""
    win = np.ascontiguousarray(win, np.float64)
    m = win.size
    k = rank(m, 50000)
    s = value_of(np.sort(key_of(win)))
    med = s[k]
    with np.errstate(over="ignore", invalid="ignore"):
        ends = [max(abs(med - s[a]), abs(s[a + k] - med)) for a in range(min(k, m - 1 - k) + 1)]
    a = int(np.argmin(ends))
    return a, ends[a]


def window_of(v, W, i):
    left, right = reach(W)
    return np.ascontiguousarray(v, np.float64)[max(0, i - left):min(len(v) - 1, i + right) + 1]
