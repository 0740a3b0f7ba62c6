"""CPU checker for slidingpercentile / median (numpy only): the definition of gdsp_sliding_percentile, computed exactly.

Keys are the f64 bits as uint64 with the fold of gdsp_key_of (-0.0 onto +0.0; negative values bit-inverted, the rest
with the sign bit set), so the order is `percentile`'s and NaNs sit by their bits.  Bases whose window lies inside the
vector are done W at a time with a chunked sliding_window_view and np.partition; the truncated windows at the two
ends one by one."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

SIGN = np.uint64(0x8000000000000000)


def key_of(v):
    u = np.ascontiguousarray(v, np.float64).view(np.uint64).copy()
    u[u == SIGN] = 0
    return np.where((u & SIGN) != 0, ~u, u | SIGN)


def value_of(k):
    k = np.ascontiguousarray(k, np.uint64)
    return np.where((k & SIGN) != 0, k & ~SIGN, ~k).view(np.float64)


def rank(count, p_thousandths):
    """gdsp_percentile_rank: (u32)((u64)count * P / 100000.0), clamped to count-1"""
    k = int(float(count * p_thousandths) / 100000.0)
    return min(k, count - 1) if count else k


def reach(W):
    left = (W - 1) // 2
    return left, W - 1 - left


def sliding_percentiles(v, W, ps):
    """{P: out} for every P of ps over the whole vector v"""
    keys = key_of(v)
    n = keys.size
    left, right = reach(W)
    res = {p: np.empty(n, np.uint64) for p in ps}
    first, last = left, n - 1 - right                 # bases whose window is whole
    if last >= first:
        ks = sorted(set(rank(W, p) for p in ps))
        view = sliding_window_view(keys, W)           # view[j] = the window of base j + left
        chunk = max(1, (1 << 23) // W)
        for a in range(0, view.shape[0], chunk):
            part = np.partition(view[a:a + chunk], ks, axis=1)
            for p in ps:
                res[p][a + left:a + left + part.shape[0]] = part[:, rank(W, p)]
    for i in range(n):
        if first <= i <= last:
            continue
        win = keys[max(0, i - left):min(n - 1, i + right) + 1]
        ks = sorted(set(rank(win.size, p) for p in ps))
        part = np.partition(win, ks)
        for p in ps:
            res[p][i] = part[rank(win.size, p)]
    return {p: value_of(r) for p, r in res.items()}


def sliding_percentile(v, W, p_thousandths):
    return sliding_percentiles(v, W, [p_thousandths])[p_thousandths]


def sliding_percentile_at(x, x0, n, W, p_thousandths, positions):
    """out[i] for the bases i of `positions` of a vector of n values, of which x holds bases [x0, x0 + len(x)) -- at
    least every base the windows of `positions` reach"""
    keys = key_of(x)
    left, right = reach(W)
    out = np.empty(len(positions), np.uint64)
    for q, i in enumerate(positions):
        a, b = max(0, i - left), min(n - 1, i + right) + 1
        assert a >= x0 and b <= x0 + keys.size
        win = keys[a - x0:b - x0]
        k = rank(win.size, p_thousandths)
        out[q] = np.partition(win, k)[k]
    return value_of(out)
