"""The checker of `distance` (gdsp_distance in include/genodsp_hip.h): every base to the nearest member of
S = {i : v[i] above T}.  `distance` is vectorised (running maxima and minima over the members' indices); `distance_loop` is
the definition read aloud, base by base, and tests/test_distance_ref.py holds the one to the other.  Plain numpy, no GPU."""
import numpy as np

SIDES = ("nearest", "left", "right")


def members(v, T=0.0, ties_above=False):
    """the test of `segments`: v > T, or v >= T with ties above; a NaN is never a member"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return (v >= T) if ties_above else (v > T)


def _to_set(inset, to, before, behind):
    """per base the distance to the nearest True of `inset` on the side(s) `to`, -1 where there is none; `before` /
    `behind`: a position in front of / behind the vector that counts as set (None: none does)"""
    n = inset.size
    idx = np.arange(n, dtype=np.int64)
    far = np.int64(1) << 40
    left = np.maximum.accumulate(np.where(inset, idx, -far))                    # the last set position <= i
    right = np.minimum.accumulate(np.where(inset, idx, far)[::-1])[::-1]        # the first one >= i
    if before is not None:
        left = np.maximum(left, before)
    if behind is not None:
        right = np.minimum(right, behind)
    dl = np.where(left > -far, idx - left, far)
    dr = np.where(right < far, right - idx, far)
    d = {"nearest": np.minimum(dl, dr), "left": dl, "right": dr}[to]
    return np.where(d >= far, -1, d)


def distance(v, T=0.0, ties_above=False, to="nearest", signed=False, cap=None):
    assert to in SIDES and (cap is None or cap >= 1)
    m = members(v, T, ties_above)
    n = m.size
    none = n if cap is None else cap
    d = _to_set(m, to, None, None)
    d = np.where(d < 0, none, d)
    if signed:
        e = _to_set(~m, to, -1, n)                                              # outside the vector is not in S
        d = np.where(m, -e, d)
    if cap is not None:
        d = np.clip(d, -cap, cap)
    return d.astype(np.float64) + 0.0                                           # (+0.0, never -0.0)


def distance_loop(v, T=0.0, ties_above=False, to="nearest", signed=False, cap=None):
    """the definition, literally"""
    n = len(v)
    member = [False] * n
    for i in range(n):
        x = float(v[i])
        member[i] = (x >= T) if ties_above else (x > T)                         # (False for a NaN either way)

    def figure(i, inset):
        """the smaller of the distances that exist towards the asked side(s); None where none does"""
        dl = dr = None
        if to != "right":
            j = i
            while j >= -1 and not inset(j):
                j -= 1
            dl = i - j if j >= -1 else None
        if to != "left":
            j = i
            while j <= n and not inset(j):
                j += 1
            dr = j - i if j <= n else None
        have = [x for x in (dl, dr) if x is not None]
        return min(have) if have else None

    out = np.empty(n, np.float64)
    for i in range(n):
        if signed and member[i]:
            e = figure(i, lambda j: j < 0 or j >= n or not member[j])
            out[i] = -e if cap is None else max(-e, -cap)
        else:
            d = figure(i, lambda j: 0 <= j < n and member[j])
            if d is None:
                d = n if cap is None else cap
            out[i] = d if cap is None else min(d, cap)
    return out


def dilate(v, r, T=0.0):
    """gdsp_morph.hip's header with left = right = r: one iff S meets [i-r, i+r]"""
    m = members(v, T)
    n = m.size
    c = np.concatenate(([0], np.cumsum(m)))
    i = np.arange(n)
    return (c[np.minimum(i + r + 1, n)] - c[np.maximum(i - r, 0)] > 0).astype(np.float64)


def erode(v, r, T=0.0):
    """one iff [i-r, i+r] lies inside S, outside the vector counting as not in S"""
    m = members(v, T)
    n = m.size
    c = np.concatenate(([0], np.cumsum(m)))
    i = np.arange(n)
    whole = (i - r >= 0) & (i + r < n)
    return (whole & (c[np.minimum(i + r + 1, n)] - c[np.maximum(i - r, 0)] == 2 * r + 1)).astype(np.float64)
