"""Checker for localstats (gdsp_localstats in include/genodsp_hip.h, genodsp_amd/csrc/gdsp_localstats.hip; not in the
reference).  CPU only: numpy and Python ints, on top of runsum_ref.

The definition.  Base c of a vector of n values has slidingsum's window [lo, hi] = [max(0, c-lft), min(n-1, c+rgt)],
rgt = (W-1)//2, lft = W-1-rgt, with m = hi-lo+1 bases.  S1 is the sum of v[k] and S2 the sum of fl(v[k] v[k]) over it, and

    mean = fl(S1/m)    N = fl(fl(m S2) - fl(S1 S1))    variance = +0.0 if N <= 0 else fl(N / fl(m m))
    stddev = sqrt(variance)    bg = max(mean, floor)    sd = max(stddev, minsd)

    mean: bg   variance: variance   stddev: sd   difference: fl(v - bg)   ratio: fl(v / bg), +0.0 where bg == 0
    zscore: fl(fl(v - mean) / sd), +0.0 where sd == 0

What a correct implementation may return.  The two sums may be formed in any order, as differences of partial sums
that reach no further than `tile` bases beyond the window on either side.  runsum_ref's tiled rule then bounds them:

    |S~ - S| <= E = gamma_M A(Z),   M = 2 (W + tile) + 4,   Z = the window widened by `tile` on either side,

and E = 0 where no sum of Z's terms can round (runsum_ref.Prefix: A(Z) <= 2^53 q).  S1 and S2 are formed exactly, from
runsum_ref.Prefix over v and over v*v computed in numpy (which is fl(v v)).

  want         the definition evaluated operation by operation in float64 from the once-rounded S1 and S2.
  [low, high]  the definition pushed through interval arithmetic from [S1 - E1, S1 + E1] and [S2 - E2, S2 + E2], the
               ends converted to doubles outwards.  Every later step is one correctly rounded operation, and rounding to
               nearest is monotone: the result of fl(x op y) over a box lies between the smallest and the largest of
               fl(corner op corner), so the ends are those, with nothing added.  (x x over an interval that contains 0
               starts at 0.)  Each use of S1 is treated as independent: wider, never wrong.  A divisor interval that
               contains 0 without being the point 0 makes the base unbounded: low = -inf, high = +inf.
Where E1 = E2 = 0 every interval is a point and low = want = high.

A window of one base (all of W = 1, base 0 of W = 2) has variance 0 by definition, and an implementation that forms
S1 and S2 as differences of rounded partial sums gets a variance of rounding noise there: on real-valued data the
z-score of such a base is 0/0 in earnest and the checker leaves it unbounded, as it must."""
import numpy as np

import runsum_ref

KINDS = ("zscore", "mean", "variance", "stddev", "difference", "ratio")


def window(n, W):
    """(lo, hi, m) per base"""
    rgt = (W - 1) // 2
    lft = W - 1 - rgt
    c = np.arange(n, dtype=np.int64)
    lo, hi = np.maximum(c - lft, 0), np.minimum(c + rgt, n - 1)
    return lo, hi, hi - lo + 1


def _max(x, level):
    return x if level is None else np.where(np.float64(level) > x, np.float64(level), x)


def figures(v, S1, S2, m, what, floor=None, minsd=None):
    """the definition from the sums on, every step one rounded float64 operation"""
    assert what in KINDS
    md = m.astype(np.float64)
    with np.errstate(all="ignore"):
        mean = S1 / md
        if what in ("mean", "difference", "ratio"):
            bg = _max(mean, floor)
            if what == "mean":
                return bg
            if what == "difference":
                return v - bg
            return np.where(bg == 0.0, 0.0, v / bg)
        N = md * S2 - S1 * S1
        variance = np.where(N <= 0.0, 0.0, N / (md * md))
        if what == "variance":
            return variance
        sd = _max(np.sqrt(variance), minsd)
        if what == "stddev":
            return sd
        return np.where(sd == 0.0, 0.0, (v - mean) / sd)


def _doubles(prefix, ints):
    """integers in the prefix's unit as doubles: (rounded to nearest, not above, not below)"""
    if ints.dtype == np.int64:                                              # (below 2^62: the way back is exact)
        near = ints.astype(np.float64)
        side = np.sign(near.astype(np.int64) - ints)
        return tuple(np.ldexp(x, prefix.E) for x in (near, np.where(side > 0, np.nextafter(near, -np.inf), near),
                                                     np.where(side < 0, np.nextafter(near, np.inf), near)))
    lst = [int(x) for x in ints.tolist()]
    near = np.array([float(x) for x in lst], np.float64)                    # int -> float: correctly rounded
    side = np.array([(b > x) - (b < x) for b, x in zip((int(f) for f in near.tolist()), lst)], np.int64)
    down = np.where(side > 0, np.nextafter(near, -np.inf), near)
    up = np.where(side < 0, np.nextafter(near, np.inf), near)
    return tuple(np.ldexp(x, prefix.E) for x in (near, down, up))


def _corners(op, al, ah, bl, bh):
    c = (op(al, bl), op(al, bh), op(ah, bl), op(ah, bh))
    return np.minimum.reduce(c), np.maximum.reduce(c)


class Local:
    """everything about one (v, W, tile) that does not depend on the figure asked for.  slack=False: E = 0 (the
    literal definition, for the checker's own tests)"""

    def __init__(self, v, W, tile, slack=True):
        assert W >= 1 and tile >= 0
        self.v = v = np.ascontiguousarray(v, np.float64)
        assert np.isfinite(v).all()
        self.n, self.W = int(v.size), W
        n = self.n
        self.lo, self.hi, self.m = window(n, W)
        rgt = (W - 1) // 2
        c = np.arange(n, dtype=np.int64)
        a, b = np.maximum(c - (W - 1 - rgt) - tile, 0), np.minimum(c + rgt + tile, n - 1)
        self.sums = []                                                       # per sum: (nearest, low, high)
        for d in (v, v * v):
            p = runsum_ref.Prefix(d, slack=slack)
            P, A, _ = p.padded()
            S = P[self.hi + 1] - P[self.lo]
            E = p.gamma_times(2 * (W + tile) + 4, A[b + 1] - A[a]) if slack else S * 0
            near, _, _ = _doubles(p, S)
            _, low, _ = _doubles(p, S - E)
            _, _, high = _doubles(p, S + E)
            point = np.array(E == 0, bool)                                  # (then S is a double, or slack is off)
            self.sums.append((near, np.where(point, near, low), np.where(point, near, high)))
        self.exact = (self.sums[0][1] == self.sums[0][2]) & (self.sums[1][1] == self.sums[1][2])    # E1 = E2 = 0

    def figure(self, what, floor=None, minsd=None):
        """(want, low, high) per base"""
        assert what in KINDS
        v, md = self.v, self.m.astype(np.float64)
        (S1, S1l, S1h), (S2, S2l, S2h) = self.sums
        want = figures(v, S1, S2, self.m, what, floor, minsd)
        unbounded = np.zeros(self.n, bool)
        with np.errstate(all="ignore"):
            meanl, meanh = S1l / md, S1h / md
            if what in ("mean", "difference", "ratio"):
                bgl, bgh = _max(meanl, floor), _max(meanh, floor)
                if what == "mean":
                    low, high = bgl, bgh
                elif what == "difference":
                    low, high = v - bgh, v - bgl
                else:
                    zero = (bgl == 0.0) & (bgh == 0.0)
                    unbounded = (bgl <= 0.0) & (bgh >= 0.0) & ~zero
                    low, high = _corners(np.divide, v, v, bgl, bgh)
                    low, high = np.where(zero, 0.0, low), np.where(zero, 0.0, high)
            else:
                sql, sqh = _corners(np.multiply, S1l, S1h, S1l, S1h)
                sql = np.where((S1l <= 0.0) & (S1h >= 0.0), 0.0, sql)
                Nl, Nh = md * S2l - sqh, md * S2h - sql
                mm = md * md
                varl, varh = np.where(Nl <= 0.0, 0.0, Nl / mm), np.where(Nh <= 0.0, 0.0, Nh / mm)
                if what == "variance":
                    low, high = varl, varh
                else:
                    sdl, sdh = _max(np.sqrt(varl), minsd), _max(np.sqrt(varh), minsd)
                    if what == "stddev":
                        low, high = sdl, sdh
                    else:
                        zero = sdh == 0.0
                        unbounded = (sdl <= 0.0) & ~zero
                        low, high = _corners(np.divide, v - meanh, v - meanl, sdl, sdh)
                        low, high = np.where(zero, 0.0, low), np.where(zero, 0.0, high)
        low, high = np.where(unbounded, -np.inf, low), np.where(unbounded, np.inf, high)
        return want, low, high


def local_stats(v, W, what="zscore", floor=None, minsd=None, tile=0, slack=True):
    """(want, low, high) per base"""
    return Local(v, W, tile, slack).figure(what, floor, minsd)


def unbounded(low, high):
    return ~(np.isfinite(low) & np.isfinite(high))


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float64).view(np.int64) == np.ascontiguousarray(b, np.float64).view(np.int64)


def verdict(got, want, low, high):
    """the bases a result fails at: outside [low, high] where that is bounded, or other bits than want where it is a
    point"""
    got = np.ascontiguousarray(got, np.float64)
    point = same_bits(low, high)
    bounded = ~unbounded(low, high)
    with np.errstate(invalid="ignore"):
        inside = (low <= got) & (got <= high)
    return (bounded & ~inside) | (point & ~same_bits(got, want))


# ------------------------------------------------------------------------------- the signals the tests share ----

GRID_SIGNALS = ("depth", "dyadic")              # exact: every figure is a point
REAL_SIGNALS = ("lognormal", "signed")          # real-valued, with local variation at every scale


def signal(name, n, seed=20261019):
    """depth: integer read depth from overlapping reads, with uncovered stretches; dyadic: multiples of 2^-30 (below
    2^-20, so that sums of their squares stay exact too); lognormal: positive, heavy-tailed, slowly modulated;
    signed: noise around a slow wave that crosses zero"""
    rng = np.random.default_rng([seed, (GRID_SIGNALS + REAL_SIGNALS).index(name)])
    if name in GRID_SIGNALS:
        d = np.zeros(n + 1, np.int64)
        reads = max(1, n // 12)
        a = rng.integers(0, n, reads)
        a = a[(a // 700) % 3 != 1]                                          # every third stretch of 700 stays uncovered
        b = np.minimum(a + rng.integers(1, 120, a.size), n)
        np.add.at(d, a, 1)
        np.add.at(d, b, -1)
        depth = np.cumsum(d[:n])
        if name == "depth":
            return depth.astype(np.float64)
        return np.ldexp((depth * 37 % 1024).astype(np.float64), -30)
    t = np.arange(n, dtype=np.float64)
    if name == "lognormal":
        return np.exp(rng.normal(0.0, 0.7, n)) * (2.0 + np.sin(t / 911.0))
    assert name == "signed"
    return rng.normal(0.0, 1.0, n) + 3.0 * np.sin(t / 1777.0)
