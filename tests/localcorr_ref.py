"""Checker for localcorrelate (gdsp_localcorr in include/genodsp_hip.h, genodsp_amd/csrc/gdsp_localcorr.hip; not in the
reference).  CPU only: numpy and Python ints, on top of runsum_ref and in the construction of localstats_ref.

The definition.  Base c of two vectors x (the signal) and y (the track) of n values has slidingsum's window [lo, hi] =
[max(0, c-lft), min(n-1, c+rgt)], rgt = (W-1)//2, lft = W-1-rgt, with m = hi-lo+1 bases.  Over it Sx and Sy are the sums
of x[k] and y[k], and Sxx, Syy, Sxy the sums of fl(x[k] x[k]), fl(y[k] y[k]) and fl(x[k] y[k]); with md = float(m)

    Nxx = fl(fl(md Sxx) - fl(Sx Sx))    Nyy = fl(fl(md Syy) - fl(Sy Sy))    Nxy = fl(fl(md Sxy) - fl(Sx Sy))
    covariance  = +0.0 if Nxy == 0 else fl(Nxy / fl(md md))
    correlation = +0.0 if Nxx <= 0 or Nyy <= 0, else with D = fl(sqrt(Nxx) sqrt(Nyy)):
                  +0.0 if D == 0 else fl(Nxy / D) clamped into [-1, 1]
    slope       = +0.0 if Nxx <= 0 else fl(Nxy / Nxx)
    intercept   = fl(fl(Sy / md) - fl(slope fl(Sx / md)))

What a correct implementation may return.  The five sums may be formed in any order, as differences of partial sums
that reach no further than `tile` bases beyond the window on either side.  runsum_ref's tiled rule bounds each of them:

    |S~ - S| <= E = gamma_M A(Z),   M = 2 (W + tile) + 4,   Z = the window widened by `tile` on either side,

and E = 0 where no sum of Z's terms can round (runsum_ref.Prefix: A(Z) <= 2^53 q).  The sums are formed exactly, from
runsum_ref.Prefix over x, y, and x*x, y*y, x*y computed in numpy (which are the rounded products).

  want         the definition evaluated operation by operation in float64 from the once-rounded sums.
  [low, high]  the definition pushed through interval arithmetic from the five [S - E, S + E], the ends converted to
               doubles outwards.  Every later step is one correctly rounded operation, and rounding to nearest is
               monotone: the result of fl(a op b) over a box lies between the smallest and the largest of
               fl(corner op corner), so the ends are those, with nothing added.  (Sx Sx over an interval that contains 0
               starts at 0.)  Every use of a sum is treated as independent: wider, never wrong.
  unbounded    low = -inf, high = +inf where the intervals do not decide a branch of the definition: Nxx <= 0 or
               Nyy <= 0 (correlation), Nxx <= 0 (slope, intercept), D == 0 (correlation), Nxy == 0 (covariance).
Where all five E are 0 every interval is a point and low = want = high.

A window of one base (all of W = 1, base 0 of W = 2) has Nxx = Nyy = Nxy = 0 by definition, and an implementation that
forms the sums as differences of rounded partial sums gets rounding noise there: on real-valued data every figure of
such a base but the intercept's mean is 0/0 in earnest, and the checker leaves it unbounded, as it must."""
import numpy as np

import runsum_ref
from localstats_ref import (GRID_SIGNALS, REAL_SIGNALS, _corners, _doubles, same_bits, signal, unbounded, verdict,     # noqa: F401
                            window)

KINDS = ("correlation", "covariance", "slope", "intercept")
TRACK_SEED = 7


def track(name, n):
    """the second track the tests share: the signal's kind, drawn again"""
    return signal(name, n, seed=TRACK_SEED)


def figures(Sx, Sy, Sxx, Syy, Sxy, m, what):
    """the definition from the sums on, every step one rounded float64 operation"""
    assert what in KINDS
    md = m.astype(np.float64)
    with np.errstate(all="ignore"):
        Nxy = md * Sxy - Sx * Sy
        if what == "covariance":
            return np.where(Nxy == 0.0, 0.0, Nxy / (md * md))
        Nxx = md * Sxx - Sx * Sx
        if what == "correlation":
            Nyy = md * Syy - Sy * Sy
            flat = (Nxx <= 0.0) | (Nyy <= 0.0)
            D = np.sqrt(np.where(flat, 1.0, Nxx)) * np.sqrt(np.where(flat, 1.0, Nyy))
            r = np.minimum(np.maximum(Nxy / D, -1.0), 1.0)
            return np.where(flat | (D == 0.0), 0.0, r)
        slope = np.where(Nxx <= 0.0, 0.0, Nxy / Nxx)
        if what == "slope":
            return slope
        return Sy / md - slope * (Sx / md)


class Local:
    """everything about one (x, y, W, tile) that does not depend on the figure asked for.  slack=False: E = 0 (the
    literal definition, for the checker's own tests)"""

    def __init__(self, x, y, W, tile, slack=True):
        assert W >= 1 and tile >= 0
        self.x = x = np.ascontiguousarray(x, np.float64)
        self.y = y = np.ascontiguousarray(y, np.float64)
        assert x.size == y.size and np.isfinite(x).all() and np.isfinite(y).all()
        self.n, self.W = int(x.size), W
        n = self.n
        self.lo, self.hi, self.m = window(n, W)
        rgt = (W - 1) // 2
        c = np.arange(n, dtype=np.int64)
        a, b = np.maximum(c - (W - 1 - rgt) - tile, 0), np.minimum(c + rgt + tile, n - 1)
        self.sums = []                                                       # per sum: (nearest, low, high)
        for d in (x, y, x * x, y * y, x * y):
            p = runsum_ref.Prefix(d, slack=slack)
            P, A, _ = p.padded()
            S = P[self.hi + 1] - P[self.lo]
            E = p.gamma_times(2 * (W + tile) + 4, A[b + 1] - A[a]) if slack else S * 0
            near, _, _ = _doubles(p, S)
            _, low, _ = _doubles(p, S - E)
            _, _, high = _doubles(p, S + E)
            point = np.array(E == 0, bool)                                  # (then S is a double, or slack is off)
            self.sums.append((near, np.where(point, near, low), np.where(point, near, high)))
        self.exact = np.logical_and.reduce([s[1] == s[2] for s in self.sums])       # every E is 0

    def figure(self, what):
        """(want, low, high) per base"""
        assert what in KINDS
        md = self.m.astype(np.float64)
        (Sx, Sxl, Sxh), (Sy, Syl, Syh), (Sxx, Sxxl, Sxxh), (Syy, Syyl, Syyh), (Sxy, Sxyl, Sxyh) = self.sums
        want = figures(Sx, Sy, Sxx, Syy, Sxy, self.m, what)
        with np.errstate(all="ignore"):
            pl, ph = _corners(np.multiply, Sxl, Sxh, Syl, Syh)
            Nxyl, Nxyh = md * Sxyl - ph, md * Sxyh - pl
            if what == "covariance":
                mm = md * md
                zero = (Nxyl == 0.0) & (Nxyh == 0.0)
                open_ = (Nxyl <= 0.0) & (Nxyh >= 0.0) & ~zero
                low, high = np.where(zero, 0.0, Nxyl / mm), np.where(zero, 0.0, Nxyh / mm)
            else:
                sql, sqh = _corners(np.multiply, Sxl, Sxh, Sxl, Sxh)
                sql = np.where((Sxl <= 0.0) & (Sxh >= 0.0), 0.0, sql)
                Nxxl, Nxxh = md * Sxxl - sqh, md * Sxxh - sql
                zero = Nxxh <= 0.0
                open_ = (Nxxl <= 0.0) & ~zero
                if what == "correlation":
                    sql, sqh = _corners(np.multiply, Syl, Syh, Syl, Syh)
                    sql = np.where((Syl <= 0.0) & (Syh >= 0.0), 0.0, sql)
                    Nyyl, Nyyh = md * Syyl - sqh, md * Syyh - sql
                    open_ = open_ | ((Nyyl <= 0.0) & ~(Nyyh <= 0.0))
                    zero = zero | (Nyyh <= 0.0)
                    open_ = open_ & ~zero                                   # (one side decided flat decides the base)
                    safe = ~(zero | open_)
                    Dl = np.sqrt(np.where(safe, Nxxl, 1.0)) * np.sqrt(np.where(safe, Nyyl, 1.0))
                    Dh = np.sqrt(np.where(safe, Nxxh, 1.0)) * np.sqrt(np.where(safe, Nyyh, 1.0))
                    zero = zero | (safe & (Dh == 0.0))
                    open_ = open_ | (safe & (Dl == 0.0) & (Dh != 0.0))
                    safe = ~(zero | open_)
                    low, high = _corners(np.divide, Nxyl, Nxyh, np.where(safe, Dl, 1.0), np.where(safe, Dh, 1.0))
                    low, high = np.minimum(np.maximum(low, -1.0), 1.0), np.minimum(np.maximum(high, -1.0), 1.0)
                    low, high = np.where(zero, 0.0, low), np.where(zero, 0.0, high)
                else:
                    safe = ~(zero | open_)
                    low, high = _corners(np.divide, Nxyl, Nxyh, np.where(safe, Nxxl, 1.0), np.where(safe, Nxxh, 1.0))
                    low, high = np.where(zero, 0.0, low), np.where(zero, 0.0, high)
                    if what == "intercept":
                        ql, qh = _corners(np.multiply, low, high, Sxl / md, Sxh / md)
                        low, high = Syl / md - qh, Syh / md - ql
        low, high = np.where(open_, -np.inf, low), np.where(open_, np.inf, high)
        return want, low, high


def local_correlation(x, y, W, what="correlation", tile=0, slack=True):
    """(want, low, high) per base"""
    return Local(x, y, W, tile, slack).figure(what)
