"""The localcorrelate checker (tests/localcorr_ref.py) against a literal loop over the definition in exact fractions,
against numpy.corrcoef window by window, against mutants of the definition, and on how much it leaves undecided.
CPU only."""
import math
from fractions import Fraction

import numpy as np
import pytest

import localcorr_ref as ref

# the windows and the real-valued signals of tests/test_localcorr.py, at a length of a few tiles
GPU_WINDOWS = (1, 2, 3, 100, 101, 1001, 4095, 4097)
REAL_N = 20011
MAXW = 4097


def tile_of(W):
    """the library's tile for W (host code: no GPU is touched)"""
    import genodsp_amd as gd
    return gd.localcorr_tile(W)


def literal(x, y, W, what):
    """the definition, base by base and term by term: exact sums (fractions) rounded once, then Python floats"""
    n = len(x)
    rgt = (W - 1) // 2
    lft = W - 1 - rgt
    out = []
    for c in range(n):
        lo, hi = max(0, c - lft), min(n - 1, c + rgt)
        s = [Fraction(0)] * 5
        for k in range(lo, hi + 1):
            a, b = float(x[k]), float(y[k])
            for i, t in enumerate((a, b, a * a, b * b, a * b)):             # one rounded product per term
                s[i] += Fraction(t)
        Sx, Sy, Sxx, Syy, Sxy = (float(t) for t in s)
        md = float(hi - lo + 1)
        Nxx, Nyy, Nxy = md * Sxx - Sx * Sx, md * Syy - Sy * Sy, md * Sxy - Sx * Sy
        covariance = 0.0 if Nxy == 0 else Nxy / (md * md)
        if Nxx <= 0 or Nyy <= 0:
            correlation = 0.0
        else:
            D = math.sqrt(Nxx) * math.sqrt(Nyy)
            correlation = 0.0 if D == 0 else min(max(Nxy / D, -1.0), 1.0)
        slope = 0.0 if Nxx <= 0 else Nxy / Nxx
        intercept = Sy / md - slope * (Sx / md)
        out.append({"correlation": correlation, "covariance": covariance, "slope": slope, "intercept": intercept}[what])
    return np.array(out, np.float64)


def small_pairs(n):
    """(name, x, y, exact): exact data leave every interval a point"""
    rng = np.random.default_rng(n)
    depth = lambda: rng.integers(0, 9, n).astype(np.float64) * (rng.random(n) < 0.7)
    yield "depth", depth(), depth(), True
    yield "dyadic", np.ldexp(rng.integers(-500, 500, n).astype(np.float64), -30), depth(), True
    yield "real", rng.normal(1.0, 2.0, n), rng.normal(-0.5, 1.0, n), False
    yield "real on itself", rng.normal(1.0, 2.0, n), None, False
    yield "constant track", depth(), np.full(n, 2.75), True
    yield "constant real track", rng.normal(1.0, 2.0, n), np.full(n, 0.1), False
    yield "zero", np.zeros(n), np.zeros(n), True


@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_the_checker_is_the_literal_definition(W):
    for n in range(1, 21):
        for name, x, y, exact in small_pairs(n):
            y = x.copy() if y is None else y
            plain = ref.Local(x, y, W, 0, slack=False)
            slack = ref.Local(x, y, W, 64)
            for what in ref.KINDS:
                lit = literal(x, y, W, what)
                want, low, high = plain.figure(what)
                assert ref.same_bits(want, lit).all(), (n, name, what)
                assert ref.same_bits(low, want).all() and ref.same_bits(high, want).all()
                want, low, high = slack.figure(what)
                assert ref.same_bits(want, lit).all()
                assert not ref.verdict(lit, want, low, high).any(), (n, name, what)         # the fraction's value is inside
                if exact:                                                   # grid data: a point, compared bit for bit
                    assert ref.same_bits(low, high).all(), (n, name, what)


def test_constant_tracks_give_plus_zero():
    x = ref.signal("depth", 300)
    for y in (np.full(300, 3.0), np.zeros(300)):
        for W in (1, 4, 7, 100):
            for what in ("correlation", "covariance", "slope"):
                assert ref.same_bits(ref.local_correlation(x, y, W, what)[0], np.zeros(300)).all()
            assert ref.same_bits(ref.local_correlation(y, x, W, "correlation")[0], np.zeros(300)).all()


@pytest.mark.parametrize("name", ref.REAL_SIGNALS)
def test_want_is_numpys_corrcoef(name):
    """numpy centres each window first (two passes), the definition is the one-pass form: Nxx = m Sxx - Sx Sx loses
    m Sxx / Nxx = E[x^2] / Var(x) of its relative precision, which is below 20 for these signals, over sums of 101 terms
    each rounded with u = 2^-53.  That is an error of the order of 20 x 101 x 1.1e-16 = 2e-13 in each of Nxx, Nyy, Nxy and
    a few times that in r: 1e-9 is three orders above it, and nine below the 1 a wrong window would cost."""
    n, W = 3001, 101
    x, y = ref.signal(name, n), ref.track(name, n) + 0.5 * ref.signal(name, n)
    lo, hi, m = ref.window(n, W)
    want = {what: ref.local_correlation(x, y, W, what)[0] for what in ref.KINDS}
    for c in range(n):
        a, b = x[lo[c]:hi[c] + 1], y[lo[c]:hi[c] + 1]
        cov = np.cov(a, b, bias=True)
        assert abs(want["correlation"][c] - np.corrcoef(a, b)[0, 1]) <= 1e-9, c
        assert abs(want["covariance"][c] - cov[0, 1]) <= 1e-9 * max(1.0, abs(cov[0, 1])), c
        slope = cov[0, 1] / cov[0, 0]
        assert abs(want["slope"][c] - slope) <= 1e-9 * max(1.0, abs(slope)), c
        icpt = b.mean() - slope * a.mean()
        assert abs(want["intercept"][c] - icpt) <= 1e-9 * max(1.0, abs(icpt)), c
    assert np.abs(want["correlation"]).max() > 0.3                          # (the pair is correlated somewhere)


# ---------------------------------------------------------------------------------------------------- mutants ----

def naive(x, y, lo, hi, m, what):
    """the figures from window sums in plain float arithmetic over the ends given"""
    P = [np.concatenate(([0.0], np.cumsum(d))) for d in (x, y, x * x, y * y, x * y)]
    S = [p[hi + 1] - p[lo] for p in P]
    return ref.figures(S[0], S[1], S[2], S[3], S[4], m, what)


def mutant(which, x, y, W, what):
    """None where the mutation changes nothing at this W"""
    n = x.size
    lo, hi, m = ref.window(n, W)
    if which == "shifted":
        lo, hi = np.minimum(lo + 1, n - 1), np.minimum(hi + 1, n - 1)
        m = hi - lo + 1
    elif which == "reach right":
        if W % 2:
            return None
        c = np.arange(n)
        lo, hi = np.maximum(c - (W - 1) // 2, 0), np.minimum(c + W - 1 - (W - 1) // 2, n - 1)
        m = hi - lo + 1
    elif which == "m = W":
        m = np.full(n, W, np.int64)
    elif which == "sample covariance":                                      # over m (m - 1), not m m
        return naive(x, y, lo, hi, m, what) * (m / np.maximum(m - 1, 1))
    elif which == "the signal on the track":
        x, y = y, x
    elif which == "track shifted":
        y = np.concatenate((y[1:], y[:1]))
    else:
        assert which == "dropped edge"
        lo = lo + 1
        m = m - 1
    return naive(x, y, lo, hi, m, what)


MUTANTS = (("shifted", "correlation"), ("shifted", "intercept"), ("reach right", "covariance"), ("m = W", "covariance"),
           ("m = W", "intercept"), ("sample covariance", "covariance"), ("the signal on the track", "slope"),
           ("the signal on the track", "intercept"), ("track shifted", "correlation"), ("dropped edge", "slope"))


@pytest.fixture(scope="module")
def real_locals():
    return {(name, W): ref.Local(ref.signal(name, REAL_N), ref.track(name, REAL_N), W, tile_of(W))
            for name in ref.REAL_SIGNALS for W in GPU_WINDOWS}


@pytest.mark.parametrize("name", ref.REAL_SIGNALS)
def test_mutants_are_rejected(real_locals, name):
    x, y = ref.signal(name, REAL_N), ref.track(name, REAL_N)
    for W in GPU_WINDOWS:
        if W < 3:
            continue                                        # (one base, or two: most figures are unbounded or trivial)
        for which, what in MUTANTS:
            got = mutant(which, x, y, W, what)
            if got is None:
                continue
            want, low, high = real_locals[name, W].figure(what)
            assert ref.verdict(got, want, low, high).any(), (W, which, what)
            assert not ref.verdict(want, want, low, high).any()


@pytest.mark.parametrize("name", ref.REAL_SIGNALS)
def test_little_is_left_unbounded_on_real_signals(real_locals, name):
    """the cap that keeps the GPU test honest: at most 0.1 % of the bases of a case, at every tested W >= 3 with the
    library's tile.  At W = 2 base 0 and a few in 20000 more are open, at W = 1 every base is (correlation, covariance
    and slope are 0/0 on rounded sums there): those two windows carry no cap."""
    for W in GPU_WINDOWS:
        for what in ref.KINDS:
            want, low, high = real_locals[name, W].figure(what)
            share = np.count_nonzero(ref.unbounded(low, high)) / REAL_N
            if W >= 3:
                assert share <= 0.001, (W, what, share)
            elif W == 1:
                assert share == 1.0, (W, what, share)
            assert not ref.verdict(want, want, low, high).any()


@pytest.mark.parametrize("name", ref.GRID_SIGNALS)
def test_nothing_is_left_unbounded_on_grid_signals(name):
    x, y = ref.signal(name, REAL_N), ref.track(name, REAL_N)
    assert np.count_nonzero(x == 0) > REAL_N // 10 and np.count_nonzero(y) > REAL_N // 3 and not np.array_equal(x, y)
    for W in GPU_WINDOWS:
        loc = ref.Local(x, y, W, tile_of(W))
        assert loc.exact.all()
        for what in ref.KINDS:
            want, low, high = loc.figure(what)
            assert ref.same_bits(low, want).all() and ref.same_bits(high, want).all(), (W, what)
