"""The localstats checker (tests/localstats_ref.py) against a literal double loop over the definition, against mutants
of the definition, and on how much it leaves undecided.  CPU only."""
import math
from fractions import Fraction

import numpy as np
import pytest

import localstats_ref as ref

# the windows and the real-valued signals of tests/test_localstats.py, at a length of a few tiles of the short windows
GPU_WINDOWS = (1, 2, 3, 100, 101, 1001, 4095, 4099, 10001, 12287)
TILE_OF = lambda W: (8192 if W <= 4097 else 16384) - 2 * ((W + 1) // 2)      # at least the kernel's tile
REAL_N = 20011


def literal(v, W, what, floor=None, minsd=None):
    """the definition, base by base and term by term: exact sums (fractions) rounded once, then Python floats"""
    n = len(v)
    rgt = (W - 1) // 2
    lft = W - 1 - rgt
    out = []
    for c in range(n):
        lo, hi = max(0, c - lft), min(n - 1, c + rgt)
        m = hi - lo + 1
        s1, s2 = Fraction(0), Fraction(0)
        for k in range(lo, hi + 1):
            s1 += Fraction(float(v[k]))
            s2 += Fraction(float(v[k]) * float(v[k]))                       # one rounded product per term
        S1, S2, md, x = float(s1), float(s2), float(m), float(v[c])
        mean = S1 / md
        N = md * S2 - S1 * S1
        variance = 0.0 if N <= 0 else N / (md * md)
        stddev = math.sqrt(variance)
        bg = mean if floor is None else max(mean, floor)
        sd = stddev if minsd is None else max(stddev, minsd)
        out.append({"mean": bg, "variance": variance, "stddev": sd, "difference": x - bg,
                    "ratio": 0.0 if bg == 0 else x / bg,
                    "zscore": 0.0 if sd == 0 else (x - mean) / sd}[what])
    return np.array(out, np.float64)


def small_vectors(n):
    rng = np.random.default_rng(n)
    yield "depth", rng.integers(0, 9, n).astype(np.float64) * (rng.random(n) < 0.7)
    yield "real", rng.normal(1.0, 2.0, n)
    yield "constant", np.full(n, 2.75)
    yield "constant real", np.full(n, 0.1)
    yield "zero", np.zeros(n)


@pytest.mark.parametrize("W", [1, 2, 3, 4, 7])
def test_the_checker_is_the_literal_definition(W):
    for n in range(1, 21):
        for name, v in small_vectors(n):
            plain = ref.Local(v, W, 0, slack=False)
            slack = ref.Local(v, W, 64)
            for what in ref.KINDS:
                for floor, minsd in ((None, None), (1.5, 0.5), (-1.0, 0.0), (float(np.mean(v)), float(np.std(v)))):
                    lit = literal(v, W, what, floor, minsd)
                    want, low, high = plain.figure(what, floor, minsd)
                    assert ref.same_bits(want, lit).all(), (n, name, what, floor, minsd)
                    assert ref.same_bits(low, want).all() and ref.same_bits(high, want).all()
                    want, low, high = slack.figure(what, floor, minsd)
                    assert ref.same_bits(want, lit).all()
                    assert not ref.verdict(lit, want, low, high).any(), (n, name, what)
                    if name in ("depth", "constant", "zero"):              # exact data: a point
                        assert ref.same_bits(low, high).all(), (n, name, what)


def test_constant_and_zero_windows_give_plus_zero():
    for v in (np.full(50, 3.0), np.zeros(50)):
        for W in (1, 4, 7, 100):
            z = ref.local_stats(v, W, "zscore")[0]
            assert ref.same_bits(z, np.zeros(50)).all()
    assert ref.same_bits(ref.local_stats(np.zeros(50), 7, "ratio")[0], np.zeros(50)).all()


# ---------------------------------------------------------------------------------------------------- mutants ----

def naive_sums(v, lo, hi, square=True):
    """window sums in plain float arithmetic from the ends given (far outside any allowance where a mutant moved them)"""
    P1 = np.concatenate(([0.0], np.cumsum(v)))
    P2 = np.concatenate(([0.0], np.cumsum(v * v if square else v)))
    ok = hi >= lo
    return np.where(ok, P1[hi + 1] - P1[lo], 0.0), np.where(ok, P2[hi + 1] - P2[lo], 0.0)


def mutant(which, v, W, what, floor):
    """None where the mutation changes nothing at this W"""
    n = v.size
    lo, hi, m = ref.window(n, W)
    square = True
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
        if W == 1:
            return None
        m = np.full(n, W, np.int64)
    elif which == "m - 1":
        m = m - 1
    elif which == "no square":
        square = False
    elif which == "ratio without floor":
        floor = None
    else:
        assert which == "dropped edge"
        lo = lo + 1
    S1, S2 = naive_sums(v, lo, hi, square)
    return ref.figures(v, S1, S2, m, what, floor)


MUTANTS = (("shifted", "mean"), ("reach right", "mean"), ("m = W", "mean"), ("m - 1", "mean"), ("m - 1", "variance"), ("no square", "variance"),
           ("ratio without floor", "ratio"), ("dropped edge", "mean"), ("dropped edge", "stddev"), ("shifted", "zscore"))


@pytest.fixture(scope="module")
def real_locals():
    return {(name, W): ref.Local(ref.signal(name, REAL_N), W, TILE_OF(W))
            for name in ref.REAL_SIGNALS for W in GPU_WINDOWS}


@pytest.mark.parametrize("name", ref.REAL_SIGNALS)
def test_mutants_are_rejected(real_locals, name):
    v = ref.signal(name, REAL_N)
    floor = float(np.mean(v))                                               # about half of the window means lie below it
    for W in GPU_WINDOWS:
        for which, what in MUTANTS:
            if W == 1 and what in ("variance", "stddev", "zscore"):
                continue                                    # (one base: variance 0 whatever the mutant sums, and the z-score
                                                            #  unbounded at every base -- the checker's last paragraph)
            level = floor if which == "ratio without floor" else None      # (elsewhere a floor would hide what the mutant changed)
            got = mutant(which, v, W, what, level)
            if got is None:
                continue
            want, low, high = real_locals[name, W].figure(what, level)
            assert ref.verdict(got, want, low, high).any(), (W, which, what)
            assert not ref.verdict(want, want, low, high).any()


@pytest.mark.parametrize("name", ref.REAL_SIGNALS)
def test_little_is_left_unbounded_on_real_signals(real_locals, name):
    v = ref.signal(name, REAL_N)
    for W in GPU_WINDOWS:
        for what in ref.KINDS:
            for floor, minsd in ((None, None), (float(np.mean(v)), 0.25 * float(np.std(v)))):
                want, low, high = real_locals[name, W].figure(what, floor, minsd)
                share = np.count_nonzero(ref.unbounded(low, high)) / REAL_N
                if W == 1 and what == "zscore" and minsd is None:
                    assert share == 1.0                                     # variance 0 by definition: 0/0 on rounded sums
                else:
                    assert share <= 0.01, (W, what, share)
                assert not ref.verdict(want, want, low, high).any()


@pytest.mark.parametrize("name", ref.GRID_SIGNALS)
def test_nothing_is_left_unbounded_on_grid_signals(name):
    v = ref.signal(name, REAL_N)
    assert np.count_nonzero(v == 0) > REAL_N // 10 and np.count_nonzero(v) > REAL_N // 3
    for W in GPU_WINDOWS:
        loc = ref.Local(v, W, TILE_OF(W))
        assert loc.exact.all()
        for what in ref.KINDS:
            want, low, high = loc.figure(what, float(np.mean(v)), 0.5)
            assert ref.same_bits(low, want).all() and ref.same_bits(high, want).all(), (W, what)
