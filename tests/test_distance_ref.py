"""tests/distance_ref.py against itself: the vectorised checker held to the literal loop of the definition
(gdsp_distance, include/genodsp_hip.h) on short vectors, and the identities that tie distance to dilate and erode, which
tests/test_distance.py leans on.  No GPU."""
import itertools

import numpy as np
import pytest

import distance_ref as ref
from oracle import cpu

OPTIONS = list(itertools.product(ref.SIDES, (False, True), (None, 1, 7)))
IDS = ["%s-%s-%s" % (to, "signed" if s else "unsigned", cap) for to, s, cap in OPTIONS]


def contents(n, rng):
    """what a vector of n bases can hold that matters: nothing, everything, NaNs, one member at either end, and noise"""
    none = np.zeros(n)
    every = np.ones(n)
    nans = np.where(rng.random(n) < 0.3, np.nan, rng.integers(0, 2, n).astype(np.float64))
    first = np.zeros(n)
    first[0] = 1
    last = np.zeros(n)
    last[n - 1] = 1
    infs = rng.choice([-np.inf, 0.0, np.inf, np.nan, 1.0], n)
    return [none, every, nans, first, last, infs, (rng.random(n) < 0.5) * 1.0, (rng.random(n) < 0.1) * 1.0,
            (rng.random(n) < 0.9) * 1.0]


@pytest.mark.parametrize("to,signed,cap", OPTIONS, ids=IDS)
def test_the_vectorised_checker_is_the_loop(to, signed, cap):
    rng = np.random.default_rng(20260101)
    for n in range(1, 41):
        for v in contents(n, rng):
            got = ref.distance(v, to=to, signed=signed, cap=cap)
            want = ref.distance_loop(v, to=to, signed=signed, cap=cap)
            assert got.tobytes() == want.tobytes(), (n, v.tolist(), got.tolist(), want.tolist())


def test_the_threshold_and_its_ties():
    v = np.array([0.0, 2.0, 3.0, np.nan, 2.0, 1.0, np.inf, -np.inf])
    assert ref.members(v, 2.0).tolist() == [False, False, True, False, False, False, True, False]
    assert ref.members(v, 2.0, True).tolist() == [False, True, True, False, True, False, True, False]
    for ties in (False, True):
        for to, signed, cap in OPTIONS:
            got = ref.distance(v, 2.0, ties, to, signed, cap)
            assert got.tobytes() == ref.distance_loop(v, 2.0, ties, to, signed, cap).tobytes()
    assert ref.distance(v, 2.0).tolist() == [2, 1, 0, 1, 2, 1, 0, 1]
    assert ref.distance(v, 2.0, signed=True).tolist() == [2, 1, -1, 1, 2, 1, -1, 1]
    assert ref.distance(v, 2.0, True, "left").tolist() == [8, 0, 0, 1, 0, 1, 0, 1]             # nothing to the left of base 0: n
    assert ref.distance(v, 2.0, True, "right", cap=1).tolist() == [1, 0, 0, 1, 0, 1, 0, 1]     # ... nothing to the right of 7: the cap


def test_what_the_definition_promises():
    rng = np.random.default_rng(7)
    for n in (1, 2, 17, 40):
        for v in contents(n, rng):
            m = ref.members(v)
            for to in ref.SIDES:
                d = ref.distance(v, to=to)
                assert ((d == 0) == m).all() and not np.signbit(d).any()                      # unsigned: 0 iff member, and +0.0
                s = ref.distance(v, to=to, signed=True)
                assert (s != 0).all() and ((s < 0) == m).all()                                # signed: nothing is 0
                assert (s[~m] == d[~m]).all()
                assert (d[d != n] <= n - 1).all()                                             # n is reached by no distance
            s = ref.distance(v, signed=True)
            edge = m & ~(np.concatenate(([False], m[:-1])) & np.concatenate((m[1:], [False])))
            assert (s[edge] == -1).all()                                                      # the edge bases of a run
            beside = ~m & (np.concatenate(([False], m[:-1])) | np.concatenate((m[1:], [False])))
            assert (s[beside] == 1).all()                                                     # the base next to a run


@pytest.mark.parametrize("r", [0, 1, 2, 5, 39, 100])
def test_distance_against_dilate_and_erode(r):
    """nearest <= r iff dilate with left = right = r says one (for r < n: a vector without a member holds n, which a
    radius of n or more would take for a distance); signed <= -(r+1) iff erode does"""
    rng = np.random.default_rng(11 + r)
    for n in list(range(1, 41)) + [200]:
        for v in contents(n, rng):
            v = np.where(np.isnan(v), 0.0, v)                                                 # (dilate's own test takes a NaN as a member)
            d = ref.distance(v)
            s = ref.distance(v, signed=True)
            for dil, ero in ((ref.dilate(v, r), ref.erode(v, r)), (cpu.dilate(v, r, r), cpu.erode(v, r, r))):
                near = (d <= r) if r < n else (d < n)                                         # (r >= n: "no member" is n, not a distance)
                assert (near == (dil == 1)).all(), (n, r, v.tolist())
                assert ((s <= -(r + 1)) == (ero == 1)).all(), (n, r, v.tolist())
            for cap in (1, 7):
                if r < cap:                                          # one capped pass answers every r below the cap, whatever n
                    assert ((ref.distance(v, cap=cap) <= r) == (ref.dilate(v, r) == 1)).all()
                    assert ((ref.distance(v, signed=True, cap=cap) <= -(r + 1)) == (ref.erode(v, r) == 1)).all()
