"""CPU: the exact running-sum checker (runsum_ref.py) against the literal definition, against itself (two back ends)
and against the restated reference -- the evidence that its bounds are right before a GPU is involved."""
from fractions import Fraction

import numpy as np
import pytest

import runsum_cases as rc
import runsum_ref as rr
from conftest import bits_equal
from oracle import cpu


def literal_clump(v, T, L, above):
    """the definition, O(n^2), in exact rationals: base t is marked <=> there are j < t <= i, i - j >= L, P[j] <= P[i];
    every marked run is then cut back to its first and last on-side base"""
    n = len(v)
    d = (v - T) if above else (T - v)
    P = [Fraction(0)]                                       # P[j+1] is the prefix through base j
    for x in d:
        P.append(P[-1] + Fraction(float(x)))
    marked = np.zeros(n, bool)
    for i in range(n):
        for j in range(-1, i):
            if i - j >= L and P[j + 1] <= P[i + 1]:
                marked[j + 1:i + 1] = True
    on = (v >= T) if above else (v <= T)
    out = np.zeros(n, bool)
    t = 0
    while t < n:
        if not marked[t]:
            t += 1
            continue
        e = t
        while e < n and marked[e]:
            e += 1
        hits = [k for k in range(t, e) if on[k]]
        if hits:
            out[hits[0]:hits[-1] + 1] = True
        t = e
    return out


def test_bounds_without_slack_are_the_literal_definition():
    rng = np.random.default_rng(rc.SEED)
    for it in range(200):
        n = int(rng.integers(1, 121))
        kind = it % 4
        above = bool((it >> 2) & 1)
        if kind == 0:                                       # integer depth, dyadic threshold: ties everywhere
            v, T = rng.poisson(5, n).astype(np.float64), 5.5
        elif kind == 1:                                     # reals
            v, T = rng.standard_normal(n) * 3, 0.731
        elif kind == 2:                                     # on the int64 back end's grid
            v, T = np.rint(rng.standard_normal(n) * 2.0 ** 32) * 2.0 ** -30, 0.25
        else:                                               # every base on the wrong side
            v, T = rng.random(n), (2.0 if above else -1.0)
        L = int(rng.integers(1, n + 2))
        want = literal_clump(v, T, L, above)
        strict, lenient = rr.clump_bounds(v, T, L, above, backend="int", slack=False)
        assert np.array_equal(strict, want) and np.array_equal(lenient, want), (it, n, L, above)
        assert np.array_equal(cpu.clump(v, T, L, above) == 1.0, want), (it, n, L, above)
        if kind in (0, 2):
            strict, lenient = rr.clump_bounds(v, T, L, above, backend="int64", slack=False)
            assert np.array_equal(strict, want) and np.array_equal(lenient, want), (it, n, L, above)
        if kind == 3:
            assert not want.any()


def test_back_ends_agree_on_grid_inputs():
    """P, A, eps and the earliest admitted partners, as integers in the same unit; long enough for eps to leave 0"""
    rng = np.random.default_rng(rc.SEED + 1)
    n = 300000
    v = 16.0 + rng.integers(0, 32 << 30, n).astype(np.float64) * 2.0 ** -30
    a, b = rr.Prefix(v, "int64"), rr.Prefix(v, "int", unit=-rr.GRID_BITS)
    assert a.P.tolist() == b.P and a.A.tolist() == b.A and a.eps.tolist() == b.eps
    assert a.eps[0] == 0 and a.eps[-1] > 0 and np.all(np.diff(a.eps) >= 0)
    k = int(np.argmax(a.eps > 0))                           # eps[k] = ceil(k A[k] / (2^53 - k)), from the first sum that can round
    assert int(a.A[k - 1]) <= (1 << 53) < int(a.A[k]) and int(a.eps[k]) == -((-k * int(a.A[k])) // ((1 << 53) - k))
    x = np.rint(rng.standard_normal(n) * 5 * 2.0 ** 30) * 2.0 ** -30
    for above in (True, False):
        ca, cb = rr.Clump(x, 0.25, above, "int64"), rr.Clump(x, 0.25, above, "int", unit=-rr.GRID_BITS)
        for fa, fb in zip(ca.prefix.froms(), cb.prefix.froms()):
            assert np.array_equal(fa, fb)
        for L in (1, 64, 5000):
            for ba, bb in zip(ca.bounds(L), cb.bounds(L)):
                assert np.array_equal(ba, bb)


def test_int64_back_end_refuses_what_it_cannot_hold():
    with pytest.raises(AssertionError):
        rr.Prefix(np.array([0.1, 0.2]), "int64")                                  # off the grid
    with pytest.raises(AssertionError):
        rr.Clump(np.array([1.0, 2.0]), 0.1, True, "int64")                        # the threshold is
    with pytest.raises(AssertionError):
        rr.Prefix(np.full(1 << 12, 2.0 ** 21), "int64")                           # sum |d| 2^30 = 2^63


@pytest.mark.parametrize("n", [1, 2, 100, 4095, 4096, 4097, 100003])
def test_exactly_summable_input_leaves_nothing_open(n):
    """read depth against a dyadic threshold (the shapes of test_clump_anticlump_bit_exact): no sum rounds, eps is 0,
    and strict == lenient == the reference, bit for bit"""
    x = cpu.synth_coverage(20240611, 3, 0, n, 0)
    for T in (float(np.floor(np.median(x))) + 0.5, float(np.floor(x.mean())) - 0.25):
        for above in (True, False):
            c = rr.Clump(x, T, above)
            assert not any(c.prefix.eps)
            for L in (1, 7, 63, 64, 100, 5000):
                strict, lenient = c.bounds(L)
                assert np.array_equal(strict, lenient)
                assert bits_equal(strict.astype(np.float64), cpu.clump(x, T, L, above)), (T, above, L)


GROUPS = rc.clump_groups()


@pytest.mark.parametrize("group", GROUPS, ids=[g[0] for g in GROUPS])
def test_reference_clump_lies_inside_the_sandwich(group):
    """every input of test_hip_clump_real.py: the conditions that test asserts, and strict <= cpu.clump <= lenient"""
    name, cls, kind, n, above, pct = group
    v, T = rc.clump_input(cls, kind, n, above, pct)
    c = rr.Clump(v, T, above, "int64" if cls == "grid" else None)
    for L in rc.lengths(kind, n, pct):
        strict, lenient = c.bounds(L)
        open_share = float(np.mean(strict != lenient))
        assert rr.runs(strict) >= 3 and 0.02 <= strict.mean() <= 0.98 and open_share < rc.CAPS[cls], (
            L, rr.runs(strict), strict.mean(), open_share)
        assert np.all(strict <= lenient)
        got = cpu.clump(v, T, L, above) == 1.0
        assert np.all(strict <= got) and np.all(got <= lenient), (L, T, open_share)


@pytest.mark.parametrize("kind", ["depth", "noise", "smooth"])
def test_sandwich_rejects_a_result_that_is_one_base_off(kind):
    """the reference's output moved by one base, or with every run one base longer, is outside"""
    for pct in (85, 25):
        v, T = rc.clump_input("natural", kind, 20011, pct == 85, pct)
        strict, lenient = rr.clump_bounds(v, T, 64, pct == 85)
        got = cpu.clump(v, T, 64, pct == 85) == 1.0
        for wrong in (np.roll(got, 1), np.roll(got, -1), got | np.roll(got, 1), got & np.roll(got, 1)):
            assert not (np.all(strict <= wrong) and np.all(wrong <= lenient))


def test_tenths_are_decided_by_rounding():
    """the adversarial class is what it claims to be: the sandwich is really open there, and nowhere on read depth"""
    v = rc.tenths(20011)
    strict, lenient = rr.clump_bounds(v, 0.2, 1, False)
    assert 0.01 < np.mean(strict != lenient) < rc.CAPS["tenths"]


@pytest.mark.parametrize("kind", ["depth", "positive", "mixed", "smooth"])
def test_reference_cumulative_sum_is_within_eps(kind):
    v = rc.cumsum_signal(kind)
    exact, eps = rr.cumsum_exact(v)
    assert np.all(np.diff(eps) >= 0) and eps[0] == 0
    got = cpu.cumulative_sum(v)
    assert np.all(np.abs(got - exact) <= eps)
    if kind == "depth":
        assert not eps.any() and bits_equal(exact, np.cumsum(v))
    else:
        assert np.abs(v).min() > eps[-1] > 0
        for n in rc.CUMSUM_LENGTHS:                         # a prefix of the signal has the prefix of its sums, and the
            if n <= 16385:                                  # same bound up to the unit it is rounded up in
                e2, eps2 = rr.cumsum_exact(v[:n])
                assert bits_equal(e2, exact[:n]) and (n <= 2 or np.allclose(eps2[-1], eps[n - 1], rtol=1e-6, atol=0))


def test_cumsum_bound_sees_a_lost_or_doubled_term():
    """what the bound is for: one term of the running sum lost, doubled, or carried from the wrong place"""
    v = rc.cumsum_signal("mixed")
    exact, eps = rr.cumsum_exact(v)
    for k, times in ((8192, 0.0), (524288, 2.0), (1000002, 0.0)):
        w = np.array(v)
        w[k] *= times
        bad = np.abs(np.cumsum(w) - exact) <= eps
        assert bad[:k].all() and not bad[k:].any()
