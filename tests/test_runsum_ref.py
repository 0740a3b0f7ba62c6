"""CPU: the exact running-sum checker (runsum_ref.py) against the literal definition, against itself (two back ends)
and against the restated reference -- the evidence that its bounds are right before a GPU is involved.  For the window
sums (slidingsum, sum) that evidence is a list of correct evaluations in different orders, all accepted, and a list of
wrong ones, each rejected at every base it touches, on every class of signal the GPU tests use."""
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


# --------------------------------------------------------------------------------- window sums: slidingsum and sum ----

WIN_N = 9001                                    # two tiles of the prefix form and a few bases, up to five of the block form


def _prefix(kind, n=WIN_N):
    v = rc.window_signal(kind)[:n]
    return v, rr.Prefix(v, "int64" if kind == "grid" else None)


def _bounds(v, W):
    c = np.arange(v.size)
    rgt = (W - 1) // 2
    lft = W - 1 - rgt
    return lft, rgt, np.maximum(c - lft, 0), np.minimum(c + rgt, v.size - 1)


def _padded(v, W):
    """v with the zeros the window reaches beyond either end: entry c + j is base c - lft + j"""
    lft, rgt, _, _ = _bounds(v, W)
    return np.concatenate((np.zeros(lft), v, np.zeros(rgt)))


def _rounded(p, lo, hi):
    """the exact sum over [lo, hi] per entry, rounded once (no more than the bases given: a mutant's wrong windows too)"""
    P = p.padded()[0]
    return p._to_float(P[hi + 1] - P[lo], False)


def _one_by_one(v, W, order):
    vp, acc = _padded(v, W), np.zeros(v.size)
    for j in order:
        acc = acc + vp[j:j + v.size]                        # (adding a padding zero changes nothing)
    return acc


def _tile_prefix(v, W, tile=rr.TILE):
    """sliding_sum_kernel: a running sum from the first base a workgroup stages (its first window's left end), and
    the difference of two of its values per output"""
    vp, out = _padded(v, W), np.empty(v.size)
    for t0 in range(0, v.size, tile):
        P = np.concatenate((np.zeros(1), np.cumsum(vp[t0:t0 + tile + W])))
        k = min(tile, v.size - t0)
        out[t0:t0 + k] = P[W:W + k] - P[:k]
    return out


def _cumsum_differenced(v, W):
    _, _, lo, hi = _bounds(v, W)
    S = np.concatenate((np.zeros(1), np.cumsum(v)))
    return S[hi + 1] - S[lo]


SLIDING_ORDERS = {"ascending": lambda v, W: _one_by_one(v, W, range(W)),
                  "descending": lambda v, W: _one_by_one(v, W, range(W - 1, -1, -1)),
                  "pairwise": lambda v, W: np.lib.stride_tricks.sliding_window_view(_padded(v, W), W).sum(axis=1),
                  "tile prefix": _tile_prefix,
                  "cumsum": _cumsum_differenced}
DENOMS = (1.0, 0.25, 3.0, -7.0)


def _within(got, exact, allow):
    return np.abs(got - exact) <= allow


@pytest.mark.parametrize("kind", rc.WINDOW_SIGNALS)
def test_sliding_checker_accepts_every_order(kind):
    """tiled routes: one by one in either direction, numpy's pairwise sum, and a tile-relative running sum differenced
    (staged span = window + tile); an exactly summable span (grid) leaves nothing open, and every order gives the bits"""
    v, p = _prefix(kind)
    for W in (1, 2, 3, 4, 101, 160, 2049, 4096, WIN_N + 1000, 14332):
        sl = rr.Sliding(p, W)
        assert sl.tiled
        for name in ("ascending", "descending", "pairwise", "tile prefix"):
            if name != "tile prefix" and W > 200 and W != 2049:
                continue                                    # (W vector additions each: the long ones once)
            s = SLIDING_ORDERS[name](v, W)
            for den in DENOMS:
                exact, allow = sl.over(den)
                assert _within(s / den, exact, allow).all(), (W, name, den)
                if kind == "grid":
                    assert bits_equal(s / den, exact) and (allow.max() == 0.0) == (den in (1.0, 0.25)), (W, name, den)
                elif W > 1:
                    assert allow.min() > 0.0


@pytest.mark.parametrize("kind", rc.WINDOW_SIGNALS)
def test_sliding_checker_accepts_the_whole_vector_route(kind):
    """W > 14332: np.cumsum differenced, on 40 009 bases (windows inside the vector, cut by either end, and W > n)"""
    v, p = _prefix(kind, 40009)
    cs, eps = rr.cumsum_exact(v, p.backend)
    for W in (14333, 20000, 50000, 100000):
        sl = rr.Sliding(p, W)
        assert not sl.tiled
        _, _, lo, hi = _bounds(v, W)
        s = _cumsum_differenced(v, W)
        for den in DENOMS:
            exact, allow = sl.over(den)
            assert _within(s / den, exact, allow).all(), (W, den)
        exact, allow = sl.over(1.0)                         # E = eps[hi] + eps[lo-1], and the rounded exact difference
        want = eps[hi] + np.where(lo > 0, eps[lo - 1], 0.0)
        assert np.all(allow >= want) and np.allclose(allow, want, rtol=1e-12, atol=0)
        assert bits_equal(exact, _rounded(p, lo, hi))
        if kind == "grid":
            assert not allow.any() and bits_equal(s, exact)


def test_window_sum_back_ends_agree():
    v = rc.window_signal("grid")[:WIN_N]
    a, b = rr.Prefix(v, "int64"), rr.Prefix(v, "int", unit=-rr.GRID_BITS)
    w = np.array(v)
    w[::3] *= 2.0 ** 13                                     # sums that do round, still on the grid
    c, d = rr.Prefix(w, "int64"), rr.Prefix(w, "int", unit=-rr.GRID_BITS)
    for x, y in ((a, b), (c, d)):
        for W in (3, 4, 1000, 5000, 14332, 14333, 20000):
            for den in DENOMS:
                for g, h in zip(rr.Sliding(x, W).over(den), rr.Sliding(y, W).over(den)):
                    assert bits_equal(g, h), (W, den)
            for args in ((1.0, False, 0.0), (float(W), False, 0.0), (1.0, True, -1.0)):
                for g, h in zip(rr.window_exact(x, W, *args), rr.window_exact(y, W, *args)):
                    assert np.array_equal(g, h), (W, args)
    assert rr.Sliding(c, 5000).over(1.0)[1].max() > 0.0


def test_sliding_exact_is_the_literal_definition():
    """sum.c:436-455 in exact rationals, odd and even W, W > n; the quotient is rounded once"""
    rng = np.random.default_rng(rc.SEED + 2)
    for it in range(60):
        n = int(rng.integers(1, 40))
        W = int(rng.integers(1, 2 * n + 3))
        den = (1.0, 0.25, 3.0, float(W), -7.0)[it % 5]
        v = rng.standard_normal(n) * 3 if it % 2 else np.rint(rng.standard_normal(n) * 2.0 ** 32) * 2.0 ** -30
        exact, allow = rr.sliding_exact(v, W, den)
        hOff = (W - 1) // 2
        for c in range(n):
            lo, hi = max(0, c + hOff - W + 1), min(n - 1, c + hOff)                # the running sum after step c + hOff
            q = sum(Fraction(float(x)) for x in v[lo:hi + 1]) / Fraction(den)
            assert exact[c] == float(q), (it, c)
            assert abs(Fraction(float(cpu.sliding_sum(v, W, den)[c])) - q) <= Fraction(float(allow[c])), (it, c)


def _seam(v, W, limit):
    """the first tile seam whose two neighbours differ by more than limit"""
    outs = rc.sliding_outs(W)
    for s in range(outs, v.size, outs):
        if abs(v[s] - v[s - 1]) > limit:
            return s
    raise AssertionError("no seam with distinct neighbours")


@pytest.mark.parametrize("kind", rc.WINDOW_SIGNALS)
def test_sliding_checker_rejects_every_mutant(kind):
    """each wrong result is outside the allowance at EVERY base it touches (and nowhere else).  20 011 bases: the
    smoothed signal has plateaus of equal values (flat depth for more than 101 bases) and the first tile seams lie in
    them; a term replaced by an equal neighbour is no mutant.  Likewise a third of `positive` is exactly 16.0 (depth 0),
    so a window moved by one base holds the same values at about half of the bases."""
    v, p = _prefix(kind, 20011)
    n = v.size
    c = np.arange(n)
    small = np.abs(v).min()
    for W in (3, 4, 100, 161, 2048, 2049, 4001):
        lft, rgt, lo, hi = _bounds(v, W)
        outs = rc.sliding_outs(W)
        sl = rr.Sliding(p, W)
        good = _rounded(p, lo, hi)
        for den in (1.0, 0.25, 3.0, float(W)):
            exact, allow = sl.over(den)
            assert small > 2 * (allow * abs(den)).max()                              # what the GPU test asserts per case
            everywhere = np.ones(n, bool)
            s = _seam(v, W, 2 * (allow * abs(den)).max())
            mutants = {"first term dropped": (good - v[lo], everywhere),
                       "last term dropped": (good - v[hi], everywhere),
                       "a term counted twice": (good + v, everywhere),
                       "zero padding replaced by v[0]": (good + v[0] * np.maximum(lft - c, 0), c < lft),
                       "zero padding replaced by v[n-1]": (good + v[-1] * np.maximum(c + rgt - (n - 1), 0), c + rgt > n - 1),
                       "a seam term replaced by its neighbour": (good + np.where((lo <= s) & (s <= hi), v[s - 1] - v[s], 0.0),
                                                                 (lo <= s) & (s <= hi)),
                       "min|v| carried into one tile": (good + np.where((c >= outs) & (c < 2 * outs), small, 0.0),
                                                        (c >= outs) & (c < 2 * outs))}
            for name, (m, touched) in mutants.items():
                assert touched.any(), name
                ok = _within(m / den, exact, allow)
                assert not ok[touched].any() and ok[~touched].all(), (W, den, name, int(ok[touched].sum()))
            # a window moved by one base differs from the right one by v[hi+1] - v[lo] (or one of them at an end)
            for name, shift in (("shifted down", -1), ("shifted up / lft and rgt swapped", 1)):
                mlo, mhi = np.clip(c + shift - lft, 0, n - 1), np.clip(c + shift + rgt, 0, n - 1)
                gained = np.where(mhi > hi, v[mhi], 0.0) - np.where(mlo < lo, v[mlo], 0.0)
                lost = np.where(mlo > lo, v[lo], 0.0) - np.where(mhi < hi, v[hi], 0.0)
                touched = np.abs(gained - lost) > 2 * allow * abs(den)
                assert touched.mean() > (0.4 if kind in ("positive", "smooth") else 0.9), (W, name, touched.mean())
                ok = _within(_rounded(p, mlo, mhi) / den, exact, allow)
                assert not ok[touched].any(), (W, den, name)
            if W % 2 == 0:                                  # (even W: [c-rgt, c+lft] is the window of base c+1)
                assert bits_equal(_rounded(p, np.clip(c - rgt, 0, n - 1), np.clip(c + lft, 0, n - 1)), _rounded(p, mlo, mhi))
            wrong = _within(good / (den * (W + 1) / W), exact, allow)               # W + 1 where W was meant
            assert wrong.mean() < 0.01, (W, den, wrong.mean())


def _wide_kernel_order(x):
    """window_sum_wide_kernel: 256 strided partial sums, then a halving tree"""
    part = np.zeros(256)
    for j in range(0, x.size, 256):
        part[:x[j:j + 256].size] += x[j:j + 256]
    d = 128
    while d:
        part[:d] += part[d:2 * d]
        d //= 2
    return part[0]


SUM_ORDERS = (lambda x: float(np.cumsum(x)[-1]), lambda x: float(np.cumsum(x[::-1])[-1]), lambda x: float(np.sum(x)),
              _wide_kernel_order)


@pytest.mark.parametrize("kind", rc.WINDOW_SIGNALS)
def test_window_sum_checker_accepts_and_rejects(kind):
    """`sum`: windows of W bases and a ragged last one; every order of a window's terms is accepted, every mutant is
    rejected at the window it touches"""
    v, p = _prefix(kind)
    n = v.size
    for W in (1000, 1001, 2700, 9000, 9001, 20000):
        starts = np.arange(0, n, W)
        ends = np.minimum(starts + W, n)
        ragged = int(ends[-1] - starts[-1])
        assert (ragged != W) == (W not in (9001,))
        for den, actual, zero in ((1.0, False, 0.0), (float(W), False, 0.0), (0.25, False, 7.0), (1.0, True, -1.0)):
            exact, allow, is_sum = rr.window_exact(p, W, den, actual, zero)
            assert np.array_equal(np.flatnonzero(is_sum), starts)
            assert bits_equal(exact[~is_sum], np.full(n - starts.size, zero)) and not allow[~is_sum].any()
            dens = (ends - starts).astype(np.float64) if actual else np.full(starts.size, den)
            assert v[:n].__abs__().min() > 2 * (allow[starts] * np.abs(dens)).max()
            if kind == "grid":
                assert (allow.max() == 0.0) == (not actual and den != float(W))
            for order in SUM_ORDERS:
                got = np.full(n, zero)
                got[starts] = [order(v[a:b]) / d for a, b, d in zip(starts, ends, dens)]
                assert _within(got, exact, allow).all(), (W, den, actual)
                assert bits_equal(got[~is_sum], exact[~is_sum])
                if kind == "grid":
                    assert bits_equal(got, exact)
            if not actual:                                  # the restated reference, the same call
                assert _within(cpu.window_sum(v, W, den, False, zero), exact, allow).all()
            good = _rounded(p, starts, ends - 1)
            k = starts.size - 1
            mutants = {"first term dropped": (good - v[starts]) / dens,
                       "last term dropped": (good - v[ends - 1]) / dens,
                       "a term counted twice": (good + v[starts + (ends - starts) // 2]) / dens,
                       "the next window's first base taken in": (good + np.where(ends < n, v[np.minimum(ends, n - 1)], v[0])) / dens,
                       "the wrong denominator": good / (dens * (W + 1) / W),
                       "zero at a window's first base": np.full(starts.size, zero + 0.0)}
            for name, m in mutants.items():
                ok = _within(m, exact[starts], allow[starts])
                assert not ok.any(), (W, den, actual, name)
            if actual and ragged != W:
                m = good / dens
                m[k] = good[k] / W                          # the ragged last window divided by W
                ok = _within(m, exact[starts], allow[starts])
                assert ok[:k].all() and not ok[k]
