"""The checker of localmad / hampel (tests/localmad_ref.py) held four ways, on the CPU: bit for bit against a literal
per-base loop in Python floats; against slidingpercentile's checker for the median; against
scipy.stats.median_abs_deviation on whole odd windows; and by telling the definition from its near neighbours (another
median for even counts, another rank for the MAD, deviations from the mean, the median taken unfolded)."""
import numpy as np
import pytest

import localmad_ref as ref
import sliding_percentile_ref as sp

DBL_MAX = float(np.finfo(np.float64).max)
KINDS = ["real", "depth", "constant", "up", "down", "zeros", "subnormal", "huge"]
SHAPES = ((1, 1), (2, 3), (5, 4), (40, 11), (97, 2), (300, 100), (301, 101), (64, 200))
SETTINGS = [dict(), dict(scale=2.5, threshold=1.5, minmad=0.75), dict(threshold=0.0, minmad=0.0)]


def data(kind, n, rng):
    if kind == "real":
        return rng.standard_normal(n) * 10.0
    if kind == "depth":
        return rng.integers(0, 8, n).astype(np.float64)
    if kind == "constant":
        return np.full(n, 3.25)
    if kind == "up":
        return np.sort(rng.standard_normal(n))
    if kind == "down":
        return -np.sort(rng.standard_normal(n))
    if kind == "zeros":
        return np.where(np.arange(n) % 2 == 0, 0.0, -0.0)
    if kind == "subnormal":
        return rng.integers(-50, 50, n).astype(np.float64) * 5e-324
    if kind == "huge":
        return rng.choice(np.array([DBL_MAX, -DBL_MAX, np.nextafter(DBL_MAX, 0), -np.nextafter(DBL_MAX, 0), 1e308]), n)
    raise ValueError(kind)


def same(a, b):
    """the same bytes; a NaN (inf / inf, the z-score of an overflowed deviation) counts as a NaN whatever its sign and
    payload, which IEEE 754 leaves open"""
    a, b = np.array(a, np.float64), np.array(b, np.float64)
    a[np.isnan(a)] = np.nan
    b[np.isnan(b)] = np.nan
    return a.tobytes() == b.tobytes()


def literal(v, W, scale=ref.SCALE, threshold=ref.THRESHOLD, minmad=None, mutant=None):
    """the definition, base by base, in Python floats (IEEE doubles, every operation rounded once)"""
    keys = sp.key_of(v)
    n = len(v)
    left, right = sp.reach(W)
    out = {w: [] for w in ref.WHAT}
    for i in range(n):
        a, b = max(0, i - left), min(n - 1, i + right) + 1
        win = [float(x) for x in v[a:b]]
        m = len(win)
        k = sp.rank(m, 50000)
        kmed = (m - 1) // 2 if mutant == "lower median" else k
        if mutant == "unfolded":
            med = sorted(win, key=lambda x: (x, np.signbit(x) == 0))[kmed]          # (-0.0 before +0.0, as it came)
        else:
            med = float(sp.value_of(np.array([sorted(int(q) for q in keys[a:b])[kmed]], np.uint64))[0])
        centre = med
        if mutant == "mean":
            centre = sum(win) / m
        devs = sorted(abs(x - centre) for x in win)
        mad = devs[k - 1] if (mutant == "rank k-1" and k > 0) else devs[k]
        madf = minmad if (minmad is not None and minmad > mad) else mad
        sigma = scale * madf
        x = win[i - a]
        diff = 0.0 if x == med else x - med
        limit = threshold * sigma
        outlier = abs(diff) > limit
        if sigma == 0:
            z = 0.0
        elif np.isinf(diff) and np.isinf(sigma):
            z = float("nan")
        else:
            z = diff / sigma
        for w, val in (("zscore", z), ("median", med), ("mad", madf), ("difference", diff),
                       ("clean", med if outlier else x), ("outlier", 1.0 if outlier else 0.0)):
            out[w].append(val)
    return {w: np.array(out[w], np.float64) for w in ref.WHAT}


@pytest.mark.parametrize("kind", KINDS)
def test_checker_matches_a_literal_loop(kind):
    rng = np.random.default_rng(KINDS.index(kind))
    for n, W in SHAPES:
        v = data(kind, n, rng)
        for kw in SETTINGS:
            got, want = ref.figures(v, W, **kw), literal(v, W, **kw)
            for w in ref.WHAT:
                assert same(got[w], want[w]), (kind, n, W, kw, w)
        assert same(ref.local_mad(v, W), literal(v, W)["zscore"]) and same(ref.hampel(v, W), literal(v, W)["clean"])


@pytest.mark.parametrize("kind", KINDS)
def test_the_block_rule_gives_the_same_mad(kind):
    """the kernel's road: the k+1 smallest deviations are a contiguous block of the sorted window"""
    rng = np.random.default_rng(100 + KINDS.index(kind))
    for n, W in SHAPES:
        v = data(kind, n, rng)
        med, mad = ref.med_mad(v, W)
        for i in range(n):
            a, m = ref.block(ref.window_of(v, W, i))
            assert np.float64(m).tobytes() == mad[i].tobytes(), (kind, n, W, i, a)


@pytest.mark.parametrize("kind", KINDS)
def test_the_median_is_slidingpercentiles(kind):
    rng = np.random.default_rng(200 + KINDS.index(kind))
    for n, W in SHAPES + ((5000, 101), (3000, 1000)):
        v = data(kind, n, rng)
        assert ref.local_mad(v, W, "median").tobytes() == sp.sliding_percentile(v, W, 50000).tobytes(), (kind, n, W)


@pytest.mark.parametrize("W", [1, 3, 11, 101, 1001])
def test_the_mad_is_scipys_on_whole_odd_windows(W):
    from numpy.lib.stride_tricks import sliding_window_view
    from scipy.stats import median_abs_deviation
    v = np.random.default_rng(W).standard_normal(4000) * 7.0
    left, right = sp.reach(W)
    want = median_abs_deviation(sliding_window_view(v, W), axis=1)
    got = ref.local_mad(v, W, "mad")[left:v.size - right]
    assert got.tobytes() == np.ascontiguousarray(want, np.float64).tobytes()
    assert same(ref.local_mad(v, W, "mad", minmad=0.0), ref.local_mad(v, W, "mad"))


@pytest.mark.parametrize("mutant", ["lower median", "rank k-1", "mean", "unfolded"])
def test_checker_tells_the_definition_from(mutant):
    """each near neighbour of the definition gives other bytes than the checker on data made to show it; the literal loop
    without the mutation gives the checker's"""
    rng = np.random.default_rng(7)
    if mutant == "unfolded":
        v, W = np.array([-0.0, -0.0, 1.0, -0.0, -0.0, 2.0, -0.0]), 3
    else:
        v, W = rng.integers(0, 50, 200).astype(np.float64) + rng.random(200), 4      # (even windows inside, odd at the left end)
    got = ref.figures(v, W)
    plain, other = literal(v, W), literal(v, W, mutant=mutant)
    assert all(same(got[w], plain[w]) for w in ref.WHAT)
    differs = [w for w in ref.WHAT if not same(got[w], other[w])]
    expected = {"lower median": "median", "rank k-1": "mad", "mean": "mad", "unfolded": "median"}[mutant]
    assert expected in differs, (mutant, differs)


def test_w1_and_the_edges():
    v = np.array([3.0, -1.0, 7.5, 0.0, -0.0])
    f = ref.figures(v, 1)
    assert f["clean"].tobytes() == v.tobytes() and not f["outlier"].any() and not f["mad"].any()
    assert f["median"].tobytes() == np.array([3.0, -1.0, 7.5, 0.0, 0.0]).tobytes()          # (-0.0 folded)
    # W = 4: left 1, right 2; base 0 sees [3, -1, 7.5] (k = 1: med 3, devs 0 4 4.5: mad 4), base 4 sees [0, -0] (k = 1)
    med, mad = ref.med_mad(v, 4)
    assert (med[0], mad[0]) == (3.0, 4.0) and (med[4], mad[4]) == (0.0, 0.0)
    assert ref.block(np.array([3.0, -1.0, 7.5])) == (0, 4.0)                                # (-1 .. 3 against 3 .. 7.5)
