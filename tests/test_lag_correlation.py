"""crosscorrelate / autocorrelate (not in the reference) through the library: gdsp_lag_products_batch and
gdsp_genome_lag_correlation of include/genodsp_hip.h.  Every sum is exact and rounded once, so everything here is bit for
bit against the exact checker tests/lagcorr_ref.py -- itself checked against fractions.Fraction -- at the shapes where
the kernel changes its route: chromosomes shorter than a tile or than a lag, the tiles at a chromosome's ends and the
clean ones between them, the last lag block, values that flush, overflow or are not finite."""
import math
import os
import random
from fractions import Fraction

import numpy as np
import pytest

import lagcorr_ref as lref
import xsum_ref as ref
from conftest import ROOT

FIGURES = lref.FIGURES
WORDS = 72
TILE, BLOCK = 1024, 256                            # gdsp_lag_tile(), gdsp_lag_block(): test_tile_and_block_are_what_the_shapes_assume


def gd():
    import genodsp_amd
    return genodsp_amd


def bits(x):
    return np.float64(x).tobytes()


# ------------------------------------------------------------------------------------------------ CPU ----

def small_genomes():
    """100 small genomes of one to three chromosomes of 1 .. 40 bases: plain values, integers, values of very different
    sizes, and some NaN and inf"""
    rnd = random.Random(29)
    out = []
    for i in range(100):
        pairs = []
        for _ in range(1 + i % 3):
            n = 1 if i < 3 else rnd.randint(1, 40)
            kind = i % 4
            if kind == 0:
                x = [rnd.gauss(0, 10) for _ in range(n)];  y = [rnd.gauss(3, 2) for _ in range(n)]
            elif kind == 1:
                x = [float(rnd.randint(0, 60)) for _ in range(n)];  y = [2 * v + rnd.randint(-3, 3) for v in x]
            elif kind == 2:
                x = [math.ldexp(rnd.gauss(0, 1), rnd.randint(-300, 300)) for _ in range(n)]
                y = [math.ldexp(rnd.gauss(0, 1), rnd.randint(-300, 300)) for _ in range(n)]
            else:
                x = [rnd.choice([math.nan, math.inf, -math.inf]) if rnd.random() < 0.15 else rnd.gauss(1e6, 1e-3) for _ in range(n)]
                y = [rnd.choice([math.nan, math.inf]) if rnd.random() < 0.15 else rnd.gauss(-5, 1) for _ in range(n)]
            pairs.append((np.array(x, np.float64), np.array(y, np.float64)))
        out.append(pairs)
    return out


def test_checker_agrees_with_fraction():
    """Python floats for the per-product roundings (each operation IEEE double), Fractions for the sums"""
    checked = 0
    for pairs in small_genomes():
        fig, counts, cov, corr = lref.curve(pairs, -5, 11)
        f = dict(zip(FIGURES, fig))
        both = [(a, b) for x, y in pairs for a, b in zip(x.tolist(), y.tolist()) if math.isfinite(a) and math.isfinite(b)]
        N = len(both)
        assert f["count"] == N
        if N == 0:
            assert all(math.isnan(c) for c in cov) and counts == [0] * 11
            continue
        meanx = float(sum(Fraction(a) for a, _ in both) / N)
        meany = float(sum(Fraction(b) for _, b in both) / N)
        assert bits(f["meanx"]) == bits(meanx) and bits(f["meany"]) == bits(meany)
        for k, d in enumerate(range(-5, 6)):
            q, n = Fraction(0), 0
            for x, y in pairs:
                xs, ys = x.tolist(), y.tolist()
                for i in range(len(xs)):
                    if 0 <= i + d < len(xs) and math.isfinite(xs[i]) and math.isfinite(ys[i + d]):
                        q += Fraction((xs[i] - meanx) * (ys[i + d] - meany))
                        n += 1
            assert counts[k] == n
            assert bits(cov[k] + 0.0) == bits(float(q / N) + 0.0), (d, cov[k], float(q / N))
            checked += 1
    assert checked > 900


def test_checkers_identities():
    seen = 0
    for pairs in small_genomes():
        fig, counts, cov, corr = lref.curve(pairs, -5, 11)
        f = dict(zip(FIGURES, fig))
        # lag 0 is correlate
        assert ref.same(cov[5], f["covariance"]) and ref.same(corr[5], f["correlation"]) and counts[5] == f["count"]
        # swapping x and y maps d to -d
        sfig, scounts, scov, scorr = lref.curve([(y, x) for x, y in pairs], -5, 11)
        assert scounts == counts[::-1]
        assert all(ref.same(a, b) for a, b in zip(scov, cov[::-1])) and all(ref.same(a, b) for a, b in zip(scorr, corr[::-1]))
        # the autocorrelation is symmetric, and its lag 0 is the variance and 1
        afig, acounts, acov, acorr = lref.curve([(x, x) for x, y in pairs], -5, 11)
        af = dict(zip(FIGURES, afig))
        assert acounts == acounts[::-1] and all(ref.same(a, b) for a, b in zip(acov, acov[::-1]))
        assert all(ref.same(a, b) for a, b in zip(acorr, acorr[::-1]))
        if af["count"] > 0:
            assert ref.same(acov[5], af["varx"])
            if not math.isnan(acorr[5]):
                assert abs(acorr[5] - 1.0) <= 2.0 ** -51
                assert all(-1.0 <= c <= 1.0 for c in acorr)
                seen += 1
    assert seen > 60
    assert lref.best([-1, 0, 1, 2], [0.5, math.nan, 0.5, 0.25]) == (-1, 0.5, 0.25)
    assert lref.best([2, 3], [0.5, 0.5]) == (2, 0.5, 0.5) and lref.best([0], [math.nan]) is None


def test_header_declares_the_lag_calls():
    text = open(os.path.join(ROOT, "include", "genodsp_hip.h")).read()
    for call in ("gdsp_lag_products_batch", "gdsp_genome_lag_correlation (", "gdsp_genome_lag_correlation_use_comm",
                 "gdsp_genome_lag_correlation_last", "gdsp_lag_tile", "gdsp_lag_block"):
        assert call in text, call
    assert "not by n(d)" in text
    g = gd()
    for name in ("lag_products", "genome_lag_correlation", "lag_tile", "lag_block"):
        assert callable(getattr(g, name)), name


def test_tile_and_block_are_what_the_shapes_assume():
    assert gd().lag_tile() == TILE and gd().lag_block() == BLOCK


# ------------------------------------------------------------------------------------------------ GPU ----

def dev():
    g = gd()
    g.set_device(0)
    return g


def up(g, pairs):
    return [(g.DeviceVector.from_numpy(x), g.DeviceVector.from_numpy(y)) for x, y in pairs]


def check(got, want, what=""):
    fig, counts, cov, corr = want
    for k, w in zip(FIGURES, fig):
        assert ref.same(got[k], w), (what, k, got[k], w)
    assert got["pairs"].tolist() == counts, what
    lags = got["lags"].tolist()
    for d, a, b in zip(lags, got["covariances"].tolist(), cov):
        assert ref.same(a, b), (what, "covariance", d, a, b)
    for d, a, b in zip(lags, got["correlations"].tolist(), corr):
        assert ref.same(a, b), (what, "correlation", d, a, b)


def same_images(a, b):
    """word for word but for the flush count and the spare word"""
    return np.array_equal(np.delete(a, [70, 71], axis=1), np.delete(b, [70, 71], axis=1))


def real(n, rng):
    return rng.standard_normal(n) * 10.0


def depth(n, rng):
    return rng.integers(0, 60, n).astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 7])
def test_lengths_around_the_tile(n):
    """lags -(B+1) .. B+1: three lag blocks, the last of three lags; chromosomes shorter than |lag| give no products"""
    g = dev()
    rng = np.random.default_rng(n)
    for make in (real, depth):
        pairs = [(make(n, rng), make(n, rng))]
        want = lref.curve(pairs, -(BLOCK + 1), 2 * BLOCK + 3)
        got = g.genome_lag_correlation(up(g, pairs), -(BLOCK + 1), 2 * BLOCK + 3)
        check(got, want, (n, make.__name__))
        assert got["pairs"][BLOCK + 1] == n and got["pairs"][0] == max(0, n - BLOCK - 1)
        if n <= BLOCK:
            assert bits(got["covariances"][0]) == bits(0.0)               # a lag no chromosome is long enough for


def genome40(rng):
    sizes = [1, 2, 3000] + [int(s) for s in rng.integers(1, 3001, 37)]
    return [(real(n, rng), depth(n, rng)) for n in sizes]


@pytest.mark.gpu
def test_forty_chromosomes_in_one_call():
    """more than one launch (32 pairs each); the images, count words included, are the checker's"""
    g = dev()
    rng = np.random.default_rng(40)
    pairs = genome40(rng)
    want = lref.curve(pairs, -40, 90)
    d = up(g, pairs)
    check(g.genome_lag_correlation(d, -40, 90), want, "forty")
    f = dict(zip(FIGURES, want[0]))
    img = g.lag_products(d, -40, 90, f["meanx"], f["meany"])
    assert img.shape == (90, WORDS) and img[:, 68].tolist() == want[1]
    assert same_images(img, lref.images(pairs, -40, 90, f["meanx"], f["meany"]))
    last = g.genome_lag_correlation_last()
    assert last["count"] == f["count"] and last["products"] == sum(want[1]) and last["nonfinite_products"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("lag_lo", [-70000, 70000])
def test_lag_ranges_far_from_zero(lag_lo):
    g = dev()
    rng = np.random.default_rng(7)
    pairs = [(real(100000, rng), depth(100000, rng))]
    want = lref.curve(pairs, lag_lo, 300)
    got = g.genome_lag_correlation(up(g, pairs), lag_lo, 300)
    check(got, want, lag_lo)
    assert got["pairs"][0] == 100000 - abs(lag_lo)


@pytest.mark.gpu
@pytest.mark.parametrize("nlags", [1, BLOCK, BLOCK + 1, 4096])
def test_numbers_of_lags(nlags):
    g = dev()
    rng = np.random.default_rng(nlags)
    pairs = [(depth(5000, rng), depth(5000, rng))]
    lo = -(nlags // 2)
    check(g.genome_lag_correlation(up(g, pairs), lo, nlags), lref.curve(pairs, lo, nlags), nlags)


@pytest.mark.gpu
def test_y_at_an_odd_offset_against_x():
    g = dev()
    rng = np.random.default_rng(3)
    n = 3 * TILE + 7
    x, y = real(n, rng), real(n, rng)
    want = lref.curve([(x, y)], -9, 19)
    for ox, oy in ((0, 1), (1, 0), (1, 1)):
        vx = g.DeviceVector.from_numpy(np.concatenate([np.full(ox, 1e9), x, [7e8]]))
        vy = g.DeviceVector.from_numpy(np.concatenate([np.full(oy, -1e9), y, [-7e8]]))
        check(g.genome_lag_correlation([((vx, ox, n, 0), (vy, oy, n, 0))], -9, 19), want, (ox, oy))


@pytest.mark.gpu
def test_spread_exponents_flush_the_lanes():
    """exponents over +-300: nearly every product leaves a residual, which goes to the lag's device image"""
    g = dev()
    rng = np.random.default_rng(300)
    h = (3 * TILE + 8) // 2

    def spread():                                         # v and -v shuffled: the mean is exactly 0, so centring keeps the spread
        v = np.ldexp(rng.standard_normal(h), rng.integers(-300, 300, h))
        return rng.permutation(np.concatenate([v, -v]))

    pairs = [(spread(), spread())]
    want = lref.curve(pairs, -5, 11)
    assert want[0][3] == 0.0 and want[0][4] == 0.0
    check(g.genome_lag_correlation(up(g, pairs), -5, 11), want, "spread")
    assert g.genome_lag_correlation_last()["flushes"] > 0


def with_specials(v, rng, share=0.03):
    v = v.copy()
    pick = rng.random(v.size) < share
    v[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf]), int(pick.sum()))
    return v


@pytest.mark.gpu
def test_nan_and_inf_scattered_in_x_and_y():
    g = dev()
    rng = np.random.default_rng(17)
    n = 4 * TILE + 3
    x, y = with_specials(real(n, rng), rng), with_specials(depth(n, rng), rng)
    x[TILE:2 * TILE + 300] = real(TILE + 300, rng)                        # (one tile, and all it meets of y, stays clean)
    y[TILE - 50:2 * TILE + 350] = depth(TILE + 400, rng)
    pairs = [(x, y), (with_specials(real(700, rng), rng), real(700, rng))]
    want = lref.curve(pairs, -20, 41)
    got = g.genome_lag_correlation(up(g, pairs), -20, 41)
    check(got, want, "specials")
    assert 0 < got["count"] < n + 700 and got["pairs"][20] == got["count"] and not np.isnan(got["correlations"]).any()


@pytest.mark.gpu
def test_products_that_overflow():
    """+-1e200 against +-1e200: the lags at which two of them meet have no covariance, the others have"""
    g = dev()
    rng = np.random.default_rng(200)
    n = 3 * TILE + 7
    x, y = real(n, rng), real(n, rng)
    x[TILE + 100], y[TILE + 110] = 1e200, -1e200                          # lag 10, in a clean tile
    x[5], y[2] = -1e200, 1e200                                            # lag -3, in the first tile
    x[n - 1], y[n - 1], x[n - 2], y[n - 2] = 1e200, 1e200, -1e200, -1e200     # lags -1, 0, 1, in the last one; the means stay small
    pairs = [(x, y)]
    want = lref.curve(pairs, -12, 25)
    got = g.genome_lag_correlation(up(g, pairs), -12, 25)
    check(got, want, "overflow")
    nans = [int(d) for d, c in zip(got["lags"], got["covariances"]) if math.isnan(c)]
    assert nans == [-3, -1, 0, 1, 10]
    f = dict(zip(FIGURES, want[0]))
    bad = sum(b for _, _, b in lref.sums(pairs, -12, 25, f["meanx"], f["meany"]))
    assert g.genome_lag_correlation_last()["nonfinite_products"] == bad == 6


@pytest.mark.gpu
def test_identities_on_the_devices_own_outputs():
    g = dev()
    rng = np.random.default_rng(11)
    pairs = [(real(n, rng), depth(n, rng)) for n in (3 * TILE + 7, 500, 2 * TILE)]
    d = up(g, pairs)
    a = g.genome_lag_correlation(d, -30, 61)
    c = g.genome_correlation(d)
    assert ref.same(a["covariances"][30], c["covariance"]) and ref.same(a["correlations"][30], c["correlation"])
    for k in FIGURES:
        assert ref.same(a[k], c[k]), k
    b = g.genome_lag_correlation([(y, x) for x, y in d], -30, 61)
    assert a["pairs"].tolist() == b["pairs"][::-1].tolist()
    assert a["covariances"].tobytes() == b["covariances"][::-1].tobytes()
    assert a["correlations"].tobytes() == b["correlations"][::-1].tobytes()
    s = g.genome_lag_correlation([(x, x) for x, y in d], -30, 61)
    assert s["covariances"].tobytes() == s["covariances"][::-1].tobytes()
    assert s["correlations"].tobytes() == s["correlations"][::-1].tobytes()
    assert bits(s["covariances"][30]) == bits(s["varx"]) and abs(s["correlations"][30] - 1.0) <= 2.0 ** -51
    assert not np.isnan(a["correlations"]).any()


@pytest.mark.gpu
def test_order_split_and_hook_do_not_matter():
    """one genome: its chromosomes reversed; cut over two calls whose raw images are added as u64; and with half of it
    arriving through the allreduce hook, as another rank's images would"""
    g = dev()
    rng = np.random.default_rng(40)
    pairs = genome40(rng)
    lo, nlags = -(BLOCK + 4), 2 * BLOCK + 9
    want = lref.curve(pairs, lo, nlags)
    f = dict(zip(FIGURES, want[0]))
    d = up(g, pairs)
    check(g.genome_lag_correlation(d[::-1], lo, nlags), want, "reversed")

    whole = g.lag_products(d, lo, nlags, f["meanx"], f["meany"])
    halves = g.lag_products(d[:17], lo, nlags, f["meanx"], f["meany"]) + g.lag_products(d[17:], lo, nlags, f["meanx"], f["meany"])
    assert whole[:, 68].tolist() == halves[:, 68].tolist() == want[1]
    for k in range(nlags):
        assert bits(g.xsum_div_round(whole[k], int(f["count"]))) == bits(g.xsum_div_round(halves[k], int(f["count"]))) == bits(want[2][k])
    assert same_images(whole, lref.images(pairs, lo, nlags, f["meanx"], f["meany"]))

    mine, theirs = d[:17], d[17:]
    sizes, means = [], []

    def allreduce(arr, op):
        assert op == "sum"
        sizes.append(int(arr.size))
        if len(sizes) == 1:                                   # the sums of x and y
            other = g.xsum_pair_image(theirs)
            total = arr.reshape(2, WORDS) + other
            n = int(total[0][68])
            means[:] = [g.xsum_div_round(total[0], n), g.xsum_div_round(total[1], n)]
        elif len(sizes) == 2:                                 # qxx, qyy, qxy
            other = g.xsum_pair_image(theirs, means=tuple(means))
        else:                                                 # the lags' images
            other = g.lag_products(theirs, lo, nlags, means[0], means[1])
        return arr + other.ravel()

    check(g.genome_lag_correlation(mine, lo, nlags, allreduce=allreduce), want, "hook")
    assert sizes == [2 * WORDS, 3 * WORDS, nlags * WORDS]
