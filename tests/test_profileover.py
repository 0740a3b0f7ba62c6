"""profileover (not in the reference) through the library: gdsp_profile_accumulate_batch and gdsp_genome_profile of
include/genodsp_hip.h.  Every sum is exact and rounded once, so everything here is bit for bit against the exact checker
tests/profileover_ref.py -- itself checked against fractions.Fraction in test_profileover_ref.py -- at the shapes where
the kernel changes its route: chromosomes shorter than a window, anchors at and near both ends, the last offset block,
more anchors than a launch takes, values that flush, overflow or are not finite."""
import math

import numpy as np
import pytest

import anchor_cases as cases
import profileover_ref as pref
import xsum_ref as ref
from anchor_cases import depth, dev, every_base, random_anchors, real, up

WORDS = 72
B = 512                                            # gdsp_profile_block(): test_block_is_what_the_shapes_assume
DBL_MAX = ref.DBL_MAX
FIGURES = ("count", "sum", "mean", "variance", "stddev", "stderr")


def check(got, want, what=""):
    assert len(got["count"]) == len(want), what
    for j, w in enumerate(want):
        for name, x in zip(FIGURES, w):
            assert ref.same(got[name][j], x), (what, "column", j, name, got[name][j], x)


def same_images(a, b):
    """word for word but for the flush count and the spare word"""
    return np.array_equal(np.delete(a, [70, 71], axis=1), np.delete(b, [70, 71], axis=1))


def same_bits(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in FIGURES)


@pytest.mark.gpu
def test_block_is_what_the_shapes_assume():
    assert dev().profile_block() == B


# ------------------------------------------------------------------------------------------ shapes ----

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 5, B, 3 * B + 7])
def test_vector_lengths(n):
    """anchors at 0, at n-1 and everywhere between, on both strands, under a narrow window and one of three offset blocks"""
    g = dev()
    rng = np.random.default_rng(n)
    for make, (off_lo, noffsets) in ((depth, (-8, 17)), (real, (-8, 17)), (real, (-B, 2 * B + 1))):
        v = [make(n, rng)]
        anchors = every_base(n)
        want = pref.profile(v, anchors, off_lo, noffsets)
        got = g.genome_profile(up(g, v), anchors, off_lo, noffsets)
        check(got, want, (n, make.__name__, off_lo))
        assert got["count"][-off_lo] == 2 * n and got["count"][0] == 2 * max(0, n + off_lo)
        assert got["offsets"].tolist() == list(range(off_lo, off_lo + noffsets))


@pytest.mark.gpu
@pytest.mark.parametrize("off_lo", [-70000, 70000])
@pytest.mark.parametrize("noffsets", [1, B - 1, B, B + 1, 2 * B + 3, 16384])
def test_numbers_of_offsets_far_from_zero(noffsets, off_lo):
    """a vector that only some of the offsets reach, and only from some of the anchors"""
    g = dev()
    rng = np.random.default_rng(noffsets)
    n = 75000
    v = [real(n, rng)]
    pos = np.concatenate([rng.integers(0, 6000, 12), rng.integers(n - 6000, n, 12), [0, n - 1, 4999, n - 5000]])
    anchors = [(0, int(p), s) for p in pos for s in (1, -1)]
    want = pref.profile(v, anchors, off_lo, noffsets)
    got = g.genome_profile(up(g, v), anchors, off_lo, noffsets)
    check(got, want, (noffsets, off_lo))
    assert 0 < got["count"].max() < len(anchors)
    if noffsets == 16384 and off_lo > 0:
        assert got["count"].min() == 0                                    # (offsets beyond the vector's length)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 1, 2, 63, 64, 65, 1000, 5000])
def test_numbers_of_anchors(count):
    g = dev()
    rng = np.random.default_rng(count)
    v = [depth(2000, rng), real(301, rng)]
    anchors = random_anchors(v, count, rng)
    want = pref.profile(v, anchors, -40, 81)
    got = g.genome_profile(up(g, v), anchors, -40, 81)
    check(got, want, count)
    last = g.genome_profile_last()
    assert last["anchors"] == count and last["samples"] == sum(int(w[0]) for w in want)
    if count == 0:
        assert all(bits(s) == bits(0.0) for s in got["sum"]) and np.isnan(got["mean"]).all()
        assert np.array_equal(g.profile_images(up(g, v), [], -40, 81), np.zeros((81, WORDS), np.uint64))


def bits(x):
    return np.float64(x).tobytes()


@pytest.mark.gpu
def test_one_position_a_thousand_times():
    g = dev()
    rng = np.random.default_rng(1000)
    v = [real(700, rng)]
    anchors = [(0, 350, 1)] * 1000 + [(0, 3, -1)] * 1000
    want = pref.profile(v, anchors, -20, 60, bin=3)
    got = g.genome_profile(up(g, v), anchors, -20, 60, bin=3)
    check(got, want)
    once = g.genome_profile(up(g, v), [(0, 350, 1), (0, 3, -1)], -20, 60, bin=3)
    assert (got["count"] == 1000 * once["count"]).all()


@pytest.mark.gpu
def test_a_small_launch_chunk_gives_several_launches():
    """a thousand anchors 300 at a time: four launches per pass, each carried; the images are those of one launch"""
    g = dev()
    rng = np.random.default_rng(300)
    v = [real(900, rng), depth(1200, rng)]
    anchors = random_anchors(v, 1000, rng)
    off_lo, noffsets = -(B + 5), 2 * B + 10
    want = pref.profile(v, anchors, off_lo, noffsets, bin=2)
    d = up(g, v)
    whole = g.profile_images(d, anchors, off_lo, noffsets)
    g.profile_set_launch_anchors(300)
    try:
        got = g.genome_profile(d, anchors, off_lo, noffsets, bin=2)
        img = g.profile_images(d, anchors, off_lo, noffsets)
        means = pref.offset_means(want, 2)
        sq = g.profile_images(d, anchors, off_lo, noffsets, mean=means)
    finally:
        g.profile_set_launch_anchors(0)
    check(got, want)
    assert same_images(img, whole) and same_images(img, pref.images(v, anchors, off_lo, noffsets))
    assert same_images(sq, pref.images(v, anchors, off_lo, noffsets, mean=means))
    with pytest.raises(g.GdspError):
        g.profile_set_launch_anchors(1 << 29)


def genome40(rng):
    sizes = [1, 2, 3000] + [int(s) for s in rng.integers(1, 3001, 37)]
    return [real(n, rng) if i % 2 else depth(n, rng) for i, n in enumerate(sizes)]


@pytest.mark.gpu
def test_forty_chromosomes_in_one_call():
    """more than one launch sequence (32 vectors each); the images, count words included, are the checker's"""
    g = dev()
    rng = np.random.default_rng(40)
    v = genome40(rng)
    anchors = random_anchors(v, 3000, rng) + [(c, 0, 1) for c in range(40)] + [(c, v[c].size - 1, -1) for c in range(40)]
    want = pref.profile(v, anchors, -50, 120, bin=4)
    d = up(g, v)
    check(g.genome_profile(d, anchors, -50, 120, bin=4), want, "forty")
    img = g.profile_images(d, anchors, -50, 120)
    assert img.shape == (120, WORDS) and same_images(img, pref.images(v, anchors, -50, 120))
    assert int(img[:, 68].sum()) == sum(int(w[0]) for w in want) == g.genome_profile_last()["samples"]


@pytest.mark.gpu
def test_a_vector_at_an_odd_index():
    """8-byte but not 16-byte aligned: a stretch that starts at an odd index of an allocation"""
    g = dev()
    rng = np.random.default_rng(3)
    n = 3 * B + 7
    whole = real(n + 1, rng)
    buf = g.DeviceVector.from_numpy(whole)
    assert buf.ptr.value % 16 == 0
    v = [whole[1:]]
    anchors = every_base(n)[::3]
    want = pref.profile(v, anchors, -B, 2 * B)
    check(g.genome_profile([(buf, 1, n)], anchors, -B, 2 * B), want)
    assert same_images(g.profile_images([(buf, 1, n)], anchors, -B, 2 * B), pref.images(v, anchors, -B, 2 * B))


# ------------------------------------------------------------------------------------------ values ----

@pytest.mark.gpu
def test_spread_exponents_flush_the_lanes():
    """exponents over +-300: a lane's two terms cannot hold such a sum, the residuals go to the offset's device image"""
    g = dev()
    rng = np.random.default_rng(300)
    n = 4000
    v = [np.ldexp(rng.standard_normal(n), rng.integers(-996, 997, n).astype(np.int32))]       # 1e-300 .. 1e300
    anchors = random_anchors(v, 20000, rng)                               # (several per workgroup: a lane adds a few values)
    want = pref.profile(v, anchors, -30, 64, bin=2)
    d = up(g, v)
    check(g.genome_profile(d, anchors, -30, 64, bin=2), want)
    last = g.genome_profile_last()
    assert last["flushes"] > 0 and last["nonfinite_squares"] > 0          # (1e300 squared)
    img = g.profile_images(d, anchors, -30, 64)
    assert same_images(img, pref.images(v, anchors, -30, 64)) and int(img[:, 70].sum()) > 0


@pytest.mark.gpu
def test_nan_and_inf_scattered():
    g = dev()
    rng = np.random.default_rng(17)
    v = [real(2 * B + 3, rng), depth(900, rng)]
    for x in v:
        hit = rng.random(x.size) < 0.03
        x[hit] = rng.choice([np.nan, np.inf, -np.inf], int(hit.sum()))
    anchors = random_anchors(v, 800, rng) + [(0, 0, 1), (1, 899, -1)]
    want = pref.profile(v, anchors, -B, 2 * B, bin=8)
    got = g.genome_profile(up(g, v), anchors, -B, 2 * B, bin=8)
    check(got, want)
    assert g.genome_profile_last()["nonfinite_squares"] == 0
    wide = g.genome_profile(up(g, v), anchors, -B, 2 * B, bin=8, lo=-math.inf, hi=math.inf)
    assert same_bits(got, wide)                                           # (infinite limits do not let the infinities in)


@pytest.mark.gpu
def test_limits():
    g = dev()
    rng = np.random.default_rng(23)
    v = [depth(1500, rng), real(700, rng)]
    anchors = random_anchors(v, 500, rng)
    for lo, hi in ((1.0, DBL_MAX), (-DBL_MAX, 20.0), (5.0, 5.0), (100.0, 200.0)):
        want = pref.profile(v, anchors, -25, 50, bin=5, lo=lo, hi=hi)
        got = g.genome_profile(up(g, v), anchors, -25, 50, bin=5, lo=lo, hi=hi)
        check(got, want, (lo, hi))
    assert got["count"].max() == 0 and np.isnan(got["stderr"]).all()       # (nothing lies in 100 .. 200)


@pytest.mark.gpu
def test_sums_and_squares_that_overflow():
    """+-DBL_MAX: a column of several +DBL_MAX sums to +inf with a finite mean; where both signs meet every q is +inf"""
    g = dev()
    rng = np.random.default_rng(200)
    a = np.full(300, DBL_MAX)
    b = rng.choice([DBL_MAX, -DBL_MAX, 1.0], 400)
    v = [a, b]
    anchors = [(0, int(p), 1) for p in rng.integers(0, 300, 40)] + [(1, int(p), -1) for p in rng.integers(0, 400, 60)]
    for vecs, anc in (([a], anchors[:40]), (v, anchors)):
        want = pref.profile(vecs, anc, -10, 20)
        got = g.genome_profile(up(g, vecs), anc, -10, 20)
        check(got, want, len(vecs))
    assert g.genome_profile_last()["nonfinite_squares"] > 0 and np.isposinf(got["variance"]).all()
    only = g.genome_profile(up(g, [a]), anchors[:40], -10, 20)
    assert np.isposinf(only["sum"]).all() and (only["mean"] == DBL_MAX).all() and (only["variance"] == 0).all()


# -------------------------------------------------------------------------------------------- bins ----

@pytest.mark.gpu
@pytest.mark.parametrize("bin", [1, 7, 1050])
def test_bins(bin):
    """1050 offsets: three offset blocks, bins of 7 that straddle their borders, and one column for all"""
    g = dev()
    rng = np.random.default_rng(7)
    v = [real(2500, rng) + np.arange(2500) * 0.01, depth(600, rng)]
    anchors = random_anchors(v, 700, rng)
    want = pref.profile(v, anchors, -500, 1050, bin=bin)
    got = g.genome_profile(up(g, v), anchors, -500, 1050, bin=bin)
    check(got, want, bin)
    assert got["offsets"].tolist() == list(range(-500, 550, bin))
    if bin > 1:                                                           # the column's own mean, not each offset's
        other = pref.profile(v, anchors, -500, 1050, bin=bin, mutant="offsetmean")
        assert any(not ref.same(a[3], b[3]) for a, b in zip(want, other))


@pytest.mark.gpu
def test_what_is_refused():
    g = dev()
    v = up(g, [np.arange(100, dtype=np.float64)])
    ok = [(0, 50, 1)]
    for args in ((ok, 0, 10, 3), (ok, 0, 10, 0), (ok, 0, 0, 1), (ok, 0, 16385, 1), (ok, 2 ** 31 - 5, 10, 1),
                 ([(0, 100, 1)], 0, 10, 1), (ok + [(0, 2 ** 32 - 1, -1)], 0, 10, 1)):
        with pytest.raises(g.GdspError):
            g.genome_profile(v, *args)
    for anchors, noffsets in ((ok, 0), (ok, 16385), ([(0, 100, 1)], 10), (ok * 70 + [(0, 100, -1)], 10)):
        with pytest.raises(g.GdspError):
            g.profile_images(v, anchors, 0, noffsets)
    assert g.genome_profile(v, ok, 2 ** 31 - 10, 10)["count"].tolist() == [0] * 10     # (the last offset is INT32_MAX)
    assert g.genome_profile(v, ok, -2 ** 31, 16384, bin=16384)["count"].tolist() == [0]


@pytest.mark.gpu
def test_the_anchor_check_sees_every_anchor():
    """the device's check of profile_images (genome_profile refuses on the host before it): a bad last anchor among one
    thread's, one workgroup's, the next workgroup's, and where only the check's stride loop reaches it"""
    g = dev()
    v = up(g, [np.arange(cases.CHECK_N, dtype=np.float64)])
    most = cases.CHECK_COUNTS[-1]
    img = g.profile_images(v, cases.check_anchors(most), 0, 1)
    assert img.shape == (1, WORDS) and int(img[0, 68]) == most == 262145
    for count in cases.CHECK_COUNTS:
        with pytest.raises(g.GdspError):
            g.profile_images(v, cases.check_anchors(count, bad_last=True), 0, 1)


# -------------------------------------------------------------------------------------- identities ----

@pytest.mark.gpu
def test_identities_on_the_devices_own_outputs():
    g = dev()
    rng = np.random.default_rng(11)
    v = [real(3 * B + 7, rng), depth(500, rng), real(2 * B, rng)]
    d = up(g, v)
    anchors = random_anchors(v, 900, rng)
    lo, hi = -(B + 30), 70

    # all minus over lo .. hi is all plus over -hi .. -lo, reversed
    minus = g.genome_profile(d, [(c, p, -1) for c, p, _ in anchors], lo, hi - lo + 1)
    plus = g.genome_profile(d, [(c, p, 1) for c, p, _ in anchors], -hi, hi - lo + 1)
    for k in FIGURES:
        assert minus[k].tobytes() == plus[k][::-1].tobytes(), k

    # every vector reversed, anchors and strands mirrored
    a = g.genome_profile(d, anchors, lo, hi - lo + 1)
    mirrored = [(c, v[c].size - 1 - p, -s) for c, p, s in anchors]
    b = g.genome_profile(up(g, [x[::-1].copy() for x in v]), mirrored, lo, hi - lo + 1)
    assert same_bits(a, b)

    # anchors = every base, one offset 0: genome_stats
    every = [(c, p, 1 if p % 2 else -1) for c in range(3) for p in range(v[c].size)]
    one = g.genome_profile(d, every, 0, 1, lo=-15.0, hi=40.0)
    st = g.genome_stats(d, lo=-15.0, hi=40.0)
    for k in ("count", "sum", "mean", "variance", "stddev"):
        assert bits(one[k][0]) == bits(st[k]), k

    # a single plus anchor returns the values themselves
    single = g.genome_profile(d, [(1, 100, 1)], -100, 500)
    assert single["sum"].tobytes() == v[1].tobytes() and single["mean"].tobytes() == v[1].tobytes()
    assert (single["count"] == 1).all() and (single["variance"] == 0).all()


@pytest.mark.gpu
def test_order_split_and_hook_do_not_matter():
    """one profile: anchors shuffled; chromosomes permuted; and half the genome arriving through the allreduce hook, as
    another rank's images would"""
    g = dev()
    rng = np.random.default_rng(40)
    v = genome40(rng)
    anchors = random_anchors(v, 2000, rng)
    off_lo, noffsets, bin = -(B + 4), 2 * B + 10, 2
    want = pref.profile(v, anchors, off_lo, noffsets, bin=bin)
    d = up(g, v)
    base = g.genome_profile(d, anchors, off_lo, noffsets, bin=bin)
    check(base, want, "base")

    shuffled = [anchors[i] for i in rng.permutation(len(anchors))]
    assert same_bits(base, g.genome_profile(d, shuffled, off_lo, noffsets, bin=bin))

    perm = rng.permutation(len(v))
    where = {int(c): i for i, c in enumerate(perm)}
    assert same_bits(base, g.genome_profile([d[c] for c in perm], [(where[c], p, s) for c, p, s in anchors], off_lo, noffsets, bin=bin))

    mine, theirs = d[:17], d[17:]
    anc_mine = [a for a in anchors if a[0] < 17]
    anc_theirs = [(c - 17, p, s) for c, p, s in anchors if c >= 17]
    sizes, means = [], []

    def allreduce(arr, op):
        assert op == "sum"
        sizes.append(int(arr.size))
        if len(sizes) == 1:
            other = g.profile_images(theirs, anc_theirs, off_lo, noffsets)
            total = (arr.reshape(noffsets, WORDS) + other).reshape(noffsets // bin, bin, WORDS).sum(axis=1, dtype=np.uint64)
            cols = [g.xsum_div_round(t, int(t[68])) if t[68] else 0.0 for t in total]
            means[:] = np.repeat(np.array(cols), bin).tolist()
        else:
            other = g.profile_images(theirs, anc_theirs, off_lo, noffsets, mean=means)
        return arr + other.ravel()

    assert same_bits(base, g.genome_profile(mine, anc_mine, off_lo, noffsets, bin=bin, allreduce=allreduce))
    assert sizes == [noffsets * WORDS, noffsets * WORDS]


@pytest.mark.gpu
def test_a_hook_that_fails_is_reported():
    g = dev()
    v = up(g, [np.arange(50, dtype=np.float64)])

    def broken(arr, op):
        raise RuntimeError("the other ranks are gone")

    with pytest.raises(RuntimeError, match="the other ranks are gone"):
        g.genome_profile(v, [(0, 10, 1)], -3, 7, allreduce=broken)
    assert g.genome_profile(v, [(0, 10, 1)], -3, 7)["sum"].tolist() == [7.0, 8.0, 9.0, 10.0, 11.0, 12.0, 13.0]
