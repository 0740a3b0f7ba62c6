"""localmad / hampel (not in the reference): each base against the median and the MAD of slidingpercentile's window around
it (gdsp_localmad, include/genodsp_hip.h).  Every figure is defined operation by operation, so everything here compares
bytes: the library against the numpy checker tests/localmad_ref.py for every figure, over the vector lengths that cross
every seam of the kernel's tile, on data made to reach every case of its search.  (The one exception a number format
forces: inf / inf, the z-score of a deviation that overflowed, is a NaN whose sign IEEE 754 leaves open -- NaNs are
compared as NaNs.)"""
import os

import numpy as np
import pytest

import localmad_ref as ref
import sliding_percentile_ref as sp
from conftest import ROOT

MAXW = 4095
WINDOWS = [1, 2, 3, 4, 11, 100, 101, 1000, 1001, 4094, 4095]
DBL_MAX = float(np.finfo(np.float64).max)


def tile_of(W):
    """outputs per workgroup of the kernel for window W, as the library reports it (host code, no GPU needed)"""
    import genodsp_amd as gd
    return gd.localmad_tile(W)


def same(a, b):
    a, b = np.array(a, np.float64), np.array(b, np.float64)
    a[np.isnan(a)] = np.nan
    b[np.isnan(b)] = np.nan
    return a.tobytes() == b.tobytes()


def where(a, b):
    a, b = np.array(a, np.float64), np.array(b, np.float64)
    return np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b)))[:5]


# ------------------------------------------------------------------------------------------------- CPU ----

def test_the_tile_is_slidingpercentiles():
    import genodsp_amd as gd
    for W in WINDOWS:
        assert tile_of(W) == gd.lib().gdsp_sliding_percentile_tile(W) and tile_of(W) >= max(1, W - 1), W
    assert tile_of(0) == 0 and tile_of(MAXW + 1) == 0
    assert gd.LOCALMAD_MAX_WINDOW == MAXW and list(gd.LOCALMAD_WHAT) == list(ref.WHAT)
    text = open(os.path.join(ROOT, "include", "genodsp_hip.h")).read()
    for k, name in enumerate(ref.WHAT):
        assert "#define GDSP_LOCALMAD_%-10s %d" % (name.upper(), k) in text and gd.LOCALMAD_WHAT[name] == k
    assert "#define GDSP_LOCALMAD_MAX_WINDOW %d" % MAXW in text


# ------------------------------------------------------------------------------------------------- GPU ----

def gd_mod():
    import genodsp_amd as gd
    gd.set_device(0)
    return gd


def lengths_for(W):
    t = tile_of(W)
    return sorted(set(x for x in (1, 2, W - 1, W, W + 1, t - 1, t, t + 1, 2 * t + 3) if x >= 1))


def data(kind, n, rng):
    if kind == "real":
        return rng.standard_normal(n) * 10.0
    if kind == "depth":
        return rng.integers(0, 8, n).astype(np.float64)
    if kind == "tower":
        v = rng.poisson(5.0, n).astype(np.float64)
        if n >= 30:
            v[n // 2 - 5:n // 2 + 5] += 100.0
        return v
    raise ValueError(kind)


def check_every_figure(gd, v, W, tag, **kw):
    want = ref.figures(v, W, **kw)
    d = gd.DeviceVector.from_numpy(v)
    out = d.like()
    for what in ref.WHAT:
        got = gd.local_mad(d, W, as_=what, out=out, **kw).numpy()
        assert same(got, want[what]), (tag, W, v.size, what, kw, where(got, want[what]))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("W", WINDOWS)
def test_matches_the_checker_bit_for_bit(W):
    gd = gd_mod()
    lengths = lengths_for(W)
    for q, n in enumerate(lengths):                                      # (every kind on the longest, one kind in turn on the others)
        for j, kind in enumerate(("real", "depth", "tower")):
            if n == lengths[-1] or j == q % 3:
                check_every_figure(gd, data(kind, n, np.random.default_rng([W, n, j])), W, kind)
    v = data("real", lengths_for(W)[-1], np.random.default_rng(W))
    d = gd.DeviceVector.from_numpy(v)
    assert gd.hampel(d, W).numpy().tobytes() == ref.hampel(v, W).tobytes()             # (hampel: as_="clean")
    assert gd.local_mad(d, W).numpy().tobytes() == ref.local_mad(v, W).tobytes()       # (local_mad: as_="zscore")


@pytest.mark.gpu
@pytest.mark.parametrize("W", [100, 101, 1000, 1001, 4094, 4095])
def test_a_tower_is_an_outlier_and_nothing_else_changes(W):
    """Poisson depth with ten bases raised by 100 across a tile seam.  With a least MAD of 2 the limit is
    8 x 1.4826 x max(MAD, 2) >= 23.7, which Poisson(5) never strays from its median by, and the tower always does"""
    gd = gd_mod()
    t = tile_of(W)
    n = 2 * t + 3
    v = np.random.default_rng(W).poisson(5.0, n).astype(np.float64)
    assert v.max() < 23
    v[t - 5:t + 5] += 100.0
    want = check_every_figure(gd, v, W, "tower", threshold=8.0, minmad=2.0)
    assert np.flatnonzero(want["outlier"]).tolist() == list(range(t - 5, t + 5))
    got = gd.hampel(gd.DeviceVector.from_numpy(v), W, threshold=8.0, minmad=2.0).numpy()
    changed = np.flatnonzero(got.view(np.uint64) != v.view(np.uint64))
    assert changed.tolist() == list(range(t - 5, t + 5)) and np.all(got[t - 5:t + 5] < 23)


def inexact(x, y):
    """fl(x - y) is not x - y (both integers held exactly)"""
    return int(x - y) != int(x) - int(y)


def crafted():
    """(name, vector, W, what the checker itself must show for the vector to be the case it is meant to be)"""
    rng = np.random.default_rng(11)
    cases = []
    cases.append(("all equal", np.full(2100, 3.25), [1, 4, 7, 101], lambda v, W, med, mad: not mad.any()))
    cases.append(("two values", (rng.random(2100) < 0.4) * 2.5, [2, 3, 7, 100],
                  lambda v, W, med, mad: set(np.unique(mad)) <= {0.0, 2.5} and len(np.unique(mad)) == 2))
    cases.append(("strictly increasing", np.arange(2100.0), [3, 5, 7, 101],             # left and right deviations tie: at the MAD's rank,
                  lambda v, W, med, mad: all(d[k] in (d[k - 1], d[k + 1]) for i in (1000, 1001)   # and for even k as L(a) == R(a)
                                             for w in [ref.window_of(v, W, i)] for k in [w.size // 2]
                                             for d in [np.sort(np.abs(w - med[i]))])
                  and (W != 5 or ref.block(ref.window_of(v, W, 1000)) == (1, 1.0))))
    low = np.tile(np.array([1.0, 1.0, 1.0, 1.0, 50.0, 60.0, 70.0]), 300)               # W = 7: base 3 sees 1 1 1 1 50 60 70 (block at a = 0),
    cases.append(("block at a = 0", low, [7], lambda v, W, med, mad: ref.block(ref.window_of(v, W, 3 + 7 * 150))[0] == 0))
    high = np.tile(np.array([-70.0, -60.0, -50.0, 1.0, 1.0, 1.0, 1.0]), 300)           # and -70 -60 -50 1 1 1 1 (block at a = k = 3)
    cases.append(("block at a = min(k, m-1-k)", high, [7], lambda v, W, med, mad: ref.block(ref.window_of(v, W, 3 + 7 * 150))[0] == 3))
    ends = rng.integers(0, 9, 2100).astype(np.float64)                                  # W = 4: 3 and 4 bases at the left end, 2 and 3 at the right;
    cases.append(("truncated windows", ends, [4, 5, 6, 100],                            # W = 5: 3 4 5 and 5 4 3
                  lambda v, W, med, mad: {ref.window_of(v, W, i).size % 2 for i in (0, 1)} == {0, 1}
                  and {ref.window_of(v, W, v.size - 1 - i).size % 2 for i in (0, 1)} == {0, 1}))
    big = rng.choice(np.array([1e16, 1e16 + 2, 1.0, 2.0, 3.0, 5.0]), 2100)              # 1e16 - 3 and 1e16 - 1 are no doubles
    cases.append(("1e16 beside small integers", big, [3, 4, 11, 101],
                  lambda v, W, med, mad: any(inexact(x, m) for i in range(200) for m in [med[i]] for x in ref.window_of(v, W, i))))
    huge = rng.choice(np.array([DBL_MAX, -DBL_MAX, 1.0]), 2100, p=[0.45, 0.45, 0.1])                        # (a MAD of +inf needs an even window split in two halves)
    cases.append(("DBL_MAX beside -DBL_MAX", huge, [3, 4, 11, 100, 101],
                  lambda v, W, med, mad: any(np.isinf(np.abs(ref.window_of(v, W, i) - med[i])).any() for i in range(200))
                  and np.isfinite(mad).any() and (W != 4 or np.isinf(mad).any())))
    zeros = np.where(np.arange(2100) % 3 == 0, 0.0, -0.0)
    cases.append(("signed zeros", zeros, [1, 3, 4], lambda v, W, med, mad: not np.signbit(med).any()))
    return cases


CRAFTED = crafted()


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(CRAFTED)), ids=[c[0].replace(" ", "_") for c in CRAFTED])
def test_crafted_vectors(which):
    gd = gd_mod()
    name, v, windows, reaches = CRAFTED[which]
    for W in windows:
        med, mad = ref.med_mad(v, W)
        with np.errstate(over="ignore"):
            assert reaches(v, W, med, mad), (name, W)                    # (the checker's own figures, not the library's)
        check_every_figure(gd, v, W, name)
        check_every_figure(gd, v, W, name, scale=0.75, threshold=1.0, minmad=0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("W", WINDOWS)
def test_the_median_is_slidingpercentiles(W):
    gd = gd_mod()
    for n in lengths_for(W)[-3:]:
        v = data("depth", n, np.random.default_rng([W, n])) - 3.0
        v[::17] = -0.0
        d = gd.DeviceVector.from_numpy(v)
        assert gd.local_mad(d, W, as_="median").numpy().tobytes() == gd.sliding_percentile(d, W, 50000).numpy().tobytes(), (W, n)


@pytest.mark.gpu
def test_batch_equals_the_single_vector_calls():
    """one launch over vectors of unequal lengths, an empty one among them, and more than one table of 32"""
    gd = gd_mod()
    rng = np.random.default_rng(5)
    lengths = [0, 1, 5000, 23457, 0, 8192, 77, 4098] + [int(x) for x in rng.integers(1, 9000, 30)]
    vecs = [gd.DeviceVector.from_numpy(rng.poisson(4.0, n).astype(np.float64) + (rng.random(n) < 0.1) * 0.5) for n in lengths]
    for W, what, kw in ((101, "zscore", {}), (1001, "clean", dict(threshold=2.0)), (4095, "mad", dict(minmad=1.0)), (2, "outlier", {})):
        outs = gd.local_mad_batch(vecs, W, as_=what, **kw)
        for v, o in zip(vecs, outs):
            if v.n == 0:
                continue
            assert o.numpy().tobytes() == gd.local_mad(v, W, as_=what, **kw).numpy().tobytes(), (W, what, v.n)
    v = vecs[2].numpy()
    assert gd.local_mad_batch(vecs, 101)[2].numpy().tobytes() == ref.local_mad(v, 101).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("W", [4, 101, 1000])
def test_a_nan_or_an_infinity_spoils_only_the_windows_that_hold_it(W):
    gd = gd_mod()
    t = tile_of(W)
    n = 2 * t + 3
    left, right = sp.reach(W)
    clean = np.random.default_rng(W).standard_normal(n) * 4.0
    want = ref.figures(clean, W)
    spots = {t - 1: np.nan, t + W + 7: np.inf, n - 1: -np.inf, 0: np.nan}
    v = clean.copy()
    for p, x in spots.items():
        v[p] = x
    touched = np.zeros(n, bool)
    for p in spots:                                                      # base i sees p where i - left <= p <= i + right
        touched[max(0, p - right):min(n, p + left + 1)] = True
    assert (~touched).sum() > 10
    d = gd.DeviceVector.from_numpy(v)
    for what in ref.WHAT:
        got = gd.local_mad(d, W, as_=what).numpy()
        assert got[~touched].tobytes() == want[what][~touched].tobytes(), (W, what)


@pytest.mark.gpu
def test_bad_arguments_are_refused_and_leave_the_output_alone():
    gd = gd_mod()
    L = gd.lib()
    d = gd.DeviceVector.from_numpy(np.arange(100.0))
    mark = np.full(100, -77.5)
    o = gd.DeviceVector.from_numpy(mark)
    nan, inf = float("nan"), float("inf")
    ok = (11, 0, 1.4826, 3.0, 0, 0.0)
    bad = [(MAXW + 1,) + ok[1:], (0,) + ok[1:], (11, 6) + ok[2:], (11, -1) + ok[2:],
           (11, 0, 0.0) + ok[3:], (11, 0, -1.0) + ok[3:], (11, 0, inf) + ok[3:], (11, 0, nan) + ok[3:],
           (11, 0, 1.4826, -1.0, 0, 0.0), (11, 0, 1.4826, nan, 0, 0.0), (11, 0, 1.4826, 3.0, 1, -0.5), (11, 0, 1.4826, 3.0, 1, nan)]
    items = gd.batch_items([d], [o])
    for args in bad:
        assert L.gdsp_localmad(d.ptr, o.ptr, d.n, *args, None) == 1, args
        assert L.gdsp_localmad_batch(items, 1, *args, None) == 1, args
    assert L.gdsp_localmad(d.ptr, d.ptr, d.n, *ok, None) == 1                       # out of place only
    assert L.gdsp_localmad_batch(gd.batch_items([d], [d]), 1, *ok, None) == 1
    assert L.gdsp_localmad(d.ptr, o.ptr, 0, *ok, None) == 0                          # n == 0: nothing to do
    gd.sync()
    assert o.numpy().tobytes() == mark.tobytes()
    assert L.gdsp_localmad(d.ptr, o.ptr, d.n, 11, 0, 1.4826, 3.0, 1, -0.5, None) == 1
    assert L.gdsp_localmad(d.ptr, o.ptr, d.n, 11, 0, 1.4826, 3.0, 0, -0.5, None) == 0   # (a least MAD that is not given is not looked at)
    assert L.gdsp_localmad(d.ptr, o.ptr, d.n, MAXW, 5, 1.4826, 0.0, 1, 0.0, None) == 0
    with pytest.raises(ValueError):
        gd.local_mad(d, 11, as_="mean")


@pytest.mark.gpu
def test_each_parameter_at_a_value_that_decides_and_one_that_cannot():
    gd = gd_mod()
    n, W = 3 * tile_of(101) + 5, 101
    v = np.random.default_rng(3).poisson(6.0, n).astype(np.float64)
    v[::211] += 40.0
    d = gd.DeviceVector.from_numpy(v)

    def got(what, **kw):
        g = gd.local_mad(d, W, as_=what, **kw).numpy()
        assert same(g, ref.figures(v, W, **kw)[what]), (what, kw)
        return g.tobytes()

    mads = ref.local_mad(v, W, "mad")
    assert 0 < mads.min() and mads.max() < 50
    # minmad: below every MAD it decides nothing; above every MAD it is the MAD everywhere
    for what in ref.WHAT:
        assert got(what, minmad=mads.min() / 2) == got(what)
    assert got("mad", minmad=50.0) == np.full(n, 50.0).tobytes() and got("zscore", minmad=50.0) != got("zscore")
    assert got("outlier", minmad=50.0) != got("outlier")
    # threshold: above every z-score nothing is an outlier and clean is the input; a low one marks more than the default
    zmax = np.abs(ref.local_mad(v, W)).max()
    assert got("outlier", threshold=zmax * 1.5) == np.zeros(n).tobytes() and got("clean", threshold=zmax * 1.5) == v.tobytes()
    assert got("outlier", threshold=1.0) != got("outlier") != np.zeros(n).tobytes()
    assert got("zscore", threshold=1.0) == got("zscore")                       # (the threshold is not in the z-score)
    # scale: in the z-score and the limit; not in median, mad and difference, and with a threshold of 0 not in the marks
    assert got("zscore", scale=1.0) != got("zscore") and got("outlier", scale=3.0) != got("outlier")
    for what in ("median", "mad", "difference"):
        assert got(what, scale=3.0) == got(what)
    assert got("outlier", scale=3.0, threshold=0.0) == got("outlier", threshold=0.0)
