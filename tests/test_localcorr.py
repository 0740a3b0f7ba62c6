"""localcorrelate (not in the reference; gdsp_localcorr in include/genodsp_hip.h) against the checker
tests/localcorr_ref.py: inside [low, high] wherever that is bounded, and the bits of `want` wherever it is a point -- which
is everywhere on read depth and on multiples of 2^-30.  Sizes aim at the kernel's seams: the tile (gdsp_localcorr_tile),
its halos of lft and rgt bases, which come from the workspace records and not from the track itself, and the ends of the
vector, where the window is cut off and m < W.  The kernel has one form, so no window lies at a change of form."""
import ctypes

import numpy as np
import pytest

import localcorr_ref as ref

MAXW = 4097
WINDOWS = [1, 2, 3, 100, 101, 1001, 4095, MAXW]
EINVAL = 1
PLUS_ZERO = np.zeros(1).view(np.uint64)[0]


def tile_of(W):
    """outputs per workgroup of the kernel for window W, as the library reports it (host code)"""
    import genodsp_amd as gd
    return gd.localcorr_tile(W)


def gd_mod():
    import genodsp_amd as gd
    gd.set_device(0)
    return gd


def lengths_for(W, every):
    T = tile_of(W)
    lft = W - 1 - (W - 1) // 2
    few = (1, W + 1, T + 1, 2 * T - 1, 3 * T + 1, lft - 1)
    more = (W - 1, W, T - 1, T, 2 * T + 1)
    return sorted(set(n for n in few + (more if every else ()) if n >= 1))


def run(gd, dx, y, W, what):
    """the library's figure for the track y (host) against the device vector dx"""
    dy = gd.DeviceVector.from_numpy(y)
    out = gd.local_correlation(dx, dy, W, as_=what)
    assert out is dy                                                        # the track's buffer holds the result
    return out.numpy()


def check(gd, x, y, W, tag, worst=None):
    """every figure of the library on (x, y) against the checker -> (the checker's record, bases left unbounded)"""
    loc = ref.Local(x, y, W, tile_of(W))
    dx = gd.DeviceVector.from_numpy(x)
    open_ = 0
    for what in ref.KINDS:
        want, low, high = loc.figure(what)
        got = run(gd, dx, y, W, what)
        bad = np.flatnonzero(ref.verdict(got, want, low, high))
        assert bad.size == 0, (tag, what, bad[:5], got[bad[:5]], want[bad[:5]], low[bad[:5]], high[bad[:5]])
        open_ = max(open_, int(np.count_nonzero(ref.unbounded(low, high))))
        if worst is not None:
            wide = ~ref.unbounded(low, high) & (high > low)
            if wide.any():
                worst[what] = max(worst.get(what, 0.0), float(np.max(np.abs(got - want)[wide] / (high - low)[wide])))
    assert dx.numpy().tobytes() == x.tobytes(), tag                         # the signal is only read
    return loc, open_


@pytest.mark.gpu
@pytest.mark.parametrize("name", ref.GRID_SIGNALS + ref.REAL_SIGNALS)
@pytest.mark.parametrize("W", WINDOWS)
def test_matches_the_checker(W, name):
    gd = gd_mod()
    worst = {}
    bases = open_ = 0
    for n in lengths_for(W, every=name in ref.GRID_SIGNALS):
        loc, o = check(gd, ref.signal(name, n), ref.track(name, n), W, (W, n, name), worst)
        bases, open_ = bases + n, open_ + o
        if name in ref.GRID_SIGNALS:
            assert loc.exact.all()                                          # (so every figure was compared bit for bit)
    if W >= 3:                                                              # of all bases of the case, per figure at worst
        assert open_ <= 0.001 * bases, (W, name, open_, bases)
    # the record: how much of the allowance the library used at worst, (got - want) / (high - low)
    print("localcorrelate bound: W=%d %s unbounded=%d/%d %s"
          % (W, name, open_, bases, " ".join("%s=%.3g" % (k, worst[k]) for k in ref.KINDS if k in worst)))


@pytest.fixture(scope="module")
def grid_pair():
    """read depth and a second depth track, three tiles of the longest tile and a ragged end; a stretch of the signal is
    constant for longer than any window, so that windows without variance exist at every W"""
    n = 3 * 8192 + 77
    x = ref.signal("depth", n)
    x[9000:9000 + 2 * MAXW] = 3.0
    return x, ref.track("depth", n)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [2, 101, 1001, MAXW])
def test_properties_on_grid_signals(W, grid_pair):
    """bit for bit: every sum is exact, so the figures are functions of the exact sums alone"""
    gd = gd_mod()
    x, y = grid_pair
    dx, dy = gd.DeviceVector.from_numpy(x), gd.DeviceVector.from_numpy(y)
    fig = {what: run(gd, dx, y, W, what) for what in ("correlation", "covariance", "slope")}
    assert np.count_nonzero(fig["correlation"]) > 0                         # (piecewise-constant depth: few at W = 2)
    # x and y swapped: Sx Sy, Sxy and sqrt(Nxx) sqrt(Nyy) are symmetric
    for what in ("correlation", "covariance"):
        assert ref.same_bits(run(gd, dy, x, W, what), fig[what]).all(), what
    # the track negated: Sy and Sxy change sign and nothing else does, so Nxy does; a zero stays the +0.0 the definition
    # writes (Nxy == 0 whichever sign the track has)
    for what in ("correlation", "covariance", "slope"):
        neg = run(gd, dx, -y, W, what)
        zero = fig[what] == 0.0
        assert ref.same_bits(neg[~zero], -fig[what][~zero]).all(), what
        assert (neg[zero].view(np.uint64) == PLUS_ZERO).all() and (fig[what][zero].view(np.uint64) == PLUS_ZERO).all(), what
    # the track a copy of the signal: Nxy is localstats' N, the covariance its variance
    var = gd.local_stats(dx, W, as_="variance").numpy()
    assert ref.same_bits(run(gd, dx, x.copy(), W, "covariance"), var).all()
    own = run(gd, dx, x.copy(), W, "correlation")
    assert (own[var == 0.0].view(np.uint64) == PLUS_ZERO).all() and (own[var != 0.0] != 0.0).all()
    assert np.count_nonzero(var == 0.0) > 0 and np.count_nonzero(var) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("W", [3, 101, 1001, MAXW])
def test_a_constant_track_gives_plus_zero(W):
    """over a tile seam (the flat stretch reaches the main kernel half from the track, half from a record) and at the
    vector's end (where the record's slots behind the vector are zeros, not the constant)"""
    gd = gd_mod()
    T = tile_of(W)
    n = 3 * T + 4 * W
    x = ref.signal("depth", n) + 1.0
    y = ref.track("depth", n) + 1.0
    y[2 * T - W:2 * T + W + 2] = 5.0                                        # over the seam of two tiles
    y[n - 2 * W - 1:] = 2.75                                                # up to the end of the vector
    y[:W + 1] = 0.0
    lo, hi, _ = ref.window(n, W)
    flat = np.zeros(n, bool)
    for level in (5.0, 2.75, 0.0):
        Q = np.concatenate(([0], np.cumsum(y != level)))
        flat |= (Q[hi + 1] - Q[lo]) == 0
    assert flat[2 * T - 1] and flat[2 * T] and flat[n - 1] and flat[0] and np.count_nonzero(flat) >= 3
    dx = gd.DeviceVector.from_numpy(x)
    for what in ("correlation", "covariance", "slope"):
        got = run(gd, dx, y, W, what)
        assert (got[flat].view(np.uint64) == PLUS_ZERO).all(), what
    check(gd, x, y, W, (W, "crafted"))


def seam_sizes(W, count):
    T = tile_of(W)
    return [(T + 1, 1, 2 * T - 1, 17, T, 1, W, 333)[k % 8] + (k // 8) for k in range(count)]


@pytest.mark.gpu
@pytest.mark.parametrize("W", [101, MAXW])
@pytest.mark.parametrize("count", [1, 3, 33])
def test_batch_equals_the_single_vector_calls(W, count):
    """33 vectors: two tables (GDSP_BATCH_MAX is 32), and the second one's records take the place of the first one's"""
    gd = gd_mod()
    names = ref.GRID_SIGNALS + ref.REAL_SIGNALS
    xs = [ref.signal(names[k % 4], n, seed=k) for k, n in enumerate(seam_sizes(W, count))]
    ys = [ref.signal(names[k % 4], n, seed=100 + k) for k, n in enumerate(seam_sizes(W, count))]
    dxs = [gd.DeviceVector.from_numpy(h) for h in xs]
    for what in ref.KINDS:
        dys = [gd.DeviceVector.from_numpy(h) for h in ys]
        outs = gd.local_correlation_batch(dxs, dys, W, as_=what)
        assert len(outs) == count and all(o is d for o, d in zip(outs, dys))
        for hx, hy, dx, o in zip(xs, ys, dxs, outs):
            assert dx.numpy().tobytes() == hx.tobytes()                     # the signals are unchanged
            assert o.numpy().tobytes() == run(gd, dx, hy, W, what).tobytes(), (W, what, dx.n)
    want, low, high = ref.local_correlation(xs[0], ys[0], W, "correlation", tile=tile_of(W))
    dys = [gd.DeviceVector.from_numpy(h) for h in ys]
    assert not ref.verdict(gd.local_correlation_batch(dxs, dys, W)[0].numpy(), want, low, high).any()


@pytest.mark.gpu
@pytest.mark.parametrize("W", [101, MAXW])
def test_a_second_batch_gets_its_own_answer(W):
    """the same signals against two different sets of tracks, one batch after the other in one process: the records of
    the first call are rewritten by the second, and each result is the checker's, bit for bit (grid signals)"""
    gd = gd_mod()
    sizes = seam_sizes(W, 5)
    xs = [ref.signal("depth", n, seed=k) for k, n in enumerate(sizes)]
    dxs = [gd.DeviceVector.from_numpy(h) for h in xs]
    results = []
    for seed in (200, 300):
        ys = [ref.signal("dyadic" if k % 2 else "depth", n, seed=seed + k) for k, n in enumerate(sizes)]
        outs = gd.local_correlation_batch(dxs, [gd.DeviceVector.from_numpy(h) for h in ys], W, as_="covariance")
        results.append([o.numpy() for o in outs])
        for hx, hy, got in zip(xs, ys, results[-1]):
            loc = ref.Local(hx, hy, W, tile_of(W))
            assert loc.exact.all()
            assert ref.same_bits(got, loc.figure("covariance")[0]).all(), (W, seed, hx.size)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(*results))


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    gd = gd_mod()
    L = gd.lib()
    d = gd.DeviceVector.from_numpy(np.arange(100.0))
    o = gd.DeviceVector.from_numpy(np.arange(100.0)[::-1].copy())
    odd = lambda v: ctypes.c_void_p(v.ptr.value + 8)
    assert L.gdsp_localcorr(d.ptr, d.ptr, d.n, 11, 0, None) == EINVAL
    assert L.gdsp_localcorr(None, o.ptr, d.n, 11, 0, None) == EINVAL
    assert L.gdsp_localcorr(d.ptr, None, d.n, 11, 0, None) == EINVAL
    assert L.gdsp_localcorr(odd(d), o.ptr, d.n - 1, 11, 0, None) == EINVAL
    assert L.gdsp_localcorr(d.ptr, odd(o), d.n - 1, 11, 0, None) == EINVAL
    assert L.gdsp_localcorr(d.ptr, o.ptr, d.n, 0, 0, None) == EINVAL
    assert L.gdsp_localcorr(d.ptr, o.ptr, d.n, MAXW + 1, 0, None) == EINVAL
    assert L.gdsp_localcorr(d.ptr, o.ptr, d.n, 11, 4, None) == EINVAL
    assert L.gdsp_localcorr(d.ptr, o.ptr, d.n, 11, -1, None) == EINVAL
    assert L.gdsp_localcorr(d.ptr, o.ptr, 0, 11, 0, None) == 0
    assert o.numpy().tobytes() == np.arange(100.0)[::-1].tobytes()          # nothing above touched the track
    items = gd.batch_items([d], [d])
    assert L.gdsp_localcorr_batch(items, 1, 11, 0, None) == EINVAL
    items = gd.batch_items([d], [o])
    assert L.gdsp_localcorr_batch(items, 1, 0, 0, None) == EINVAL
    assert L.gdsp_localcorr_batch(items, 1, MAXW + 1, 0, None) == EINVAL
    assert L.gdsp_localcorr_batch(items, 1, 11, 4, None) == EINVAL
    assert L.gdsp_localcorr_batch(items, 0, 11, 0, None) == 0
    assert L.gdsp_localcorr(d.ptr, o.ptr, d.n, MAXW, 3, None) == 0
    with pytest.raises(ValueError):
        gd.local_correlation(d, o, 11, as_="nonsense")
    with pytest.raises(ValueError):
        gd.local_correlation_batch([d], [o], 11, as_="zscore")
    assert gd.LOCALCORR_MAX_WINDOW == MAXW


def test_the_tile_query():
    """host code: 0 outside 1..the maximum; inside, the tile plus both even-rounded reaches is what a workgroup stages
    (8192 positions of each input), and the largest window of all leaves 4096"""
    import genodsp_amd as gd
    assert gd.LOCALCORR_MAX_WINDOW == MAXW
    assert tile_of(0) == 0 and tile_of(MAXW + 1) == 0 and tile_of(2 ** 31) == 0
    assert tile_of(MAXW) == 4096 and tile_of(1) == 8192
    even = lambda w: (w + 1) & ~1
    for W in WINDOWS + [4, 4096]:
        T = tile_of(W)
        rgt = (W - 1) // 2
        assert T >= 4096 and T % 2 == 0 and T + even(W - 1 - rgt) + even(rgt) == 8192, (W, T)
