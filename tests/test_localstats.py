"""localstats (not in the reference; gdsp_localstats in include/genodsp_hip.h) against the checker tests/localstats_ref.py:
inside [low, high] wherever that is bounded, and the bits of `want` wherever it is a point -- which is everywhere on read
depth and on multiples of 2^-30.  Sizes aim at the kernel's seams: the tile (gdsp_localstats_tile), its halos of lft and
rgt bases, the change from the 512-thread form to the 1024-thread form between W = 4097 and 4098, and the ends of the
vector, where the window is cut off and m < W."""
import numpy as np
import pytest

import localstats_ref as ref

MAXW = 12287
WINDOWS = [1, 2, 3, 100, 101, 1001, 4095, 4099, 10001, MAXW]              # (4095, 4099: either side of the change of form)
EINVAL = 1


def tile_of(W):
    """outputs per workgroup of the kernel for window W, as the library reports it (host code)"""
    import genodsp_amd as gd
    return gd.lib().gdsp_localstats_tile(W)


def gd_mod():
    import genodsp_amd as gd
    gd.set_device(0)
    return gd


def lengths_for(W, every):
    T = tile_of(W)
    lft = W - 1 - (W - 1) // 2
    few = (1, W + 1, T + 1, 2 * T - 1, 3 * T + 1, lft - 1)
    more = (W - 1, W, T - 1, T, 2 * T + 1, 3 * T - 1)
    return sorted(set(n for n in few + (more if every else ()) if n >= 1))


def levels(loc):
    """a floor and a smallest stddev that are equal to the figure of one base, above some and below others"""
    mid = loc.n // 2
    return float(loc.figure("mean")[0][mid]), float(loc.figure("stddev")[0][mid])


def check(gd, v, W, tag, worst=None):
    """every figure of the library on v against the checker, plain and with a floor and a smallest stddev"""
    loc = ref.Local(v, W, tile_of(W))
    d = gd.DeviceVector.from_numpy(v)
    floor, minsd = levels(loc)
    for what in ref.KINDS:
        for fl, ms in ((None, None), (floor, minsd)):
            if fl is not None and what == "variance":
                continue                                                    # (neither level touches it)
            want, low, high = loc.figure(what, fl, ms)
            got = gd.local_stats(d, W, as_=what, floor=fl, minsd=ms).numpy()
            bad = np.flatnonzero(ref.verdict(got, want, low, high))
            assert bad.size == 0, (tag, what, fl, ms, bad[:5], got[bad[:5]], want[bad[:5]], low[bad[:5]], high[bad[:5]])
            if worst is not None:
                wide = ~ref.unbounded(low, high) & (high > low)
                if wide.any():
                    worst[what] = max(worst.get(what, 0.0), float(np.max(np.abs(got - want)[wide] / (high - low)[wide])))
    assert d.numpy().tobytes() == v.tobytes(), tag                          # out of place
    return loc


@pytest.mark.gpu
@pytest.mark.parametrize("name", ref.GRID_SIGNALS + ref.REAL_SIGNALS)
@pytest.mark.parametrize("W", WINDOWS)
def test_matches_the_checker(W, name):
    gd = gd_mod()
    worst = {}
    for n in lengths_for(W, every=name in ref.GRID_SIGNALS):
        loc = check(gd, ref.signal(name, n), W, (W, n, name), worst)
        if name in ref.GRID_SIGNALS:
            assert loc.exact.all()                                          # (so every figure was compared bit for bit)
    # the record: how much of the allowance the library used at worst, (got - want) / (high - low)
    print("localstats bound: W=%d %s %s" % (W, name, " ".join("%s=%.3g" % (k, worst[k]) for k in ref.KINDS if k in worst)))


@pytest.mark.gpu
@pytest.mark.parametrize("W", [3, 101, 1001, 10001])
def test_zero_and_constant_windows_give_plus_zero(W):
    gd = gd_mod()
    T = tile_of(W)
    n = 2 * T + 3 * W
    v = ref.signal("depth", n) + 1.0
    v[T - W:T + W + 2] = 0.0                                                # over the seam of two tiles
    v[n - 2 * W - 1:] = 2.75                                                # up to the end of the vector
    v[:W + 1] = 0.0
    d = gd.DeviceVector.from_numpy(v)
    lo, hi, _ = ref.window(n, W)
    P = np.concatenate(([0], np.cumsum(v != 0.0)))
    zeros = (P[hi + 1] - P[lo]) == 0
    Q = np.concatenate(([0], np.cumsum(v != 2.75)))
    flat = (Q[hi + 1] - Q[lo]) == 0
    assert np.count_nonzero(zeros) >= 4 and np.count_nonzero(flat) >= W
    plus_zero = np.zeros(1).view(np.uint64)[0]
    ratio = gd.local_stats(d, W, as_="ratio").numpy()
    assert (ratio[zeros].view(np.uint64) == plus_zero).all()
    z = gd.local_stats(d, W).numpy()
    assert (z[zeros | flat].view(np.uint64) == plus_zero).all()
    assert (gd.local_stats(d, W, as_="stddev").numpy()[zeros | flat].view(np.uint64) == plus_zero).all()
    check(gd, v, W, (W, "crafted"))


@pytest.mark.gpu
@pytest.mark.parametrize("W", [101, 10001])
@pytest.mark.parametrize("count", [1, 3, 33])
def test_batch_equals_the_single_vector_calls(W, count):
    gd = gd_mod()
    T = tile_of(W)
    sizes = [(T + 1, 1, 2 * T - 1, 17, T, 1, W, 333)[k % 8] + (k // 8) for k in range(count)]
    names = ref.GRID_SIGNALS + ref.REAL_SIGNALS
    hosts = [ref.signal(names[k % 4], n, seed=k) for k, n in enumerate(sizes)]
    vecs = [gd.DeviceVector.from_numpy(h) for h in hosts]
    floor, minsd = float(np.mean(hosts[0])), float(np.std(hosts[0])) / 2
    for what in ref.KINDS:
        for fl, ms in ((None, None), (floor, minsd)):
            outs = gd.local_stats_batch(vecs, W, as_=what, floor=fl, minsd=ms)
            assert len(outs) == count
            for h, v, o in zip(hosts, vecs, outs):
                assert o.ptr != v.ptr and v.numpy().tobytes() == h.tobytes()                 # the inputs are unchanged
                assert o.numpy().tobytes() == gd.local_stats(v, W, as_=what, floor=fl, minsd=ms).numpy().tobytes(), (W, what, v.n)
    want, low, high = ref.local_stats(hosts[0], W, "zscore", tile=T)
    assert not ref.verdict(gd.local_stats_batch(vecs, W)[0].numpy(), want, low, high).any()


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    gd = gd_mod()
    L = gd.lib()
    d = gd.DeviceVector.from_numpy(np.arange(100.0))
    o = d.like()
    assert L.gdsp_localstats(d.ptr, d.ptr, d.n, 11, 0, 0, 0.0, 0, 0.0, None) == EINVAL
    assert L.gdsp_localstats(d.ptr, o.ptr, d.n, 0, 0, 0, 0.0, 0, 0.0, None) == EINVAL
    assert L.gdsp_localstats(d.ptr, o.ptr, d.n, MAXW + 1, 0, 0, 0.0, 0, 0.0, None) == EINVAL
    assert L.gdsp_localstats(d.ptr, o.ptr, d.n, 11, 6, 0, 0.0, 0, 0.0, None) == EINVAL
    assert L.gdsp_localstats(d.ptr, o.ptr, d.n, 11, -1, 0, 0.0, 0, 0.0, None) == EINVAL
    assert L.gdsp_localstats(d.ptr, o.ptr, 0, 11, 0, 0, 0.0, 0, 0.0, None) == 0
    items = gd.batch_items([d], [d])
    assert L.gdsp_localstats_batch(items, 1, 11, 0, 0, 0.0, 0, 0.0, None) == EINVAL
    items = gd.batch_items([d], [o])
    assert L.gdsp_localstats_batch(items, 1, 0, 0, 0, 0.0, 0, 0.0, None) == EINVAL
    assert L.gdsp_localstats_batch(items, 1, MAXW + 1, 0, 0, 0.0, 0, 0.0, None) == EINVAL
    assert L.gdsp_localstats_batch(items, 1, 11, 6, 0, 0.0, 0, 0.0, None) == EINVAL
    assert L.gdsp_localstats(d.ptr, o.ptr, d.n, MAXW, 5, 0, 0.0, 0, 0.0, None) == 0
    with pytest.raises(ValueError):
        gd.local_stats(d, 11, as_="nonsense")
    assert gd.LOCALSTATS_MAX_WINDOW == MAXW


def test_the_tile_query():
    """host code: 0 outside 1..the maximum; inside, a tile and both reaches fit what one workgroup stages (8192 values
    while that leaves 4096 outputs, else 16384), and the largest window of all leaves 4096"""
    assert tile_of(0) == 0 and tile_of(MAXW + 1) == 0 and tile_of(2 ** 31) == 0
    assert MAXW >= 10001 and tile_of(MAXW) == 4096
    for W in WINDOWS + [4096, 4097, 4098]:
        T = tile_of(W)
        staged = 8192 if W <= 4097 else 16384
        assert T >= 4096 and T % 2 == 0 and staged - 2 <= T + W - 1 <= staged, (W, T)
