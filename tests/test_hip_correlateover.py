"""correlateover through the library (gdsp_interval_correlation[_batch] of include/genodsp_hip.h; not in the reference).
Every figure is compared bit for bit, NaN matching NaN, with the exact checker (tests/correlateover_ref.py: correlate's
checker on the interval's pair sample).  The vectors have a few tiles; the intervals sit where the cut can go wrong:
one and two bases, the frame's tile seams from both sides, the whole vector, more pieces inside one tile than one or two
items hold, duplicates, nesting, descending order."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import correlateover_ref as ref                                                                # noqa: E402

DBL_MAX = ref.DBL_MAX
TILE = 4096
N = 3 * TILE + 5
KINDS = ["depth", "real", "cancel", "binades", "nonfinite", "huge", "constant"]


def gd():
    import genodsp_amd
    return genodsp_amd


def dev():
    g = gd()
    g.set_device(0)
    return g


def data(kind, n, seed=0):
    """(x, y) of n values each"""
    rng = np.random.default_rng(1000 + seed)
    t = np.arange(n, dtype=np.float64)
    if kind == "depth":                                  # integer read depth in both: one double holds every sum
        x = rng.poisson(6, n).astype(np.float64)
        return x, np.floor(x / 2) + rng.poisson(2, n)
    if kind == "real":                                   # smooth real values
        x = 20 + 10 * np.sin(t / 37.0) + rng.standard_normal(n)
        return x, 0.3 * x + 5 * np.cos(t / 91.0) + rng.standard_normal(n) * 0.25
    if kind == "cancel":                                 # huge values that cancel: a two-term expansion cannot hold the sums
        x = rng.choice([1e16, 1.0, -1e16, 1e32, -1e32, 0.5], n)
        return x, rng.choice([1e16, 1.0, -1e16, 3.0], n)
    if kind == "binades":                                # v, -v, w, -w, ...: wherever the pairs cancel the means are 0 and the
        x, y = np.zeros(n), np.zeros(n)                  # deviations are the values, spread over hundreds of binades
        h = n // 2
        x[0:2*h:2] = rng.choice([-1.0, 1.0], h) * 2.0 ** rng.integers(-150, 150, h)
        y[0:2*h:2] = rng.choice([-1.0, 1.0], h) * 2.0 ** rng.integers(-120, 120, h)
        x[1:2*h:2], y[1:2*h:2] = -x[0:2*h:2], -y[0:2*h:2]
        return x, y
    if kind == "nonfinite":                              # NaN and +-inf in either track: left out of the sample
        x, y = data("real", n, seed + 1)
        for v, s in ((x, 1), (y, 2)):
            at = np.random.default_rng(s).integers(0, n, max(1, n // 9))
            v[at] = np.random.default_rng(s + 7).choice([math.nan, math.inf, -math.inf], at.size)
        if n > 600:
            x[300:420], y[500:560] = math.nan, math.inf
        return x, y
    if kind == "huge":                                   # products that overflow: variance +inf; covariance NaN where y is huge too
        x = rng.choice([1e200, -1e200, 3e199], n)
        y = rng.standard_normal(n)
        y[n // 2:] = rng.choice([1e200, -2e200], n - n // 2)
        return x, y
    if kind == "constant":                               # a constant track
        return data("real", n, seed)[0], np.full(n, 2.5)
    raise ValueError(kind)


def intervals(n, lead):
    """(start, end) where the cut can go wrong in a vector of n values `lead` values behind its 16-byte frame"""
    if n == 1:
        return np.array([0, 0], np.uint32), np.array([1, 1], np.uint32)
    rng = np.random.default_rng(n + lead)
    iv = [(0, 1), (0, 2), (n - 1, n), (n - 2, n), (7, 8), (0, n), (0, n), (1, n - 1)]
    for f in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1):         # frame positions at a tile seam
        p = f - lead
        iv += [(100, p), (p, p + 300), (p, p + 1), (p - 1, p + 1), (p - 2, p), (p, n)]
    base = TILE - lead + 40                                      # 129 intervals inside tile 1: three items
    iv += [(base + int(s), base + int(s) + 1 + int(w)) for s, w in zip(rng.integers(0, TILE - 200, 129), rng.integers(0, 150, 129))]
    base = 2 * TILE - lead + 3                                   # 65 inside tile 2: two items
    iv += [(base + int(s), base + int(s) + 1 + int(w)) for s, w in zip(rng.integers(0, TILE - 200, 65), rng.integers(0, 150, 65))]
    iv += [(200, 900), (200, 900), (250, 800), (300, 301), (0, TILE + 9), (50, 3 * TILE)]      # duplicates and nested overlaps
    iv.sort(key=lambda r: (-r[0], -r[1]))                        # descending
    return np.array([r[0] for r in iv], np.uint32), np.array([r[1] for r in iv], np.uint32)


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (np.isnan(a) & np.isnan(b)) | ((a == b) & (np.signbit(a) == np.signbit(b)))


def check(got, want, what=""):
    assert got["count"].dtype == np.uint32 and np.array_equal(got["count"], want["count"]), (what, "count")
    for name in ref.FIGURES[1:]:
        bad = np.flatnonzero(~same(got[name], want[name]))
        assert bad.size == 0, (what, name, int(bad[0]), float(got[name][bad[0]]), float(want[name][bad[0]]))


def views(g, x, y, lead, ylead=None):
    """the pair on the device, each `lead` values into a buffer of n + 1 (lead 1: 8-byte but not 16-byte aligned)"""
    ylead = lead if ylead is None else ylead
    n = x.size
    bx, by = np.zeros(n + 1), np.zeros(n + 1)
    bx[lead:lead + n], by[ylead:ylead + n] = x, y
    return (g.DeviceVector.from_numpy(bx), lead, n), (g.DeviceVector.from_numpy(by), ylead, n)


_WANT = {}


def expected(kind, n, lead, limits=()):
    """the checker's figures, computed once per case"""
    key = (kind, n, lead, limits)
    if key not in _WANT:
        x, y = data(kind, n)
        start, end = intervals(n, lead)
        _WANT[key] = ref.interval_correlation(x, y, start, end, *limits)
    return _WANT[key]


# ------------------------------------------------------------------------------------------------ CPU ----

def test_bad_arguments_are_refused_with_a_message():
    """refused before the device is touched"""
    g = gd()
    L = g.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake, track = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)           # never dereferenced: the arguments are refused first
    out = np.zeros(4, g.INTERVAL_CORR)

    def one(start, end, n, x=fake, y=track):
        start, end = np.array(start, np.uint32), np.array(end, np.uint32)
        return L.gdsp_interval_correlation(x, y, n, vp(start), vp(end), start.size, -DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX, vp(out), None)

    for start, end, n, text in (([5, 7], [9, 7], 100, "start < end"), ([5, 9], [9, 8], 100, "start < end"),
                                ([5, 50], [9, 101], 100, "beyond its vector"), ([0], [1], 0, "beyond its vector")):
        assert one(start, end, n) == 1 and text in L.gdsp_last_error().decode(), L.gdsp_last_error()
    assert one([5], [9], 100, y=None) == 1 and b"a track is NULL or not 8-byte aligned" in L.gdsp_last_error()
    assert one([5], [9], 100, y=ctypes.c_void_p(0x20004)) == 1 and b"a track is NULL or not 8-byte aligned" in L.gdsp_last_error()
    assert one([5], [9], 100, x=ctypes.c_void_p(0x10004)) == 1 and b"8-byte aligned" in L.gdsp_last_error()
    assert one([5], [9], 100, x=None) == 1
    with pytest.raises(g.GdspError):
        g.call("gdsp_interval_correlation", fake, None, 100, vp(np.array([5], np.uint32)), vp(np.array([9], np.uint32)), 1,
               -DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX, vp(out), None)
    item = (g.BatchItem * 1)()
    item[0].d_in, item[0].d_out, item[0].n = 0x10000, 0x20000, 100
    s, e, which = np.array([5], np.uint32), np.array([9], np.uint32), np.array([1], np.uint32)
    rc = L.gdsp_interval_correlation_batch(item, 1, vp(which), vp(s), vp(e), 1, -DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX, vp(out), None)
    assert rc == 1 and b"beyond the table" in L.gdsp_last_error()
    assert L.gdsp_interval_correlation(fake, track, 100, None, None, 1, -DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX, vp(out), None) == 1
    assert L.gdsp_interval_correlation(fake, track, 100, vp(s), vp(e), 1, -DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX, None, None) == 1
    assert L.gdsp_interval_correlation(fake, track, 100, None, None, 0, -DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX, None, None) == 0    # nothing asked
    assert g.interval_correlation_tile() == g.interval_stats_tile() == TILE
    assert g.INTERVAL_CORR.itemsize == 72
    with pytest.raises(g.GdspError):
        g.interval_correlation_set_launch_pieces(1 << 23)


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_interval_matches_the_checker(kind, lead):
    g = dev()
    x, y = data(kind, N)
    dx, dy = views(g, x, y, lead)
    start, end = intervals(N, lead)
    got = g.interval_correlation(dx, dy, start, end)
    check(got, expected(kind, N, lead), (kind, lead))
    last = g.interval_correlation_last()
    assert last["intervals"] == start.size and last["pieces"] >= start.size + 20
    if kind == "depth":
        assert last["flagged1"] == 0 and last["flagged2"] == 0               # read depth never leaves the fast route
    if kind == "cancel":
        assert last["flagged1"] > 0                                           # pass 1's second sum really ran
    if kind == "binades":
        assert last["flagged2"] > 0                                           # and pass 2's
        whole = int(np.flatnonzero((start == 0) & (end == N))[0])
        assert got["mean"][whole] == 0.0 and got["filemean"][whole] == 0.0 and got["stddev"][whole] > 2.0 ** 140
    if kind == "huge":
        whole = int(np.flatnonzero((start == 0) & (end == N))[0])
        assert got["stddev"][whole] == math.inf and math.isnan(got["covariance"][whole]) and math.isnan(got["correlation"][whole])
        first = int(np.flatnonzero((start == 200) & (end == 900))[0])        # y is small there: the crossed products are finite
        assert got["stddev"][first] == math.inf and math.isfinite(got["covariance"][first]) and math.isnan(got["slope"][first])
    if kind == "constant":
        assert np.all(got["filestddev"] == 0.0) and np.all(np.isnan(got["correlation"])) and np.all(got["filemean"] == 2.5)
    if kind == "nonfinite":
        empty = int(np.flatnonzero((start == 300) & (end == 301))[0])        # x is NaN there: an empty sample
        assert got["count"][empty] == 0 and all(math.isnan(got[k][empty]) for k in ref.FIGURES[1:])
        assert np.all(got["count"][end - start > 700] < (end - start)[end - start > 700])
    bx, by = dx[0].numpy(), dy[0].numpy()
    assert same(bx[lead:lead + N], x).all() and same(by[lead:lead + N], y).all()      # neither track is written


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset1"])
def test_a_vector_of_one_value(lead):
    g = dev()
    for kind in ("depth", "nonfinite"):
        x, y = data(kind, 1, 3)
        dx, dy = views(g, x, y, lead)
        start, end = intervals(1, lead)
        got = g.interval_correlation(dx, dy, start, end)
        check(got, ref.interval_correlation(x, y, start, end), (kind, lead))
        if kind == "depth":
            assert got["count"].tolist() == [1, 1] and got["stddev"][0] == 0.0 and math.isnan(got["slope"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("lead,ylead", [(0, 1), (1, 0)], ids=["track_offset1", "signal_offset1"])
def test_a_track_of_the_other_parity(lead, ylead):
    """the track is not congruent to the signal modulo 16 bytes: read value by value, the same figures"""
    g = dev()
    for kind in ("real", "binades"):
        x, y = data(kind, N)
        dx, dy = views(g, x, y, lead, ylead)
        start, end = intervals(N, lead)
        check(g.interval_correlation(dx, dy, start, end), expected(kind, N, lead), (kind, lead, ylead))


@pytest.mark.gpu
def test_limits_on_either_track():
    g = dev()
    for kind, limits in (("real", (12.0, 28.0, -DBL_MAX, DBL_MAX)), ("real", (-DBL_MAX, DBL_MAX, 4.0, 9.5)), ("depth", (1.0, 8.0, 2.0, 6.0)),
                         ("nonfinite", (15.0, DBL_MAX, -DBL_MAX, 8.0)), ("real", (1e9, DBL_MAX, -DBL_MAX, DBL_MAX))):
        x, y = data(kind, N)
        dx, dy = views(g, x, y, 1)
        start, end = intervals(N, 1)
        got = g.interval_correlation(dx, dy, start, end, *limits)
        want = expected(kind, N, 1, limits)
        check(got, want, (kind, limits))
        none = limits[0] == 1e9
        assert (not got["count"].any()) if none else (0 < got["count"].sum() < expected(kind, N, 1)["count"].sum())


@pytest.mark.gpu
def test_the_whole_vector_is_correlates_genome_and_rows_follow_the_intervals():
    g = dev()
    for kind in ("depth", "real", "cancel", "huge"):
        for lead in (0, 1):
            x, y = data(kind, N)
            dx, dy = views(g, x, y, lead)
            whole = g.genome_correlation([(dx, dy)])
            got = g.interval_correlation(dx, dy, [0], [N])
            assert got["count"][0] == whole["count"]
            for mine, theirs in zip(ref.FIGURES[1:], ref._FROM[1:]):
                assert same(got[mine][0], whole[theirs]), (kind, lead, mine, got[mine][0], whole[theirs])
    # permuting the intervals permutes the records; splitting the launches does not move them
    x, y = data("binades", N)
    dx, dy = views(g, x, y, 1)
    start, end = intervals(N, 1)
    got = g.interval_correlation(dx, dy, start, end)
    perm = np.random.default_rng(4).permutation(start.size)
    again = g.interval_correlation(dx, dy, start[perm], end[perm])
    g.interval_correlation_set_launch_pieces(3)
    try:
        small = g.interval_correlation(dx, dy, start, end)
        assert g.interval_correlation_last()["pieces"] > start.size
    finally:
        g.interval_correlation_set_launch_pieces(0)
    for name in ref.FIGURES:
        assert same(again[name], got[name][perm]).all() and same(small[name], got[name]).all(), name


@pytest.mark.gpu
def test_thirty_three_vectors_cross_the_launch_table():
    """more vectors than one launch table holds, one of them empty, every other pair a slice at offset 1; and the same rows
    from launches of three pieces"""
    g = dev()
    rng = np.random.default_rng(33)
    ns = [int(n) for n in rng.integers(1, 700, 33)]
    ns[0], ns[31], ns[32], ns[7] = TILE + 9, 300, 2 * TILE + 1, 0
    pairs = [data(("depth", "real", "binades")[k % 3], max(n, 1), k) for k, n in enumerate(ns)]
    xs, ys = [], []
    for k, ((x, y), n) in enumerate(zip(pairs, ns)):
        dx, dy = views(g, x[:max(n, 1)], y[:max(n, 1)], k % 2)
        xs.append((dx[0], k % 2, n))
        ys.append((dy[0], k % 2, n))
    iv = [(k, 0, ns[k]) for k in (0, 31, 32)] + [(k, ns[k] - 1, ns[k]) for k in (0, 31, 32)]
    for _ in range(300):
        k = int(rng.integers(0, 33))
        if ns[k] == 0:
            continue
        s = int(rng.integers(0, ns[k]))
        iv.append((k, s, min(ns[k], s + 1 + int(rng.integers(0, 400)))))
    order = rng.permutation(len(iv))
    which, start, end = (np.array([iv[i][c] for i in order], np.uint32) for c in range(3))
    got = g.interval_correlation(xs, ys, start, end, vec=which)
    for k in sorted(set(which.tolist())):
        sel = which == k
        want = ref.interval_correlation(pairs[k][0][:ns[k]], pairs[k][1][:ns[k]], start[sel], end[sel])
        check({name: got[name][sel] for name in ref.FIGURES}, want, k)
    g.interval_correlation_set_launch_pieces(3)
    try:
        small = g.interval_correlation(xs, ys, start, end, vec=which)
    finally:
        g.interval_correlation_set_launch_pieces(0)
    for name in ref.FIGURES:
        assert same(small[name], got[name]).all(), name
    with pytest.raises(g.GdspError):                               # an interval on the empty vector
        g.interval_correlation(xs, ys, [0], [1], vec=[7])
