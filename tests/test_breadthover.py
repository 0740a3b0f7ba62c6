"""breadthover through the library (gdsp_interval_breadth[_batch] of include/genodsp_hip.h; not in the reference).  Every
figure is a count, so every comparison is integer equality.  The checker is numpy on the CPU (tests/breadthover_ref.py:
statsover's sample and one boolean mask per threshold and interval); the data kinds are test_percentilesover's.

Run as a program it prints a digest of the mixed call below (its poison test starts it with GDSP_POISON set)."""
import ctypes
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import breadthover_ref as ref                                                                  # noqa: E402
from test_percentilesover import data                                                          # noqa: E402

DBL_MAX = ref.DBL_MAX
INF = math.inf
KINDS = ["depth", "equal", "real", "small", "sprinkled"]


def gd():
    import genodsp_amd
    return genodsp_amd


def dev():
    g = gd()
    g.set_device(0)
    return g


def same(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def thresholds(x, nt):
    """nt thresholds for the data x: values that occur in it, both zeros, both infinities, DBL_MAX, duplicates, and the
    whole list in descending order of first appearance (then whatever order the cut to nt leaves)"""
    fin = np.sort(x[np.isfinite(x)])
    own = [float(fin[fin.size // 2]), float(fin[fin.size // 4]), float(fin[-1]), float(fin[0])]
    ts = [INF, DBL_MAX, own[2], own[0], own[0], 7.0, 1.0, 0.0, -0.0, own[1], own[3], -DBL_MAX, -INF, own[0], 20.0, -INF]
    assert len(ts) == 16
    return {1: [own[0]], 2: [own[0], -INF], 15: ts[:15], 16: ts}[nt]


def check(got, v, start, end, ts, strict, lo=-DBL_MAX, hi=DBL_MAX, what=""):
    count, atleast = ref.interval_breadth(v, start, end, ts, strict, lo, hi)
    assert got["count"].dtype == np.uint32 and got["atleast"].dtype == np.uint32
    assert got["atleast"].shape == atleast.shape, what
    bad = np.flatnonzero(got["count"] != count)
    assert bad.size == 0, (what, "count", int(bad[0]), int(start[bad[0]]), int(end[bad[0]]), int(got["count"][bad[0]]), int(count[bad[0]]))
    bad = np.flatnonzero((got["atleast"] != atleast).any(axis=1))
    assert bad.size == 0, (what, int(bad[0]), int(start[bad[0]]), int(end[bad[0]]), got["atleast"][bad[0]], atleast[bad[0]])


def lengths(g):
    tile = g.interval_breadth_tile()
    return [1, 2, 63, 64, 65, 127, 128, 129, tile - 1, tile, tile + 1, 3 * tile + 1]


# ------------------------------------------------------------------------------------------------ CPU ----

def test_bad_arguments_are_refused_with_a_message():
    """refused before the device is touched"""
    L = gd().lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(0x10000)                                       # never dereferenced: the arguments are refused first
    count, atleast = np.zeros(4, np.uint32), np.zeros(4 * 17, np.uint32)
    s, e = np.array([5], np.uint32), np.array([9], np.uint32)
    ok = np.array([1.0] * 17)

    def one(start, end, n, ts, nt, v=fake, strict=0):
        return L.gdsp_interval_breadth(v, n, vp(start), vp(end), len(start), vp(ts), nt, strict, -DBL_MAX, DBL_MAX, vp(count), vp(atleast), None)

    for nt in (0, 17, -1):
        assert one(s, e, 100, ok, nt) == 1 and b"1..16" in L.gdsp_last_error()
    for strict in (0, 1):
        assert one(s, e, 100, np.array([1.0, np.nan]), 2, strict=strict) == 1 and b"NaN" in L.gdsp_last_error()
    for start, end, n, text in (([5, 7], [9, 7], 100, "start < end"), ([5, 9], [9, 8], 100, "start < end"),
                                ([5, 50], [9, 101], 100, "beyond its vector"), ([0], [1], 0, "beyond its vector")):
        rc = one(np.array(start, np.uint32), np.array(end, np.uint32), n, ok, 1)
        assert rc == 1 and text in L.gdsp_last_error().decode(), L.gdsp_last_error()
    assert one(s, e, 100, ok, 1, v=ctypes.c_void_p(0x10004)) == 1 and b"8-byte aligned" in L.gdsp_last_error()
    # a vector index beyond the table, and NULL arrays
    item = (gd().BatchItem * 1)()
    item[0].d_in, item[0].d_out, item[0].n = 0x10000, None, 100
    which = np.array([1], np.uint32)
    rc = L.gdsp_interval_breadth_batch(item, 1, vp(which), vp(s), vp(e), 1, vp(ok), 1, 0, -DBL_MAX, DBL_MAX, vp(count), vp(atleast), None)
    assert rc == 1 and b"beyond the table" in L.gdsp_last_error()
    assert L.gdsp_interval_breadth(fake, 100, None, None, 1, vp(ok), 1, 0, -DBL_MAX, DBL_MAX, vp(count), vp(atleast), None) == 1
    assert b"NULL" in L.gdsp_last_error()
    assert L.gdsp_interval_breadth(fake, 100, vp(s), vp(e), 1, None, 1, 0, -DBL_MAX, DBL_MAX, vp(count), vp(atleast), None) == 1
    assert b"NULL" in L.gdsp_last_error()
    assert L.gdsp_interval_breadth(fake, 100, vp(s), vp(e), 1, vp(ok), 1, 0, -DBL_MAX, DBL_MAX, None, None, None) == 1
    assert b"NULL" in L.gdsp_last_error()
    assert L.gdsp_interval_breadth(fake, 100, None, None, 0, vp(ok), 1, 0, -DBL_MAX, DBL_MAX, None, None, None) == 0       # nothing asked
    tile = gd().interval_breadth_tile()
    assert tile == gd().interval_stats_tile() and tile & (tile - 1) == 0


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_length_matches_the_checker(kind, lead):
    """every length at which the walk can go wrong, from an odd start, and an interval up to the vector's last base for
    both parities of n; lead 1: the vector is a slice at offset 1 of its buffer, 8-byte but not 16-byte aligned; both
    ties, 1, 2, 15 and 16 thresholds"""
    g = dev()
    Ls = lengths(g)
    for n in (Ls[-1] + 8, Ls[-1] + 9):
        x = data(kind, n + lead, seed=len(kind))
        d = g.DeviceVector.from_numpy(x)
        v = x[lead:]
        start = np.array([1] * len(Ls) + [3, n - Ls[-2], n - 1, n - 65], np.uint32)
        end = np.array([1 + L for L in Ls] + [3 + Ls[-1], n, n, n], np.uint32)
        lo, hi = (-1e299, 1e299) if kind == "sprinkled" else (-DBL_MAX, DBL_MAX)
        for nt, strict in ((16, False), (16, True), (15, False), (2, True), (1, False), (1, True)):
            ts = thresholds(v, nt)
            got = g.interval_breadth((d, lead, n) if lead else d, start, end, ts, strict, lo, hi)
            check(got, v, start, end, ts, strict, lo, hi, (kind, n, nt, strict))
            last = g.interval_breadth_last()
            assert last["intervals"] == start.size and last["launches"] == 1 and last["pieces"] >= start.size + 6
            if nt == 16:
                assert np.array_equal(got["atleast"][:, 12], got["count"]) and not got["atleast"][:, 0].any()    # -inf and +inf
                assert np.array_equal(got["atleast"][:, 3], got["atleast"][:, 4])                                  # the duplicates agree
                assert np.array_equal(got["atleast"][:, 7], got["atleast"][:, 8])                                  # and the two zeros
        if kind == "sprinkled":
            assert np.all(got["count"][8:14] < (end - start)[8:14])    # the long ones: m < e - s
        assert same(d.numpy(), x)                                  # the signal is never written


@pytest.mark.gpu
def test_an_interval_with_nothing_sampled():
    g = dev()
    tile = g.interval_breadth_tile()
    n = 3 * tile
    x = data("real", n)
    x[100:400] = np.nan
    x[5000:5000 + n // 2] = np.inf
    d = g.DeviceVector.from_numpy(x)
    start = np.array([100, 150, 5000, 0, 0], np.uint32)
    end = np.array([400, 151, 5000 + n // 2, n, n], np.uint32)
    ts = [-INF, 0.0, 2.0, INF]
    for strict in (False, True):
        got = g.interval_breadth(d, start, end, ts, strict)
        check(got, x, start, end, ts, strict)
        assert got["count"][:3].tolist() == [0, 0, 0] and not got["atleast"][:3].any() and got["atleast"][3:, :3].all()
        # and where the limits leave nothing
        got = g.interval_breadth(d, start, end, ts, strict, 1e9, DBL_MAX)
        assert not got["count"].any() and not got["atleast"].any()
    for bad in ([], [1.0] * 17, [1.0, math.nan]):
        with pytest.raises(g.GdspError):
            g.interval_breadth(d, start, end, bad)


TS_MIXED = [10.0, -INF, 0.0, 25.0, 2.0, 10.0, INF]


def mixed_call(g=None):
    """Three vectors in one call -- the second a slice at offset 1 of its buffer --, short and long intervals mixed,
    overlapping, nested and repeated, unsorted, and more than 64 pieces inside one tile, so that a tile takes more than
    one item -> (vectors, views, which, start, end, rows of the default call)"""
    g = g or dev()
    tile = g.interval_breadth_tile()
    rng = np.random.default_rng(17)
    ns = [2 * tile + 77, 3 * tile + 1, tile // 2 + 9]
    xs = [data("depth", ns[0], 4), data("sprinkled", ns[1] + 1, 5), data("real", ns[2], 6)]
    ds = [g.DeviceVector.from_numpy(x) for x in xs]
    vecs = [ds[0], (ds[1], 1, ns[1]), ds[2]]
    views = [xs[0], xs[1][1:], xs[2]]
    iv = []
    for k, n in enumerate(ns):
        iv += [(k, 0, n), (k, 0, n), (k, 1, n - 1), (k, 100, 100 + tile), (k, 100, 101 + tile), (k, 200, 300), (k, 210, 290),
               (k, 210, 290), (k, n - 1, n), (k, 0, 1), (k, n - tile // 2 - 1, n)]
        for _ in range(40):
            s = int(rng.integers(0, n - 1))
            iv.append((k, s, min(n, s + 1 + int(rng.integers(0, 1500)))))
        for _ in range(6):
            s = int(rng.integers(0, n // 2))
            iv.append((k, s, min(n, s + tile + int(rng.integers(0, n // 2)))))
    for _ in range(150):                                       # all inside tile 1 of vector 0
        s = tile + int(rng.integers(0, tile - 70))
        iv.append((0, s, s + 1 + int(rng.integers(0, 64))))
    iv = [(k, s, min(e, ns[k])) for k, s, e in iv if s < min(e, ns[k])]
    order = rng.permutation(len(iv))
    which, start, end = (np.array([iv[i][c] for i in order], np.uint32) for c in range(3))
    got = g.interval_breadth(vecs, start, end, TS_MIXED, False, -1e299, 1e299, vec=which)
    return vecs, views, which, start, end, got


def digest(got):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(got["count"]).tobytes())
    h.update(np.ascontiguousarray(got["atleast"]).tobytes())
    return h.hexdigest()


@pytest.mark.gpu
def test_mixed_call_permuted_split_and_poisoned():
    g = dev()
    vecs, views, which, start, end, got = mixed_call(g)
    last = g.interval_breadth_last()
    tiles = sum((len(v) + 1 + g.interval_breadth_tile() - 1) // g.interval_breadth_tile() for v in views)
    assert last["launches"] == 1 and last["pieces"] > start.size + 30 and last["workgroups"] > tiles >= 8     # a tile with more than one item
    for k, v in enumerate(views):
        sel = which == k
        check({"count": got["count"][sel], "atleast": got["atleast"][sel]}, v, start[sel], end[sel], TS_MIXED, False, -1e299, 1e299, k)
        one = g.interval_breadth(vecs[k], start[sel], end[sel], TS_MIXED, False, -1e299, 1e299)
        assert np.array_equal(one["count"], got["count"][sel]) and np.array_equal(one["atleast"], got["atleast"][sel]), k
    # permuted intervals give the permuted rows
    perm = np.random.default_rng(2).permutation(start.size)
    again = g.interval_breadth(vecs, start[perm], end[perm], TS_MIXED, False, -1e299, 1e299, vec=which[perm])
    assert np.array_equal(again["count"], got["count"][perm]) and np.array_equal(again["atleast"], got["atleast"][perm])
    # many small launches
    g.interval_breadth_set_launch_pieces(3)
    try:
        small = g.interval_breadth(vecs, start, end, TS_MIXED, False, -1e299, 1e299, vec=which)
        assert g.interval_breadth_last()["launches"] > start.size // 3
    finally:
        g.interval_breadth_set_launch_pieces(0)
    assert np.array_equal(small["count"], got["count"]) and np.array_equal(small["atleast"], got["atleast"])
    # every device allocation poisoned (the library's workspace among them), in a fresh process
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GDSP_POISON="nan"),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip().splitlines()[-1] == digest(got)


@pytest.mark.gpu
def test_seventy_vectors_in_one_call():
    """more than two launch tables of 32 vectors: lengths 0 to 300, some empty, intervals on the first and the last
    vector of every table"""
    g = dev()
    rng = np.random.default_rng(70)
    ns = [int(n) for n in rng.integers(1, 301, 70)]
    for k in (5, 33, 40, 68):
        ns[k] = 0
    xs = [data("depth" if k % 2 else "sprinkled", max(n, 1) + 1, 100 + k) for k, n in enumerate(ns)]
    ds = [g.DeviceVector.from_numpy(x) for x in xs]
    vecs = [(d, k % 2, n) for k, (d, n) in enumerate(zip(ds, ns))]           # every other one a slice at offset 1
    views = [x[k % 2:k % 2 + n] for k, (x, n) in enumerate(zip(xs, ns))]
    iv = [(k, 0, ns[k]) for k in (0, 31, 32, 63, 64, 69)] + [(k, ns[k] - 1, ns[k]) for k in (0, 31, 32, 63, 64, 69)]
    for _ in range(400):
        k = int(rng.integers(0, 70))
        if ns[k] == 0:
            continue
        s = int(rng.integers(0, ns[k]))
        iv.append((k, s, min(ns[k], s + 1 + int(rng.integers(0, 200)))))
    order = rng.permutation(len(iv))
    which, start, end = (np.array([iv[i][c] for i in order], np.uint32) for c in range(3))
    ts = [1.0, 10.0, 20.0, -INF, 0.0]
    for strict in (False, True):
        got = g.interval_breadth(vecs, start, end, ts, strict, -1e299, 1e299, vec=which)
        assert g.interval_breadth_last()["launches"] == 3
        for k in sorted(set(which.tolist())):
            sel = which == k
            check({"count": got["count"][sel], "atleast": got["atleast"][sel]}, views[k], start[sel], end[sel], ts, strict, -1e299, 1e299, k)
    with pytest.raises(g.GdspError):
        g.interval_breadth(vecs, [0], [1], ts, vec=[70])
    with pytest.raises(g.GdspError):
        g.interval_breadth(vecs, [0], [1], ts, vec=[5])                        # an empty vector has no interval


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["depth", "small", "sprinkled"])
def test_cross_checks_against_interval_stats(kind):
    """count is interval_stats' count, column -inf is the count and column +inf is 0, and the columns do not increase
    with the threshold"""
    g = dev()
    tile = g.interval_breadth_tile()
    n = 3 * tile + 50
    x = data(kind, n, seed=8)
    d = g.DeviceVector.from_numpy(x)
    rng = np.random.default_rng(9)
    start = rng.integers(0, n - 1, 300).astype(np.uint32)
    end = np.minimum(n, start + 1 + rng.integers(0, 2 * tile, 300)).astype(np.uint32)
    fin = x[np.isfinite(x)]
    ts = sorted(set([-INF, INF, 0.0, DBL_MAX, -DBL_MAX] + [float(t) for t in np.quantile(fin, [0.1, 0.3, 0.5, 0.7, 0.9])]))
    for strict in (False, True):
        got = g.interval_breadth(d, start, end, ts, strict, -1e299, 1e299)
        st = g.interval_stats(d, start, end, -1e299, 1e299)
        assert np.array_equal(got["count"].astype(np.uint64), st["count"])
        assert np.array_equal(got["atleast"][:, 0], got["count"]) and not got["atleast"][:, -1].any()
        assert np.all(np.diff(got["atleast"].astype(np.int64), axis=1) <= 0)
        check(got, x, start, end, ts, strict, -1e299, 1e299, kind)
    assert same(d.numpy(), x)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["depth", "real"])
def test_the_whole_vector_is_the_histograms_atleast(kind):
    """one interval covering the vector against genome_histogram at the same edges: n - below - the cumulative counts"""
    g = dev()
    n = 300001
    x = data(kind, n, seed=12)
    d = g.DeviceVector.from_numpy(x)
    edges = np.array([0.0, 1.0, 5.0, 10.0, 20.0, 39.0, 1000.0]) if kind == "depth" else np.linspace(-30.0, 40.0, 15)
    counts, below, above, total = g.genome_histogram([d], edges)
    assert total == n
    cum = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    want = n - int(below) - cum                                  # values >= edges[j] (bin j is [edge j, edge j+1)); the last: `above`
    assert int(want[-1]) == int(above)
    got = g.interval_breadth(d, [0], [n], edges)
    assert int(got["count"][0]) == n
    assert np.array_equal(got["atleast"][0].astype(np.int64), want), (got["atleast"][0], want)
    check(got, x, [0], [n], edges, False, what=kind)
    assert same(d.numpy(), x)


if __name__ == "__main__":
    print(digest(mixed_call()[5]))
