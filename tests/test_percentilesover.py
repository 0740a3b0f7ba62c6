"""percentilesover through the library (gdsp_interval_percentiles[_batch] of include/genodsp_hip.h; not in the reference).
A value is an input value chosen by integer comparisons, so every comparison is bit for bit.  The checker is numpy on
the CPU (tests/percentilesover_ref.py: statsover's sample, percentile's keys and rank rule, np.sort per interval).

Run as a program it prints a digest of the mixed call below (its poison test starts it with GDSP_POISON set)."""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import percentilesover_ref as ref                                                              # noqa: E402
import sliding_percentile_ref as sref                                                          # noqa: E402

DBL_MAX = ref.DBL_MAX
PS = [0, 1, 50000, 99999, 100000]
PS16 = [50000, 0, 100000, 25000, 50000, 75000, 99999, 1, 0, 33333, 66667, 100000, 10, 90000, 50000, 12345]


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


def check(got, v, start, end, ps, lo=-DBL_MAX, hi=DBL_MAX, what=""):
    count, values = ref.interval_percentiles(v, start, end, ps, lo, hi)
    assert got["values"].shape == values.shape, what
    bad = np.flatnonzero(got["count"] != count)
    assert bad.size == 0, (what, "count", int(bad[0]), int(start[bad[0]]), int(end[bad[0]]))
    bad = np.flatnonzero((got["values"].view(np.uint64) != values.view(np.uint64)).any(axis=1))
    assert bad.size == 0, (what, int(bad[0]), int(start[bad[0]]), int(end[bad[0]]), got["values"][bad[0]], values[bad[0]])


def lengths(g):
    short, piece = g.interval_percentiles_short(), g.interval_percentiles_piece()
    return sorted(set([1, 2, 63, 64, 65, 511, 512, 513, short - 1, short, short + 1, piece - 1, piece, piece + 1, 3 * piece + 1]))


def data(kind, n, seed=1):
    rng = np.random.default_rng(seed)
    if kind == "depth":                                         # integer depth, heavy ties
        return np.repeat(rng.integers(0, 40, n // 50 + 1), 50)[:n].astype(np.float64)
    if kind == "equal":
        return np.full(n, 7.0)
    if kind == "last_digit":                                    # 1.0 + j 2^-52: the keys differ in their last digit only
        return 1.0 + rng.permutation(n) % 512 * 2.0 ** -52
    if kind == "top_digit":                                     # powers of two of either sign: sign and exponent only
        return np.ldexp(np.where(rng.random(n) < 0.5, -1.0, 1.0), rng.integers(-40, 40, n) * 16)
    if kind == "real":
        return rng.standard_normal(n) * 10.0 + 2.0
    if kind == "small":                                         # negatives, denormals, zeros of both signs
        x = rng.integers(-2 ** 40, 2 ** 40, n).astype(np.float64) * 5e-324
        x[rng.random(n) < 0.3] = -0.0
        x[rng.random(n) < 0.3] = 0.0
        neg = rng.random(n) < 0.2
        x[neg] = -np.abs(rng.standard_normal(int(neg.sum())))
        return x
    assert kind == "sprinkled"                                  # NaN, infinities and values beyond the limits among reals
    x = rng.standard_normal(n) * 10.0
    pick = rng.random(n) < 0.15
    x[pick] = rng.choice(np.array([np.nan, -np.nan, np.inf, -np.inf, 1e300, -1e300, -0.0]), int(pick.sum()))
    return x


KINDS = ["depth", "equal", "last_digit", "top_digit", "real", "small", "sprinkled"]


# ------------------------------------------------------------------------------------------------ CPU ----

def test_bad_arguments_are_refused_with_a_message():
    """refused before the device is touched"""
    L = gd().lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(0x10000)                                       # never dereferenced: the arguments are refused first
    count, values = np.zeros(4, np.uint32), np.zeros(4 * 17)
    s, e = np.array([5], np.uint32), np.array([9], np.uint32)
    ok = np.array([50000] * 17, np.uint32)

    def one(start, end, n, ps, np_):
        return L.gdsp_interval_percentiles(fake, n, vp(start), vp(end), len(start), vp(ps), np_, -DBL_MAX, DBL_MAX, vp(count), vp(values), None)

    for np_ in (0, 17, -1):
        assert one(s, e, 100, ok, np_) == 1 and b"1..16" in L.gdsp_last_error()
    assert one(s, e, 100, np.array([50000, 100001], np.uint32), 2) == 1 and b"100000" in L.gdsp_last_error()
    for start, end, n, text in (([5, 7], [9, 7], 100, "start < end"), ([5, 9], [9, 8], 100, "start < end"),
                                ([5, 50], [9, 101], 100, "beyond its vector"), ([0], [1], 0, "beyond its vector")):
        rc = one(np.array(start, np.uint32), np.array(end, np.uint32), n, ok, 1)
        assert rc == 1 and text in L.gdsp_last_error().decode(), L.gdsp_last_error()
    assert L.gdsp_interval_percentiles(ctypes.c_void_p(0x10004), 100, vp(s), vp(e), 1, vp(ok), 1, -DBL_MAX, DBL_MAX, vp(count), vp(values), None) == 1
    assert L.gdsp_interval_percentiles(fake, 100, None, None, 0, vp(ok), 1, -DBL_MAX, DBL_MAX, None, None, None) == 0      # nothing asked
    short, piece = gd().interval_percentiles_short(), gd().interval_percentiles_piece()
    assert short <= 8192 and short & (short - 1) == 0 and piece >= short


def test_every_interval_fault_of_the_batch_call_names_the_call_and_the_fault():
    """one fault per call; each is refused before the device is touched"""
    g = gd()
    L = g.lib()
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    count, values = np.zeros(2, np.uint32), np.zeros(2)
    ok = np.array([50000], np.uint32)
    u32 = lambda *a: np.array(a, np.uint32)

    def table(*ptr_n):
        items = (g.BatchItem * max(1, len(ptr_n)))()
        for k, (ptr, n) in enumerate(ptr_n):
            items[k].d_in, items[k].n = ptr, n
        return items

    two = table((0x10000, 100), (0x20000, 50))                           # never dereferenced: the arguments are refused first
    for items, m, vec, start, end, text in (
            (two, 2, u32(0, 1), None, u32(9, 9), "NULL interval arrays"),
            (two, 2, u32(0, 1), u32(5, 5), None, "NULL interval arrays"),
            (None, 2, u32(0, 1), u32(5, 5), u32(9, 9), "no vectors"),
            (two, 0, u32(0, 1), u32(5, 5), u32(9, 9), "no vectors"),
            (table((0x10000, 100), (0x20004, 50)), 2, u32(0, 1), u32(5, 5), u32(9, 9), "a vector must be 8-byte aligned"),
            (two, 2, u32(0, 2), u32(5, 5), u32(9, 9), "an interval names a vector beyond the table"),
            (two, 2, u32(0, 1), u32(5, 9), u32(9, 9), "an interval must have start < end"),
            (two, 2, u32(0, 1), u32(5, 5), u32(9, 51), "an interval ends beyond its vector")):
        rc = L.gdsp_interval_percentiles_batch(items, m, vp(vec), vp(start), vp(end), 2, vp(ok), 1, -DBL_MAX, DBL_MAX, vp(count), vp(values), None)
        assert rc == 1 and L.gdsp_last_error().decode() == "gdsp_interval_percentiles_batch: " + text, (text, L.gdsp_last_error())


# ------------------------------------------------------------------------------------------------ GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_length_matches_the_checker(kind, lead):
    """every length at which the route or the sort changes, from an odd start; lead 1: the vector is a slice at offset 1
    of its buffer, 8-byte but not 16-byte aligned"""
    g = dev()
    Ls = lengths(g)
    n = Ls[-1] + 8
    x = data(kind, n + lead, seed=len(kind))
    d = g.DeviceVector.from_numpy(x)
    v = x[lead:]
    start = np.array([1] * len(Ls) + [3, n - Ls[-2]], np.uint32)
    end = np.array([1 + L for L in Ls] + [3 + Ls[-1], n], np.uint32)
    lo, hi = (-1e299, 1e299) if kind == "sprinkled" else (-DBL_MAX, DBL_MAX)
    got = g.interval_percentiles((d, lead, n) if lead else d, start, end, PS, lo, hi)
    last = g.interval_percentiles_last()
    check(got, v, start, end, PS, lo, hi, kind)
    short = g.interval_percentiles_short()
    nlong = int(((end - start) > short).sum())
    assert (last["intervals"], last["short"], last["long"]) == (start.size, start.size - nlong, nlong) and nlong >= 5
    if kind == "equal":                                        # one value: every long query ends after its first pass
        assert last["ended_early"] == nlong * len(PS) and last["passes"] == 1
        assert np.all(got["values"] == 7.0)
    if kind == "last_digit":                                   # the median is not settled before the last digit
        assert last["ended_early"] < nlong * len(PS) and last["passes"] > 1
        g.interval_percentiles(d if not lead else (d, lead, n), start, end, [50000])
        assert g.interval_percentiles_last()["ended_early"] == 0
    if kind == "sprinkled":
        assert np.all(got["count"][2:] < (end - start)[2:])   # m < e - s
    if kind == "small":
        zero = got["values"] == 0.0
        assert zero.any() and not np.signbit(got["values"][zero]).any()
    assert same(d.numpy(), x)                                  # the signal is never written


@pytest.mark.gpu
def test_an_interval_with_nothing_sampled():
    g = dev()
    n = 3 * g.interval_percentiles_piece()
    x = data("real", n)
    x[100:400] = np.nan
    x[5000:5000 + n // 2] = np.inf
    d = g.DeviceVector.from_numpy(x)
    start = np.array([100, 150, 5000, 0, 0], np.uint32)
    end = np.array([400, 151, 5000 + n // 2, n, n], np.uint32)
    got = g.interval_percentiles(d, start, end, PS)
    check(got, x, start, end, PS)
    assert got["count"][:3].tolist() == [0, 0, 0] and np.isnan(got["values"][:3]).all() and not np.isnan(got["values"][3:]).any()
    # and where the limits leave nothing
    got = g.interval_percentiles(d, start, end, PS, 1e9, DBL_MAX)
    assert not got["count"].any() and np.isnan(got["values"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["depth", "real", "sprinkled"])
def test_sixteen_percentiles_with_duplicates_out_of_order(kind):
    g = dev()
    Ls = lengths(g)
    n = Ls[-1] + 8
    x = data(kind, n, seed=3)
    d = g.DeviceVector.from_numpy(x)
    start = np.array([5] * len(Ls), np.uint32)
    end = np.array([5 + L for L in Ls], np.uint32)
    got = g.interval_percentiles(d, start, end, PS16)
    check(got, x, start, end, PS16, what=kind)
    for a, b in ((0, 4), (0, 14), (1, 8), (2, 11)):           # the duplicates agree
        assert same(got["values"][:, a], got["values"][:, b])
    for bad in ([], PS16 + [5], [100001]):
        with pytest.raises(g.GdspError):
            g.interval_percentiles(d, start, end, bad)


def mixed_call(g=None):
    """Three vectors in one call -- the second a slice at offset 1 of its buffer --, short and long intervals mixed,
    overlapping, nested and repeated, unsorted -> (vectors, views, which, start, end, rows of the default call)"""
    g = g or dev()
    short, piece = g.interval_percentiles_short(), g.interval_percentiles_piece()
    rng = np.random.default_rng(17)
    ns = [2 * piece + 77, 3 * piece + 1, short + 9]
    xs = [data("depth", ns[0], 4), data("sprinkled", ns[1] + 1, 5), data("real", ns[2], 6)]
    ds = [g.DeviceVector.from_numpy(x) for x in xs]
    vecs = [ds[0], (ds[1], 1, ns[1]), ds[2]]
    views = [xs[0], xs[1][1:], xs[2]]
    iv = []
    for k, n in enumerate(ns):
        iv += [(k, 0, n), (k, 0, n), (k, 1, n - 1), (k, 100, 100 + short), (k, 100, 101 + short), (k, 200, 300), (k, 210, 290),
               (k, 210, 290), (k, n - 1, n), (k, 0, 1), (k, n - short - 1, n)]
        for _ in range(40):
            s = int(rng.integers(0, n - 1))
            iv.append((k, s, min(n, s + 1 + int(rng.integers(0, 1500)))))
        for _ in range(6):
            s = int(rng.integers(0, n // 2))
            iv.append((k, s, min(n, s + short + int(rng.integers(0, n // 2)))))
    iv = [(k, s, min(e, ns[k])) for k, s, e in iv if s < min(e, ns[k])]
    order = rng.permutation(len(iv))
    which, start, end = (np.array([iv[i][c] for i in order], np.uint32) for c in range(3))
    got = g.interval_percentiles(vecs, start, end, PS, -1e299, 1e299, vec=which)
    return vecs, views, which, start, end, got


def digest(got):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(got["count"]).tobytes())
    h.update(np.ascontiguousarray(got["values"]).tobytes())
    return h.hexdigest()


@pytest.mark.gpu
def test_mixed_call_permuted_batched_and_poisoned():
    g = dev()
    vecs, views, which, start, end, got = mixed_call(g)
    last = g.interval_percentiles_last()
    assert last["short"] > 100 and last["long"] > 15 and last["batches"] == 1
    for k, v in enumerate(views):
        sel = which == k
        check({"count": got["count"][sel], "values": got["values"][sel]}, v, start[sel], end[sel], PS, -1e299, 1e299, k)
        one = g.interval_percentiles(vecs[k], start[sel], end[sel], PS, -1e299, 1e299)
        assert np.array_equal(one["count"], got["count"][sel]) and same(one["values"], got["values"][sel]), k
    # permuted intervals give the permuted rows
    perm = np.random.default_rng(2).permutation(start.size)
    again = g.interval_percentiles(vecs, start[perm], end[perm], PS, -1e299, 1e299, vec=which[perm])
    assert np.array_equal(again["count"], got["count"][perm]) and same(again["values"], got["values"][perm])
    # many small batches of the long route
    g.interval_percentiles_set_batch(3)
    try:
        small = g.interval_percentiles(vecs, start, end, PS, -1e299, 1e299, vec=which)
        assert g.interval_percentiles_last()["batches"] == last["long"]       # five queries an interval: one interval a batch
    finally:
        g.interval_percentiles_set_batch(0)
    assert np.array_equal(small["count"], got["count"]) and same(small["values"], got["values"])
    # every device allocation poisoned (the library's workspace among them), in a fresh process
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GDSP_POISON="nan"),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip().splitlines()[-1] == digest(got)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["depth", "small", "sprinkled"])
def test_extremes_and_count_are_interval_stats(kind):
    g = dev()
    n = 3 * g.interval_percentiles_piece() + 50
    x = data(kind, n, seed=8)
    d = g.DeviceVector.from_numpy(x)
    rng = np.random.default_rng(9)
    start = rng.integers(0, n - 1, 300).astype(np.uint32)
    end = np.minimum(n, start + 1 + rng.integers(0, 2 * g.interval_percentiles_short(), 300)).astype(np.uint32)
    got = g.interval_percentiles(d, start, end, [0, 100000], -1e299, 1e299)
    st = g.interval_stats(d, start, end, -1e299, 1e299)
    assert np.array_equal(got["count"].astype(np.uint64), st["count"])
    assert same(got["values"][:, 0], st["min"]) and same(got["values"][:, 1], st["max"])


@pytest.mark.gpu
@pytest.mark.parametrize("W", [101, 4095])
def test_a_window_is_sliding_percentile_at_its_base(W):
    g = dev()
    n = 3 * W + 1000
    x = data("real", n, seed=W)
    x[::3] = np.round(x[::3])                                   # ties
    d = g.DeviceVector.from_numpy(x)
    wl, wr = sref.reach(W)
    at = np.unique(np.concatenate([np.arange(0, 40), np.arange(n - 40, n), [wl - 1, wl, wl + 1, n - wr - 2, n - wr - 1, n - wr],
                                   np.random.default_rng(1).integers(0, n, 150)]))
    start = np.maximum(0, at - wl).astype(np.uint32)
    end = (np.minimum(n - 1, at + wr) + 1).astype(np.uint32)
    for p in (50000, 10000, 99999):
        got = g.interval_percentiles(d, start, end, [p])
        assert same(got["values"][:, 0], g.sliding_percentile(d, W, p).numpy()[at]), (W, p)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["depth", "real", "small"])
def test_the_whole_vector_is_percentile(kind):
    g = dev()
    n = 300001
    x = data(kind, n, seed=12)
    d = g.DeviceVector.from_numpy(x)
    got = g.interval_percentiles(d, [0], [n], PS16)
    count, want = g.percentile([d], PS16)
    assert int(got["count"][0]) == count == n
    assert same(got["values"][0], want)
    check(got, x, [0], [n], PS16, what=kind)


if __name__ == "__main__":
    print(digest(mixed_call()[5]))
