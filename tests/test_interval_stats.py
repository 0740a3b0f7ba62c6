"""statsover through the library (gdsp_interval_stats, gdsp_interval_stats_batch, gdsp_interval_stats_combine of
include/genodsp_hip.h; not in the reference).  Every figure is a function of the interval's sample alone, exact and
rounded once, so every comparison is bit for bit.  The checker is numpy on the CPU: tests/xsum_ref.py's exact sum of the
finite, in-range values of v[s:e] for count, sum and mean; numpy's min / max with + 0.0; the first index of the sample
equal to the maximum.  On integer read depth np.add.reduceat in float64 is exact and checks a whole chromosome.

Run as a program it prints a digest of the flagged-pieces call below (its poison test starts it with GDSP_POISON set)."""
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

import xsum_ref as ref                                                                         # noqa: E402

DBL_MAX = ref.DBL_MAX
TINY = 5e-324
WORDS = 72


def gd():
    import genodsp_amd
    return genodsp_amd


def expect(v, s, e, lo=-DBL_MAX, hi=DBL_MAX):
    """(count, sum, mean, min, max, maxpos) of interval [s, e) of v, by the definition"""
    x = v[s:e]
    keep = ~(x < lo) & ~(x > hi) & np.isfinite(x)
    smp = x[keep]
    n = int(smp.size)
    M = ref.exact_int(smp)
    total = ref.round_ratio(M, 1 << ref.SCALE)
    if n == 0:
        return (0, total, math.nan, math.nan, math.nan, -1)
    mx = smp.max()
    return (n, total, ref.round_ratio(M, n << ref.SCALE), float(smp.min() + 0.0), float(mx + 0.0),
            s + int(np.flatnonzero(keep & (x == mx))[0]))


def check(got, v, start, end, lo=-DBL_MAX, hi=DBL_MAX, what=""):
    assert len(got["count"]) == len(start)
    for i, (s, e) in enumerate(zip(start, end)):
        w = expect(v, int(s), int(e), lo, hi)
        assert int(got["count"][i]) == w[0], (what, i, s, e, got["count"][i], w[0])
        for k, name in ((1, "sum"), (2, "mean"), (3, "min"), (4, "max")):
            assert ref.same(got[name][i], w[k]), (what, name, i, s, e, got[name][i], w[k])
        assert int(got["maxpos"][i]) == w[5], (what, i, s, e, got["maxpos"][i], w[5])


# ------------------------------------------------------------------------------------------------ CPU ----

def piece(a0, a1=0.0, mn=None, mx=None, count=1, maxpos=0, flag=0):
    r = np.zeros(1, gd().INTERVAL_PIECE)
    r["a0"], r["a1"], r["count"], r["maxpos"], r["flag"] = a0, a1, count, maxpos, flag
    r["min"] = a0 if mn is None else mn
    r["max"] = a0 if mx is None else mx
    return r


def test_combine_one_piece_of_integers():
    got = gd().interval_stats_combine(piece(12.0, 0.0, 1.0, 5.0, count=5, maxpos=7))
    assert (int(got["count"]), got["sum"], got["mean"], got["min"], got["max"], int(got["maxpos"])) == (5, 12.0, 2.4, 1.0, 5.0, 7)
    assert ref.same(got["mean"], 12.0 / 5) and got["image"] == 0           # two doubles were enough


def test_combine_terms_that_cancel():
    vals = [1e308, 1e308, -1e308, -1e308, 1.0]
    got = gd().interval_stats_combine(np.concatenate([piece(x, maxpos=10 + i) for i, x in enumerate(vals)]))
    want = ref.stats(np.array(vals))
    assert int(got["count"]) == 5 and ref.same(got["sum"], want[1]) and ref.same(got["mean"], want[2])
    assert got["sum"] == 1.0 and got["mean"] == 0.2
    assert got["min"] == -1e308 and got["max"] == 1e308 and int(got["maxpos"]) == 10     # the lowest position of the maximum
    # the same through two-term pieces, in another order
    got2 = gd().interval_stats_combine(np.concatenate([piece(1.0, maxpos=14), piece(-1e308, -1e308 * 2.0 ** -54, maxpos=12),
                                                       piece(1e308, 1e308 * 2.0 ** -54, maxpos=11)]))
    assert got2["sum"] == 1.0


def test_combine_a_sum_that_rounds_to_infinity():
    for sign in (1.0, -1.0):
        got = gd().interval_stats_combine(np.concatenate([piece(sign * DBL_MAX), piece(sign * DBL_MAX, maxpos=1)]))
        assert got["sum"] == sign * math.inf and got["mean"] == sign * DBL_MAX and int(got["count"]) == 2
    # DBL_MAX + half an ulp of it rounds to infinity, a hair less does not
    got = gd().interval_stats_combine(np.concatenate([piece(DBL_MAX), piece(2.0 ** 970, maxpos=1)]))
    assert got["sum"] == math.inf
    got = gd().interval_stats_combine(np.concatenate([piece(DBL_MAX), piece(2.0 ** 970, -1.0, maxpos=1)]))
    assert got["sum"] == DBL_MAX


def test_combine_a_mean_of_subnormals():
    for vals in ([TINY] * 3, [TINY, TINY, 3 * TINY, -TINY], [TINY], [TINY, 0.0], [-TINY, 0.0, 0.0], [7 * TINY] * 2 + [0.0]):
        ps = np.concatenate([piece(x, maxpos=i) for i, x in enumerate(vals)])
        got, want = gd().interval_stats_combine(ps), ref.stats(np.array(vals))
        assert ref.same(got["sum"], want[1]) and ref.same(got["mean"], want[2]), (vals, got, want)
    # one piece, count 3, sum one subnormal: 1/3 of the smallest double rounds to zero
    got = gd().interval_stats_combine(piece(TINY, 0.0, 0.0, TINY, count=3))
    assert ref.same(got["mean"], 0.0) and got["sum"] == TINY


def test_combine_the_mean_of_a_two_term_sum():
    """s + e with s = fl(s + e): the sum is s, and the mean is (s + e) / n rounded once -- not s / n"""
    rng = np.random.default_rng(4)
    imaged = 0
    cases = [(1.0, 2.0 ** -53, 3), (1.0, -2.0 ** -54, 3), (3.0, 2.0 ** -52, 3), (2.0 ** -1021, 2.0 ** -1074, 7), (-5.5, 2.0 ** -60, 1),
             (1e308, 2.0 ** 960, 2 ** 32), (1.0, TINY, 3), (2.0 ** 53 + 2, 1.0, 2), (2.0 ** 53 + 2, -1.0, 2), (6.0, 2.0 ** -51, 4)]
    for _ in range(3000):
        s = float(np.ldexp(rng.standard_normal(), int(rng.integers(-1000, 1000))))
        ulp = math.ulp(s)
        bits = int(rng.integers(1, 54))
        e = float(np.ldexp(float(rng.integers(1, 2 ** bits)), -bits - int(rng.integers(1, 12)))) * ulp * (1 if rng.random() < 0.5 else -1)
        cases.append((s, e, int(rng.integers(1, 2 ** int(rng.integers(1, 33))))))
    for s, e, n in cases:
        if e == 0.0 or s + e != s:
            continue
        got = gd().interval_stats_combine(np.concatenate([piece(s, e, s, s, count=n - n // 2), piece(0.0, count=n // 2)]))
        M = ref.exact_int(np.array([s, e]))
        assert ref.same(got["sum"], s), (s, e)
        assert ref.same(got["mean"], ref.round_ratio(M, n << ref.SCALE)), (s, e, n, got["mean"])
        imaged += got["image"]
    assert imaged < len(cases) // 20                                 # the 128-bit division took nearly all of them


def test_combine_nothing_sampled():
    for ps in (piece(0.0, 0.0, math.inf, -math.inf, count=0, maxpos=0xFFFFFFFF),
               np.concatenate([piece(0.0, 0.0, math.inf, -math.inf, count=0, maxpos=0xFFFFFFFF)] * 3)):
        got = gd().interval_stats_combine(ps)
        assert int(got["count"]) == 0 and ref.same(got["sum"], 0.0) and int(got["maxpos"]) == -1
        assert math.isnan(got["mean"]) and math.isnan(got["min"]) and math.isnan(got["max"])


def test_combine_zeros_and_flagged_pieces():
    got = gd().interval_stats_combine(np.concatenate([piece(-0.0, maxpos=4), piece(0.0, maxpos=2)]))
    assert ref.same(got["min"], 0.0) and ref.same(got["max"], 0.0) and ref.same(got["sum"], 0.0) and int(got["maxpos"]) == 2
    # a flagged piece brings its image; its terms are not looked at
    img = np.zeros(WORDS, np.uint64)
    for x in (1e308, 3.5, -1e308, 2.0 ** -1070):
        gd().xsum_add_host(img, x)
    ps = np.concatenate([piece(2.0, maxpos=1), piece(math.nan, math.nan, -1e308, 1e308, count=4, maxpos=9, flag=1)])
    got = gd().interval_stats_combine(ps, img)
    want = ref.stats(np.array([2.0, 1e308, 3.5, -1e308, 2.0 ** -1070]))
    assert int(got["count"]) == 5 and ref.same(got["sum"], want[1]) and ref.same(got["mean"], want[2]) and got["image"] == 1
    with pytest.raises(gd().GdspError):
        gd().interval_stats_combine(ps, None)


def test_bad_arguments_are_refused_with_a_message():
    """refused before the device is touched"""
    L = gd().lib()
    rec = np.zeros(4, gd().INTERVAL_STAT)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    fake = ctypes.c_void_p(0x10000)                                       # never dereferenced: the arguments are refused first
    for start, end, n, text in (([5, 7], [9, 7], 100, "start < end"), ([5, 9], [9, 8], 100, "start < end"),
                                ([5, 50], [9, 101], 100, "beyond its vector"), ([0], [1], 0, "beyond its vector")):
        s, e = np.array(start, np.uint32), np.array(end, np.uint32)
        rc = L.gdsp_interval_stats(fake, n, vp(s), vp(e), len(start), -DBL_MAX, DBL_MAX, vp(rec), None)
        assert rc == 1 and text in L.gdsp_last_error().decode(), L.gdsp_last_error()
    s = np.array([1], np.uint32)
    for args in ((fake, 100, None, vp(s), 1), (fake, 100, vp(s), None, 1)):
        assert L.gdsp_interval_stats(*args, -DBL_MAX, DBL_MAX, vp(rec), None) == 1 and b"NULL" in L.gdsp_last_error()
    assert L.gdsp_interval_stats(fake, 100, vp(s), vp(s + 1), 1, -DBL_MAX, DBL_MAX, None, None) == 1
    assert L.gdsp_interval_stats(ctypes.c_void_p(0x10004), 100, vp(s), vp(s + 1), 1, -DBL_MAX, DBL_MAX, vp(rec), None) == 1
    assert L.gdsp_interval_stats(fake, 100, None, None, 0, -DBL_MAX, DBL_MAX, None, None) == 0      # nothing asked


# ------------------------------------------------------------------------------------------------ GPU ----

N = 70001
NAN_AT, FLAT_AT, ZERO_AT = (20000, 20100), (30000, 30200), (40000, 40010)


def dev():
    g = gd()
    g.set_device(0)
    return g


def data(kind, n=N, seed=11):
    rng = np.random.default_rng(seed)
    if kind == "depth":
        x = rng.integers(0, 60, n).astype(np.float64)
    elif kind == "real":
        x = rng.standard_normal(n) * 10.0 + 2.0
    else:                                                      # adversarial
        x = np.ldexp(rng.standard_normal(n), rng.integers(-300, 300, n))          # mixed signs across 600 binades
        x[1000:4000:3], x[1001:4000:3], x[1002:4000:3] = 1e308, 1.0, -1e308       # huge cancelling pairs
        x[5000:5400:2], x[5001:5400:2] = DBL_MAX, -DBL_MAX
        x[6000:6300] = DBL_MAX                                                    # a sum beyond DBL_MAX
        sub = x[8000:9000]
        sub[:] = rng.integers(-2 ** 52, 2 ** 52, sub.size).astype(np.float64) * TINY
        pick = rng.random(n) < 0.01
        x[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0]), int(pick.sum()))
    if n >= ZERO_AT[1]:
        x[NAN_AT[0]:NAN_AT[1]] = np.nan
        x[FLAT_AT[0]:FLAT_AT[1]] = 7.0
        x[ZERO_AT[0]:ZERO_AT[1]] = -0.0
    return x


def interval_set(n, T, seed=5):
    rng = np.random.default_rng(seed)
    iv = [(0, 1), (n - 1, n), (0, n), (0, n), (5, n), (n - T - 3, n), (NAN_AT[0] + 10, NAN_AT[1] - 10), FLAT_AT,
          (FLAT_AT[0] + 1, FLAT_AT[1]), ZERO_AT, (1000, 9000), (2000, 8000), (3000, 7000), (3000, 7000), (6000, 6300)]
    for b in range(T, n, T):                                   # on and one base either side of every tile boundary
        iv += [(b - 1, b), (b, b + 1), (b - 1, b + 1), (b - T, b), (b - T + 1, b - 1), (b - T - 1, b + 1),
               (b + 1, min(n, b + T + 1)), (b - 2, b - 1), (b + 1, b + 2)]
    for _ in range(150):                                       # heavily overlapping
        s = 10000 + int(rng.integers(0, 50))
        iv.append((s, s + 4000 + int(rng.integers(0, 3000))))
    for _ in range(500):
        s = int(rng.integers(0, n - 1))
        iv.append((s, min(n, s + 1 + int(rng.integers(0, 2000)))))
    for _ in range(25):
        s = int(rng.integers(0, n // 2))
        iv.append((s, s + 1 + int(rng.integers(n // 4, n // 2))))
    iv = [(max(0, s), e) for s, e in iv if max(0, s) < e <= n]
    order = rng.permutation(len(iv))                           # unsorted
    return np.array([iv[i][0] for i in order], np.uint32), np.array([iv[i][1] for i in order], np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["depth", "real", "adversarial"])
def test_matches_the_checker(kind):
    g = dev()
    x = data(kind)
    d = g.DeviceVector.from_numpy(x)
    start, end = interval_set(N, g.interval_stats_tile())
    got = g.interval_stats(d, start, end)
    last = g.interval_stats_last()
    check(got, x, start, end, what=kind)
    assert last["intervals"] == start.size and last["pieces"] >= start.size
    # the slow path is taken where it must be, and only there
    if kind == "adversarial":
        assert last["flagged"] > 0
    if kind == "depth":
        assert last["flagged"] == 0 and last["imaged"] == 0
    i = int(np.flatnonzero((start == FLAT_AT[0]) & (end == FLAT_AT[1]))[0])
    assert int(got["maxpos"][i]) == FLAT_AT[0] and got["max"][i] == 7.0 and got["min"][i] == 7.0
    i = int(np.flatnonzero((start == NAN_AT[0] + 10) & (end == NAN_AT[1] - 10))[0])
    assert int(got["count"][i]) == 0 and int(got["maxpos"][i]) == -1 and math.isnan(got["mean"][i]) and ref.same(got["sum"][i], 0.0)
    assert np.array_equal(d.numpy().view(np.uint64), x.view(np.uint64))            # the signal is not modified
    # the order of the intervals does not change a record
    perm = np.random.default_rng(1).permutation(start.size)
    again = g.interval_stats(d, start[perm], end[perm])
    for name in got:
        assert np.array_equal(again[name].view(np.uint64), got[name][perm].view(np.uint64)), name


@pytest.mark.gpu
@pytest.mark.parametrize("kind,lo,hi", [("depth", 10.0, 40.0), ("real", -3.5, 1e301), ("adversarial", -1e300, 1e300),
                                        ("depth", 1e9, DBL_MAX)])
def test_limits(kind, lo, hi):
    g = dev()
    x = data(kind)
    start, end = interval_set(N, g.interval_stats_tile(), seed=8)
    start, end = start[:400], end[:400]
    got = g.interval_stats(g.DeviceVector.from_numpy(x), start, end, lo=lo, hi=hi)
    check(got, x, start, end, lo, hi, (kind, lo, hi))
    if lo == 1e9:
        assert not got["count"].any() and (got["maxpos"] == -1).all()


@pytest.mark.gpu
def test_batch_equals_the_single_vector_calls():
    g = dev()
    rng = np.random.default_rng(3)
    T = g.interval_stats_tile()
    lengths = [T + 1, 12345, 1, 33333, 2 * T, 7]
    xs = [data("real" if k % 2 else "adversarial", n + 1, seed=k)[:n + 1] for k, n in enumerate(lengths)]
    ds = [g.DeviceVector.from_numpy(x) for x in xs]
    # vector 3 is read from its second value on: 8-byte but not 16-byte aligned
    vecs = [ds[0], ds[1], ds[2], (ds[3], 1, lengths[3]), ds[4], ds[5]]
    views = [xs[0], xs[1], xs[2], xs[3][1:], xs[4], xs[5]]
    ns = [v.size for v in views]
    which, start, end = [], [], []
    for k, n in enumerate(ns):
        cuts = [(0, n), (0, 1), (n - 1, n)] + [(b - 1, min(n, b + 1)) for b in range(T - 1, n, T)] + [(b, min(n, b + 2)) for b in range(T, n, T)]
        for _ in range(120):
            s = int(rng.integers(0, n))
            cuts.append((s, min(n, s + 1 + int(rng.integers(0, 3000)))))
        for s, e in cuts:
            which.append(k), start.append(s), end.append(e)
    order = rng.permutation(len(which))
    which, start, end = (np.array(a, np.uint32)[order] for a in (which, start, end))
    got = g.interval_stats(vecs, start, end, vec=which)
    for k in range(len(vecs)):
        sel = which == k
        one = g.interval_stats(vecs[k], start[sel], end[sel])
        for name in got:
            assert np.array_equal(one[name].view(np.uint64), got[name][sel].view(np.uint64)), (k, name)
        check(one, views[k], start[sel], end[sel], what=k)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["depth", "real", "adversarial"])
def test_one_interval_over_the_vector_is_genome_stats(kind):
    g = dev()
    x = data(kind, 300001)
    d = g.DeviceVector.from_numpy(x)
    got = g.interval_stats(d, [0], [x.size])
    st = g.genome_stats([d])
    assert float(got["count"][0]) == st["count"]
    assert ref.same(got["sum"][0], st["sum"]) and ref.same(got["mean"][0], st["mean"])
    check(got, x, [0], [x.size], what=kind)


@pytest.mark.gpu
def test_a_whole_chromosome_of_read_depth():
    """chr1, 248,956,422 bases: 1 kb bins tiling it and a few dozen intervals of 1-200 Mbp, against numpy's exact integer
    sums on the read-back vector"""
    g = dev()
    n = 248956422
    d = g.synth_coverage(20240611, 0, 0, n, 0)
    x = d.numpy()
    rng = np.random.default_rng(2)
    bins = np.arange(0, n, 1000, dtype=np.int64)
    start = list(bins)
    end = list(np.minimum(bins + 1000, n))
    nb = len(start)
    for _ in range(40):
        s = int(rng.integers(0, n - 1000000))
        start.append(s)
        end.append(min(n, s + int(rng.integers(1000000, 200000000))))
    start.append(0)
    end.append(n)
    start, end = np.array(start, np.uint32), np.array(end, np.uint32)
    got = g.interval_stats(d, start, end)
    last = g.interval_stats_last()
    assert last["flagged"] == 0 and last["imaged"] == 0 and last["intervals"] == start.size
    assert np.isfinite(x).all() and float(x.max()) * n < 2.0 ** 53            # float64 sums of it are exact
    sums = np.add.reduceat(x, bins)
    assert np.array_equal(got["sum"][:nb], sums)
    assert np.array_equal(got["count"][:nb], (end[:nb] - start[:nb]).astype(np.uint64))
    assert np.array_equal(got["mean"][:nb], sums / (end[:nb] - start[:nb]))
    assert np.array_equal(got["max"][:nb], np.maximum.reduceat(x, bins))
    assert np.array_equal(got["min"][:nb], np.minimum.reduceat(x, bins))
    full = x[:(nb - 1) * 1000].reshape(nb - 1, 1000)
    assert np.array_equal(got["maxpos"][:nb - 1], bins[:nb - 1] + full.argmax(axis=1))
    for i in range(nb - 1, start.size):
        s, e = int(start[i]), int(end[i])
        seg = x[s:e]
        total = float(np.add.reduce(seg))
        assert (int(got["count"][i]), got["sum"][i], got["mean"][i]) == (e - s, total, total / (e - s)), i
        assert got["max"][i] == seg.max() and got["min"][i] == seg.min() and int(got["maxpos"][i]) == s + int(seg.argmax()), i
    assert np.array_equal(d.numpy().view(np.uint64), x.view(np.uint64))           # unchanged afterwards


def flagged_beyond_the_first_tile():
    """Two vectors in one call.  Both are integer read depth, which flags nothing; the second starts on an odd element of
    its buffer (8-byte but not 16-byte aligned: its frame has a lead), is 2 T + 5 long, and has huge cancelling triples in
    its second tile and across the boundary into its third.  The piece [2 T - 1, 2 T + 5), all of it in the third tile, sums
    to -1e308 + 2 + 2^-200, which no two doubles hold: asked for alone, it is one piece and that piece is flagged.  Checked
    against the exact checker -> (one hash of every byte returned, the flagged pieces of the first call)"""
    g = dev()
    T = g.interval_stats_tile()
    rng = np.random.default_rng(21)
    n = 2 * T + 5
    x0, x1 = rng.integers(0, 60, 1000).astype(np.float64), rng.integers(0, 60, n).astype(np.float64)
    for a, b in ((T + 100, T + 400), (2 * T - 32, 2 * T + 4)):               # (frame tile k is [k T - 1, (k + 1) T - 1) of x1)
        x1[a:b:3], x1[a + 1:b:3], x1[a + 2:b:3] = 1e308, 1.0, -1e308
    x1[2 * T + 4] = 2.0 ** -200
    d0, d1 = g.DeviceVector.from_numpy(x0), g.DeviceVector.from_numpy(np.concatenate([[1e300], x1]))
    iv = [(0, 0, 1000), (0, 10, 20),
          (1, T + 50, T + 500), (1, T + 100, T + 103), (1, T - 1, 2 * T - 1),     # wholly inside the second tile
          (1, 2 * T - 100, 2 * T + 3), (1, 2 * T - 2, 2 * T + 5),                 # across into the third
          (1, 0, n), (1, 0, T - 1), (1, 1, n - 1)]
    which, start, end = (np.array(a, np.uint32) for a in zip(*iv))
    got = g.interval_stats([d0, (d1, 1, n)], start, end, vec=which)
    flagged = g.interval_stats_last()["flagged"]
    third = g.interval_stats([d0, (d1, 1, n)], [2 * T - 1], [2 * T + 5], vec=[1])
    last = g.interval_stats_last()
    assert (last["pieces"], last["flagged"]) == (1, 1), last
    h = hashlib.sha256()
    for k, x in enumerate((x0, x1)):
        sel = which == k
        check({name: got[name][sel] for name in got}, x, start[sel], end[sel], what=k)
    check(third, x1, [2 * T - 1], [2 * T + 5], what="third tile")
    for table in (got, third):
        for name in sorted(table):
            h.update(np.ascontiguousarray(table[name]).tobytes())
    return h.hexdigest(), flagged


@pytest.mark.gpu
def test_flagged_pieces_beyond_the_first_tile_and_vector():
    """the second, exact sum of a flagged piece reads the right stretch wherever the piece lies; and again with every
    device allocation poisoned (the library's own staging and image buffers among them), in a fresh process"""
    want, flagged = flagged_beyond_the_first_tile()
    assert flagged > 0
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GDSP_POISON="nan"),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip().splitlines()[-1] == "%s %d" % (want, flagged)


@pytest.mark.gpu
def test_many_small_launches_give_the_same_figures():
    """Three vectors in one call, the second a slice at offset 1 of its buffer, a few hundred intervals of one, two and
    three pieces, unsorted; the first vector has huge cancelling values, so pieces over them are flagged.  At most three
    pieces per launch: the figures are those of one launch, bit for bit, the flagged pieces' second sums among them."""
    g = dev()
    T = g.interval_stats_tile()
    rng = np.random.default_rng(33)
    ns = [2 * T + 300, T + 700, 3000]
    xs = [rng.integers(0, 60, ns[0]).astype(np.float64), rng.integers(0, 60, ns[1] + 1).astype(np.float64),
          rng.standard_normal(ns[2]) * 10.0]
    a, b = T + 100, T + 400
    xs[0][a:b:3], xs[0][a + 1:b:3], xs[0][a + 2:b:3] = 1e308, 1.0, -1e308
    xs[0][2 * T:2 * T + 3] = -1e308, 8.0, 2.0 ** -200                        # a sum no two doubles hold: its piece is flagged
    ds = [g.DeviceVector.from_numpy(x) for x in xs]
    vecs = [ds[0], (ds[1], 1, ns[1]), ds[2]]
    iv = [(0, T + 50, T + 500), (0, T + 100, T + 103), (0, T - 5, 2 * T + 5), (0, 0, ns[0]), (0, T - 1, T), (0, T, T + 1),
          (0, 2 * T, 2 * T + 6),
          (1, T - 3, T + 3), (1, 0, ns[1]), (1, T - 2, T - 1), (2, 0, ns[2]), (2, ns[2] - 1, ns[2])]
    for _ in range(300):
        k = int(rng.integers(0, 3))
        s = int(rng.integers(0, ns[k] - 1))
        iv.append((k, s, min(ns[k], s + 1 + int(rng.integers(0, 600)))))
    order = rng.permutation(len(iv))
    which, start, end = (np.array([iv[i][c] for i in order], np.uint32) for c in range(3))
    got = g.interval_stats(vecs, start, end, vec=which)
    whole = g.interval_stats_last()
    assert whole["intervals"] == start.size and whole["pieces"] > start.size + 10 and whole["flagged"] >= 1
    g.interval_stats_set_launch_pieces(3)
    try:
        small = g.interval_stats(vecs, start, end, vec=which)
        split = g.interval_stats_last()
    finally:
        g.interval_stats_set_launch_pieces(0)
    assert sorted(small) == sorted(got) and len(got) == 6
    for name in got:
        assert np.array_equal(small[name].view(np.uint64), got[name].view(np.uint64)), name
    assert split["pieces"] == whole["pieces"] and split["intervals"] == start.size
    assert split["flagged"] >= 1
    with pytest.raises(g.GdspError):
        g.interval_stats_set_launch_pieces((1 << 22) + 1)


if __name__ == "__main__":
    print("%s %d" % flagged_beyond_the_first_tile())
