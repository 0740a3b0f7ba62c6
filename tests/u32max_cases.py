"""What the tests of a chromosome of 2^32 - 1 bases share (test_hip_u32max.py, test_hip_u32max_ops.py and the CPU proof
of the method, test_u32max_locality.py).  A plain module, no fixtures.

The method.  A vector of 2^32 - 1 doubles is 34.4 GB: no checker runs over it.  The signal is synthetic and can be
regenerated anywhere (oracle.cpu.synth_coverage), so the device's result is fetched at a list of `places()` -- M bases
each: both ends of the chromosome, either side of base 2^31 (where a signed 32-bit index turns negative), the last seam
below 2^32 of every tiling the library uses (where `i + reach` or the next tile's start wraps in 32 bits), a few random
ones -- and held bit for bit to the operator's CPU checker run over the regenerated window plus a halo.  That is sound
when the halo makes the window independent of the rest of the chromosome; test_u32max_locality.py proves it for every
case of CASES, on the CPU, on a short vector with the same checkers, halos and place rule.

CASES is group A, the operators whose reach is bounded: name -> Case.  A case's checker takes the regenerated tracks (one
array, or the signal and a second track) and returns the expected values over the same bases."""
import numpy as np

from conftest import bits_equal
from oracle import cpu

import distance_ref
import fillgaps_ref
import localcorr_ref
import localmad_ref
import localstats_ref
import prominence_ref
import sliding_percentile_ref

SEED = 20240611
N = 2 ** 32 - 1
CHROM = 3
TRACK_CHROM = 5          # the second track of local_correlation: the same kind of signal, another chromosome index
M = 6000
MEMBER_TILE = 8192       # gdsp_member_tile.h: bases per tile of the membership bits (distance, fillgaps)
WINDOWS = (101, 1001, 4095, 10001)    # the windows of CASES whose tile depends on them

_FIXED_TILES = (2304, 2304 - 10, 3984, 4096, 16384, 32768, 1 << 18)      # smooth, peaks, morphology, cumulativesum


def library_tiles():
    """every tile size the library reports (host calls: no GPU is touched)"""
    import genodsp_amd as gd
    L = gd.lib()
    tiles = [gd.interval_stats_tile(), gd.segments_tile(), gd.paint_tile(), gd.lag_tile(), gd.xsum_pair_tile(), MEMBER_TILE,
             int(L.gdsp_distance_tile()), int(L.gdsp_fillgaps_tile()), int(L.gdsp_interval_tile())]
    for W in WINDOWS:
        tiles += [gd.localmad_tile(W), gd.localcorr_tile(W), int(L.gdsp_prominence_tile(W)), int(L.gdsp_localstats_tile(W)),
                  int(L.gdsp_sliding_percentile_tile(W))]
    return [int(t) for t in tiles if t]                                    # (0: the window is beyond that operator)


_tiles = None


def seam_tiles():
    """the fixed tilings first (as they always were), then what the library adds to them, each once"""
    global _tiles
    if _tiles is None:
        seen = list(_FIXED_TILES)
        for t in library_tiles():
            if t not in seen:
                seen.append(t)
        _tiles = tuple(seen)
    return _tiles


def places(n=N, m=M, mid=2 ** 31):
    """window starts: both ends, either side of `mid`, the last seam of each tiling below n, six random ones"""
    top = []
    for tile in seam_tiles():
        top.append(max(0, min(n - m, (n // tile) * tile - m // 2)))
    rng = np.random.default_rng(5)
    every = [0, mid - m // 2, mid, n - m] + top + [int(s) for s in rng.integers(0, n - m, 6)]
    return list(dict.fromkeys(every))                                     # (tiles below m share the last window: once)


def fetch(vec, start, count):
    return vec.buf.download(np.float64, count, vec.offset + 8 * start)


def regenerate(start, count, halo, mode=1, n=N, chrom=CHROM):
    lo, hi = max(0, start - halo), min(n, start + count + halo)
    return cpu.synth_coverage(SEED, chrom, lo, hi - lo, mode), start - lo


def check(vec, oracle_fn, halo, bound_fn=None):
    for s in places():
        x, left = regenerate(s, M, halo)
        want = oracle_fn(x)[left:left + M]
        got = fetch(vec, s, M)
        if bound_fn is None:
            assert bits_equal(got, want), (s, int(np.flatnonzero(got != want)[0]))
        else:
            assert np.all(np.abs(got - want) <= bound_fn(x)[left:left + M]), s


# ------------------------------------------------------------------------------------------------ group A ----

class Case:
    """One operator at one setting.  mode: 0 integer depth (no sum can round: sums are held bit for bit), 1 real-valued;
    halo: bases regenerated on either side of a window; check(tracks) -> expected values over the tracks' bases;
    run(gd, tracks, out) -> the DeviceVector with the result: `out`, or with in_place the track it overwrote (the
    caller hands it a copy, or the second track); tracks: how many (the second comes from TRACK_CHROM); align: windows start and end at
    multiples of it (window_sum's blocks), or at the vector's end; parts: the tests the places are dealt over, where the
    checker is slow (a 4095-base partition per base), so that each test stays as quick as its neighbours"""

    def __init__(self, mode, halo, check, run, tracks=1, in_place=False, align=1, parts=1):
        self.mode, self.halo, self.check, self.run = mode, halo, check, run
        self.tracks, self.in_place, self.align, self.parts = tracks, in_place, align, parts

    def window(self, start, n=N, m=M):
        """(start, count) of the bases compared at a place"""
        a = self.align
        s = (start // a) * a
        e = min(n, -(-(start + m) // a) * a)
        if n - e < a:
            e = n                                                          # (the last, ragged block comes along)
        return s, e - s

    def regenerate(self, start, count, n=N):
        chroms = (CHROM, TRACK_CHROM)[:self.tracks]
        got = [regenerate(start, count, self.halo, self.mode, n, c) for c in chroms]
        return [x for x, _ in got], got[0][1]

    def expected(self, start, count, n=N):
        xs, left = self.regenerate(start, count, n)
        return self.check(xs)[left:left + count]


T_SPARSE = 60.0          # depth x factor above 60: a sparse set, with gaps below and above 1000 bases


def _exact_stats(x, W, what):
    want, low, high = localstats_ref.local_stats(x, W, what, tile=0)
    assert localstats_ref.same_bits(low, high).all()                        # integer depth: every figure is a point
    return want


def _exact_corr(xs, W, what):
    want, low, high = localcorr_ref.local_correlation(xs[0], xs[1], W, what, tile=0)
    assert localcorr_ref.same_bits(low, high).all()
    return want


def _one_track(fn):
    return lambda gd, t, out: fn(gd, t[0], out)


def _cases():
    c = {}
    for denom in (1.0, 7.0):
        c["sliding_sum-W1001-denom%g" % denom] = Case(
            0, 1001, lambda xs, d=denom: cpu.sliding_sum(xs[0], 1001, d),
            _one_track(lambda gd, v, out, d=denom: gd.sliding_sum(v, 1001, denom=d, out=out)))
    for W in (1000, 8193):
        c["window_sum-W%d" % W] = Case(
            0, 0, lambda xs, W=W: cpu.window_sum(xs[0], W),
            _one_track(lambda gd, v, out, W=W: gd.window_sum(v, W)), in_place=True, align=W)
    for name, mx in (("max", True), ("min", False)):
        c["best_extrema-W1001-%s" % name] = Case(
            1, 1001, lambda xs, mx=mx: cpu.best_extrema(xs[0], 1001, mx),
            _one_track(lambda gd, v, out, mx=mx: gd.best_extrema(v, 1001, mx, out=out)))
    c["local_extrema-N1001"] = Case(
        1, 1001, lambda xs: cpu.local_extrema(xs[0], 1001, True, 0.0),
        _one_track(lambda gd, v, out: gd.local_extrema(v, 1001, True, 0.0, out=out)))
    for W in (101, 4095):
        c["sliding_percentile-W%d" % W] = Case(
            1, W, lambda xs, W=W: sliding_percentile_ref.sliding_percentile(xs[0], W, 50000),
            _one_track(lambda gd, v, out, W=W: gd.sliding_percentile(v, W, 50000, out=out)), parts=4 if W > 1000 else 1)
        for k, as_ in enumerate(("prominence", "base")):
            c["prominence-W%d-%s" % (W, as_)] = Case(
                1, W, lambda xs, W=W, k=k: prominence_ref.prominence(xs[0], W)[k],
                _one_track(lambda gd, v, out, W=W, as_=as_: gd.prominence(v, W, as_=as_, out=out)))
    for W in (101, 10001):
        for as_ in ("zscore", "mean"):
            c["local_stats-W%d-%s" % (W, as_)] = Case(
                0, W, lambda xs, W=W, as_=as_: _exact_stats(xs[0], W, as_),
                _one_track(lambda gd, v, out, W=W, as_=as_: gd.local_stats(v, W, as_=as_, out=out)))
    c["local_mad-W101-zscore"] = Case(
        1, 101, lambda xs: localmad_ref.local_mad(xs[0], 101, "zscore"),
        _one_track(lambda gd, v, out: gd.local_mad(v, 101, as_="zscore", out=out)))
    c["hampel-W1001"] = Case(
        1, 1001, lambda xs: localmad_ref.hampel(xs[0], 1001),
        _one_track(lambda gd, v, out: gd.hampel(v, 1001, out=out)), parts=2)
    for as_ in ("correlation", "covariance"):
        c["local_correlation-W101-%s" % as_] = Case(
            0, 101, lambda xs, as_=as_: _exact_corr(xs, 101, as_),
            lambda gd, t, out, as_=as_: gd.local_correlation(t[0], t[1], 101, as_=as_), tracks=2, in_place=True)
    for name, kw in (("unsigned", {}), ("signed", {"signed": True}), ("left", {"to": "left"})):
        c["distance-cap1000-%s" % name] = Case(
            1, 1001, lambda xs, kw=kw: distance_ref.distance(xs[0], T=T_SPARSE, cap=1000, **kw),
            _one_track(lambda gd, v, out, kw=kw: gd.distance(v, T=T_SPARSE, cap=1000, **kw)), in_place=True)
    for how in ("linear", "nearest"):
        c["fill_gaps-maxgap1000-%s" % how] = Case(           # its reach is maxgap + 1
            1, 1001, lambda xs, how=how: fillgaps_ref.fill_gaps(xs[0], T=T_SPARSE, how=how, maxgap=1000),
            _one_track(lambda gd, v, out, how=how: gd.fill_gaps(v, T=T_SPARSE, how=how, maxgap=1000)), in_place=True)
    return c


CASES = _cases()
