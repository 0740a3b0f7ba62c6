"""stats / normalize / multiplyconst / divideconst (not in the reference) through the library: gdsp_genome_stats and
the accumulator of include/genodsp_hip.h.  Every figure is exact and rounded once, so everything here is bit for bit:
the host rounding of hand-built images (no GPU), then the device passes against the exact checker tests/xsum_ref.py
on adversarial data, and the same figures from different cuts of one genome."""
import ctypes
import json
import math
import os
import socket
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import xsum_ref as ref
from conftest import ROOT

DBL_MAX = ref.DBL_MAX
TINY = 5e-324
WORDS = 72


def gd():
    import genodsp_amd
    return genodsp_amd


def img_of(M, n=1, inf=0):
    """a hand-built image of the value M * 2^-1074 (M a Python int), in canonical digits"""
    w = np.zeros(WORDS, np.uint64)
    for k in range(67):
        w[k] = (M >> (32 * k)) & 0xFFFFFFFF
    w[67] = (M >> (32 * 67)) & 0xFFFFFFFFFFFFFFFF
    w[68], w[69] = n, inf
    return w


def bits(x):
    return np.float64(x).tobytes()


# ------------------------------------------------------------------------------------------------ CPU ----

def test_checker_agrees_with_fsum():
    rng = np.random.default_rng(1)
    for x in (rng.standard_normal(1000) * 10, rng.integers(0, 50, 777).astype(np.float64),
              np.array([1e308, 1.0, -1e308]), rng.standard_normal(300) * 1e-310, np.array([0.1] * 10),
              np.ldexp(rng.standard_normal(500), rng.integers(-1000, 1000, 500))):
        assert bits(ref.stats(x)[1]) == bits(math.fsum(x))
        assert Fraction(ref.exact_int(x), 1 << 1074) == sum(Fraction(v) for v in x.tolist())


def test_rounding_at_every_boundary():
    r = gd().xsum_round
    assert bits(r(img_of(0))) == bits(0.0)                                   # exact zero: +0.0
    assert bits(r(img_of(3) - img_of(3) + img_of(0))) == bits(0.0)
    assert r(img_of(1)) == TINY and r(img_of(-1)) == -TINY                   # the subnormal range
    assert r(img_of(12345)) == 12345 * TINY
    assert r(img_of(1 << 1074)) == 1.0
    # ties to even: 1 + 2^-53 -> 1, 1 + 3*2^-53 -> 1 + 2^-51
    one = 1 << 1074
    assert r(img_of(one + (1 << (1074 - 53)))) == 1.0
    assert r(img_of(one + 3 * (1 << (1074 - 53)))) == 1.0 + 2.0 ** -51
    assert r(img_of(one + (1 << (1074 - 53)) + 1)) == 1.0 + 2.0 ** -52      # above the tie by 2^-1074
    assert r(img_of(-(one + (1 << (1074 - 53))))) == -1.0
    # DBL_MAX + half an ulp -> inf, a hair below -> DBL_MAX
    big = ((1 << 1024) - (1 << 970)) << 1074
    assert r(img_of(big)) == math.inf and r(img_of(-big)) == -math.inf
    assert r(img_of(big - 1)) == DBL_MAX and r(img_of(-(big - 1))) == -DBL_MAX
    assert r(img_of(1 << (1024 + 40 + 1074))) == math.inf
    # the smallest normal and the largest subnormal, and the tie between them
    assert r(img_of(1 << 52)) == 2.0 ** -1022
    assert r(img_of((1 << 52) - 1)) == 2.0 ** -1022 - TINY
    assert r(img_of(3, inf=1)) == math.inf                                    # some q was +inf


def test_rounding_of_unnormalised_images():
    """an image straight from the accumulate (signed digits of any size, not carried) rounds like its canonical form"""
    rng = np.random.default_rng(7)
    for _ in range(200):
        w = np.zeros(WORDS, np.uint64)
        M = 0
        for k in rng.integers(0, 67, 5):
            d = int(rng.integers(-2 ** 62, 2 ** 62))
            w[k] = np.uint64((int(w[k]) + d) & 0xFFFFFFFFFFFFFFFF)
            M += d << (32 * int(k))
        assert bits(gd().xsum_round(w)) == bits(ref.round_ratio(M, 1 << 1074))


def test_division_by_n_against_fraction():
    dr = gd().xsum_div_round
    rng = np.random.default_rng(2)
    max32 = (int(DBL_MAX) << 1074) * 2 ** 32                                # 2^32 copies of DBL_MAX
    cases = [(1, 3), (-1, 3), (1, 2), (3, 2), (5, 2), (7, 4), (1 << 1074, 3), (-(1 << 1074), 7), (1, 1 << 63),
             ((1 << 1024) - 1 << 1074, 1), (((1 << 1024) - (1 << 970)) << 1074, 1), (max32, 2 ** 32),
             (2 ** 2100, 2 ** 64 - 1), (12345678901234567890123456789, 2 ** 40 + 17)]
    for _ in range(300):
        M = int(rng.integers(1, 2 ** 62)) << int(rng.integers(0, 2000))
        cases.append((M if rng.random() < 0.5 else -M, int(rng.integers(1, 2 ** 63))))
    for M, n in cases:
        want = ref.round_ratio(M, n << 1074)
        got = dr(img_of(M), n)
        assert bits(got) == bits(want), (M, n, got, want)
        if math.isfinite(want) and want != 0:                                # against Fraction, rounded once
            assert Fraction(want) == Fraction(M, n << 1074) or \
                abs(Fraction(want) - Fraction(M, n << 1074)) <= abs(Fraction(math.nextafter(want, math.inf)) - Fraction(want)) / 2
    assert dr(img_of(max32), 2 ** 32) == DBL_MAX                       # 2^32 copies of DBL_MAX: mean DBL_MAX
    assert math.isnan(dr(img_of(5), 0))
    assert dr(img_of(5, inf=2), 3) == math.inf


def test_host_deposit_builds_the_checkers_image():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(100) * 10, [DBL_MAX, -DBL_MAX, TINY, -TINY, 0.0, -0.0, 2.0 ** -1022],
                        np.ldexp(1.0, np.arange(-1074, 1024))])
    w = np.zeros(WORDS, np.uint64)
    for v in x:
        gd().xsum_add_host(w, v)
    assert int(w[68]) == x.size
    assert bits(gd().xsum_round(w)) == bits(ref.stats(x)[1])
    assert bits(gd().xsum_div_round(w, x.size)) == bits(ref.stats(x)[2])
    gd().xsum_add_host(w, math.nan)                                          # non-finite values are not added
    assert int(w[68]) == x.size


def test_header_declares_the_layout():
    text = open(os.path.join(ROOT, "include", "genodsp_hip.h")).read()
    defs = dict(l.split()[1:3] for l in text.splitlines() if l.startswith("#define GDSP_XSUM_"))
    g = gd()
    assert int(defs["GDSP_XSUM_WORDS"]) == g.XSUM_WORDS == WORDS
    assert int(defs["GDSP_XSUM_DIGITS"]) == g.XSUM_DIGITS == 68
    assert int(defs["GDSP_XSUM_WORD_COUNT"]) == g.XSUM_WORD_COUNT
    assert int(defs["GDSP_XSUM_WORD_INF"]) == g.XSUM_WORD_INF
    assert int(defs["GDSP_XSUM_WORD_FLUSHES"]) == g.XSUM_WORD_FLUSHES


# ------------------------------------------------------------------------------------------------ GPU ----

def dev():
    g = gd()
    g.set_device(0)
    return g


def data(kind, n, rng):
    if kind == "real":
        return rng.standard_normal(n) * 10.0
    if kind == "depth":
        return rng.integers(0, 60, n).astype(np.float64)
    if kind == "cancel":
        x = rng.standard_normal(n)
        x[::3] = 1e308
        x[1::3] = 1.0
        x[2::3] = -1e308
        return x
    if kind == "subnormal":
        return rng.integers(-2 ** 52, 2 ** 52, n).astype(np.float64) * TINY
    if kind == "exponents":
        e = np.arange(n) % 2098 - 1074
        return np.where(rng.random(n) < 0.5, -1.0, 1.0) * np.ldexp(1.0, e)
    if kind == "altmax":
        return np.where(np.arange(n) % 2 == 0, DBL_MAX, -DBL_MAX)
    if kind == "max":
        return np.full(n, DBL_MAX)
    if kind == "specials":
        x = rng.standard_normal(n) * 100
        pool = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 5e3])
        pick = rng.random(n) < 0.2
        x[pick] = rng.choice(pool, int(pick.sum()))
        return x
    if kind == "spread":                                  # a residual at nearly every add
        return np.ldexp(rng.standard_normal(n), rng.integers(-1074, 1000, n))
    raise ValueError(kind)


KINDS = ["real", "depth", "cancel", "subnormal", "exponents", "altmax", "max", "specials", "spread"]


def check(got, want, what=""):
    keys = ("count", "sum", "mean", "variance", "stddev")
    for k, w in zip(keys, want):
        assert ref.same(got[k], w), (what, k, got[k], w)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 4095, 4096, 4097, 300001])
def test_matches_the_checker(kind, n):
    g = dev()
    rng = np.random.default_rng(n)
    x = data(kind, n, rng)
    got = g.genome_stats([g.DeviceVector.from_numpy(x)])
    check(got, ref.genome([x]), (kind, n))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["real", "depth", "specials", "cancel"])
@pytest.mark.parametrize("window,lo,hi", [(1, -DBL_MAX, DBL_MAX), (7, -DBL_MAX, DBL_MAX), (1, 0.5, 30.0), (100, -5.0, 1e301)])
def test_window_and_range(kind, window, lo, hi):
    g = dev()
    rng = np.random.default_rng(window)
    xs = [data(kind, n, rng) for n in (100003, 77, 4096 * 3 + 1)]
    got = g.genome_stats([g.DeviceVector.from_numpy(x) for x in xs], window=window, lo=lo, hi=hi)
    check(got, ref.genome(xs, window, lo, hi), (kind, window))


@pytest.mark.gpu
def test_every_exponent_and_the_overflowing_sum():
    g = dev()
    e = np.ldexp(1.0, np.arange(-1074, 1024))
    check(g.genome_stats([g.DeviceVector.from_numpy(np.concatenate([e, -e[::2]]))]), ref.stats(np.concatenate([e, -e[::2]])))
    # 2^20 copies of DBL_MAX: the sum is +inf, the mean DBL_MAX, the variance 0
    x = np.full(1 << 20, DBL_MAX)
    got = g.genome_stats([g.DeviceVector.from_numpy(x)])
    assert got["sum"] == math.inf and got["mean"] == DBL_MAX and got["variance"] == 0.0 and got["count"] == 1 << 20
    # alternating +-DBL_MAX: sum 0, mean 0, every q = DBL_MAX^2 = +inf
    x = np.where(np.arange(1000) % 2 == 0, DBL_MAX, -DBL_MAX)
    got = g.genome_stats([g.DeviceVector.from_numpy(x)])
    assert bits(got["sum"]) == bits(0.0) and bits(got["mean"]) == bits(0.0) and got["variance"] == math.inf
    assert g.genome_stats_last()["inf_squares"] == 1000
    # [1e308, 1, -1e308]: a naive sum gives 0
    got = g.genome_stats([g.DeviceVector.from_numpy(np.array([1e308, 1.0, -1e308]))])
    assert got["sum"] == 1.0 and got["mean"] == 1.0 / 3


@pytest.mark.gpu
def test_an_empty_sample():
    g = dev()
    got = g.genome_stats([g.DeviceVector.from_numpy(np.array([np.nan, np.inf, 3.0]))], lo=5.0)
    assert got["count"] == 0 and bits(got["sum"]) == bits(0.0) and math.isnan(got["mean"]) and math.isnan(got["stddev"])
    assert g.genome_stats([])["count"] == 0


@pytest.mark.gpu
def test_a_whole_chromosome():
    """chr1, 248,956,422 bases of synthetic real-valued coverage and of read depth"""
    g = dev()
    n = 248956422
    for mode in (1, 0):
        d = g.synth_coverage(20240611, 0, 0, n, mode)
        got = g.genome_stats([d])
        x = d.numpy()
        check(got, ref.stats(x), mode)
        st = g.genome_stats_last()
        assert st["count"] == n
        del d, x


def pieces_of(g, x, cuts, window=1, lo=-DBL_MAX, hi=DBL_MAX):
    """x as one vector cut at `cuts` (odd offsets too: 8-byte aligned sources)"""
    v = g.DeviceVector.from_numpy(x)
    edges = [0] + list(cuts) + [x.size]
    return v, [(v, a, b - a) for a, b in zip(edges[:-1], edges[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("window", [1, 3, 1000])
def test_the_cut_does_not_matter(window):
    """one vector, many pieces (stretches at odd offsets), a batch of 40 vectors against one call per vector added
    with the accumulator, two streams: the same canonical image and the same figures, bit for bit"""
    g = dev()
    rng = np.random.default_rng(11)
    x = np.concatenate([data("real", 200000, rng), data("spread", 50000, rng), data("depth", 60001, rng)])
    want = ref.genome([x], window)
    v, whole = pieces_of(g, x, [])
    check(g.genome_stats([v], window=window), want, "whole")
    cuts = sorted(set(int(c) for c in rng.integers(1, x.size - 1, 45)))
    v, parts = pieces_of(g, x, cuts)
    check(g.genome_stats(parts, window=window), want, "pieces")                  # 46 pieces: two launches
    a = g.xsum_image([v], window=window)
    b = g.xsum_image(parts, window=window)
    assert np.array_equal(np.delete(a, 70), np.delete(b, 70))                  # (word 70 counts flushes: it may differ)
    assert np.array_equal(np.delete(a, [69, 70, 71]), np.delete(ref.image(ref.sample(x, window)), [69, 70, 71]))
    # per piece, accumulated one call after the other into one image, on two streams
    s1, s2 = g.Stream(), g.Stream()
    acc = g.DeviceBuffer(WORDS * 8)
    g.call("gdsp_xsum_init", ctypes.c_void_p(acc.ptr), None)
    g.sync(None)
    for i, p in enumerate(parts):
        s = (s1 if i % 2 else s2).handle
        g.xsum_accumulate([p], acc, window=window, stream=s)
        g.sync(s)
    w = acc.download(np.uint64, WORDS)
    assert bits(g.xsum_round(w)) == bits(want[1]) and bits(g.xsum_div_round(w, int(w[68]))) == bits(want[2])


@pytest.mark.gpu
def test_a_batch_of_many_vectors():
    g = dev()
    rng = np.random.default_rng(5)
    xs = [data(KINDS[i % len(KINDS)], int(rng.integers(1, 30000)), rng) for i in range(70)]
    vs = [g.DeviceVector.from_numpy(x) for x in xs]
    check(g.genome_stats(vs), ref.genome(xs))
    one = [g.xsum_image([v]) for v in vs]
    total = np.zeros(WORDS, np.uint64)
    for im in one:
        total += im
    all_ = g.xsum_image(vs)
    assert bits(g.xsum_round(total)) == bits(g.xsum_round(all_)) == bits(ref.genome(xs)[1])
    assert total[68] == all_[68]


@pytest.mark.gpu
def test_constant_operators_and_normalize_match_numpy():
    g = dev()
    rng = np.random.default_rng(9)
    xs = [data(k, n, rng) for k, n in (("real", 100003), ("depth", 4097), ("specials", 9999), ("subnormal", 31))]
    for c in (3.0, 1e-300, -7.25, 1e6, math.pi):
        vs = [g.DeviceVector.from_numpy(x) for x in xs]
        g.multiply_constant(vs, c)
        with np.errstate(all="ignore"):
            for v, x in zip(vs, xs):
                assert v.numpy().tobytes() == (x * c).tobytes()
        vs = [g.DeviceVector.from_numpy(x) for x in xs]
        g.divide_constant(vs, c)
        g.divide_constant(g.DeviceVector.from_numpy(xs[0]), c)
        with np.errstate(all="ignore"):
            for v, x in zip(vs, xs):
                assert v.numpy().tobytes() == (x / c).tobytes()
    with pytest.raises(g.GdspError):
        g.divide_constant([g.DeviceVector.from_numpy(xs[0])], 0.0)
    fin = [x[np.abs(x) < 1e150] for x in xs]                                 # (squares that stay finite)
    for to in ("mean", "zscore"):
        vs = [g.DeviceVector.from_numpy(x) for x in fin]
        st = g.normalize(vs, to=to)
        want = ref.genome(fin)
        check(st, want, to)
        for v, x in zip(vs, fin):
            with np.errstate(all="ignore"):
                w = x / want[2] if to == "mean" else (x - want[2]) / want[4]
            assert v.numpy().tobytes() == w.tobytes(), to
    with pytest.raises(ValueError):
        g.normalize([g.DeviceVector.from_numpy(np.array([1.0, -1.0]))], to="mean")       # mean 0
    with pytest.raises(ValueError):
        g.normalize([g.DeviceVector.from_numpy(np.array([2.0, 2.0]))], to="zscore")      # stddev 0
    with pytest.raises(ValueError):
        g.normalize([g.DeviceVector.from_numpy(np.array([2.0]))], to="median")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


RANK_SCRIPT = r'''
import os, sys, json
import numpy as np
import torch.distributed as dist
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import genodsp_amd as g
import xsum_ref as ref
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
g.set_device(0)
rng = np.random.default_rng(4)
xs = [rng.standard_normal(n) * 10 for n in (50000, 70001, 3, 9000)] + [np.ldexp(rng.standard_normal(20000), rng.integers(-1074, 1000, 20000))]
mine = [g.DeviceVector.from_numpy(x) for i, x in enumerate(xs) if i % world == rank]
import torch
def allreduce(arr, op):
    assert op == "sum"
    t = torch.from_numpy(arr.view(np.int64).copy())
    dist.all_reduce(t)
    return t.numpy().view(np.uint64)
got = g.genome_stats(mine, window=3, allreduce=allreduce)
want = ref.genome(xs, 3)
ok = all(ref.same(got[k], w) for k, w in zip(("count", "sum", "mean", "variance", "stddev"), want))
with open(os.path.join(sys.argv[2], "rank%d.json" % rank), "w") as f:
    json.dump({"rank": rank, "ok": ok, "got": [got[k] for k in ("count", "sum", "mean", "variance", "stddev")]}, f)
dist.destroy_process_group()
'''


@pytest.mark.gpu
def test_the_reduction_hook_over_two_ranks(tmp_path):
    """two processes on the one GPU, each with some of the chromosomes, their images summed by gloo"""
    script = tmp_path / "ranks.py"
    script.write_text(RANK_SCRIPT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), str(script), ROOT, str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.load(open(tmp_path / ("rank%d.json" % r))) for r in (0, 1)]      # (each rank's own file: stdout interleaves)
    assert all(l["ok"] for l in lines), lines
    assert lines[0]["got"] == lines[1]["got"]
