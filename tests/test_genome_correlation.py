"""correlate (not in the reference) through the library: gdsp_genome_correlation and the pair accumulators of
include/genodsp_hip.h.  The sums are exact and rounded once and the rest is derived from them operation by operation,
so everything here is bit for bit against the exact checker tests/correlate_ref.py -- itself checked against
fractions.Fraction -- on adversarial data, in both alignments of y against x, and from different cuts of one genome."""
import json
import math
import os
import random
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import correlate_ref as cref
import xsum_ref as ref
from conftest import ROOT
from test_genome_stats import data, _free_port

DBL_MAX = ref.DBL_MAX
WORDS = 72
TILE = 2048                                        # gdsp_xsum_pair_tile(): test_the_tile_is_what_the_shapes_assume
FIGURES = cref.FIGURES


def gd():
    import genodsp_amd
    return genodsp_amd


def bits(x):
    return np.float64(x).tobytes()


# ------------------------------------------------------------------------------------------------ CPU ----

def small_samples():
    """200 small pair samples: n = 1 .. 40, plain values, integers, and values of very different sizes"""
    rnd = random.Random(17)
    out = []
    for i in range(200):
        n = 1 if i < 5 else rnd.randint(1, 40)
        kind = i % 4
        if kind == 0:
            x = [rnd.gauss(0, 10) for _ in range(n)];  y = [rnd.gauss(3, 2) for _ in range(n)]
        elif kind == 1:
            x = [float(rnd.randint(0, 60)) for _ in range(n)];  y = [2 * v + rnd.randint(-3, 3) for v in x]
        elif kind == 2:
            x = [math.ldexp(rnd.gauss(0, 1), rnd.randint(-300, 300)) for _ in range(n)]
            y = [math.ldexp(rnd.gauss(0, 1), rnd.randint(-300, 300)) for _ in range(n)]
        else:
            x = [rnd.gauss(1e6, 1e-3) for _ in range(n)];  y = [-v + rnd.gauss(0, 1e-6) for v in x]
        out.append((np.array(x, np.float64), np.array(y, np.float64)))
    return out


def fraction_to_double(q):
    return float(q)                                # Fraction.__float__: int / int true division, correctly rounded


def test_checker_agrees_with_fraction():
    """varx and cov: Python floats for the per-pair roundings (each operation IEEE double), Fractions for the sums"""
    for x, y in small_samples():
        n = x.size
        got = dict(zip(FIGURES, cref.figures(x, y)))
        meanx = fraction_to_double(sum(Fraction(v) for v in x.tolist()) / n)
        meany = fraction_to_double(sum(Fraction(v) for v in y.tolist()) / n)
        assert bits(got["meanx"]) == bits(meanx) and bits(got["meany"]) == bits(meany)
        dx = [v - meanx for v in x.tolist()]
        dy = [v - meany for v in y.tolist()]
        varx = fraction_to_double(sum(Fraction(a * a) for a in dx) / n)
        cov = fraction_to_double(sum(Fraction(a * b) for a, b in zip(dx, dy)) / n)
        assert bits(got["varx"]) == bits(varx) and got["count"] == n
        assert bits(got["covariance"] + 0.0) == bits(cov + 0.0), (got["covariance"], cov)


def test_checkers_correlation_is_symmetric():
    seen = 0
    for x, y in small_samples():
        a = dict(zip(FIGURES, cref.figures(x, y)))
        b = dict(zip(FIGURES, cref.figures(y, x)))
        assert ref.same(a["correlation"], b["correlation"]) and ref.same(a["covariance"], b["covariance"])
        assert ref.same(a["varx"], b["vary"]) and ref.same(a["meany"], b["meanx"]) and ref.same(a["sdx"], b["sdy"])
        if not math.isnan(a["correlation"]):
            assert -1.0 <= a["correlation"] <= 1.0
            seen += 1
    assert seen > 150
    one = dict(zip(FIGURES, cref.figures([3.0], [4.0])))                  # n = 1: no spread, nothing to correlate
    assert one["varx"] == 0.0 and one["covariance"] == 0.0 and math.isnan(one["correlation"]) and math.isnan(one["slope"])


def test_header_declares_the_pair_calls_and_the_figure_order():
    text = open(os.path.join(ROOT, "include", "genodsp_hip.h")).read()
    assert "typedef struct gdsp_xsum_pair { const double* d_x; const double* d_y; uint32_t n; uint32_t first; int device; void* stream; } gdsp_xsum_pair;" in text
    for call in ("gdsp_xsum_pair_accumulate_batch", "gdsp_xsum_pair_accumulate_dev_batch", "gdsp_genome_correlation (",
                 "gdsp_genome_correlation_use_comm", "gdsp_genome_correlation_last"):
        assert call in text, call
    enum = text[text.index("enum { GDSP_CORR_COUNT = 0"):]
    enum = enum[:enum.index("}")]
    names = [w.strip().split()[0] for w in enum[len("enum {"):].split(",") if w.strip()]
    assert names == ["GDSP_CORR_COUNT", "GDSP_CORR_SUMX", "GDSP_CORR_SUMY", "GDSP_CORR_MEANX", "GDSP_CORR_MEANY", "GDSP_CORR_VARX",
                     "GDSP_CORR_VARY", "GDSP_CORR_SDX", "GDSP_CORR_SDY", "GDSP_CORR_COV", "GDSP_CORR_CORRELATION", "GDSP_CORR_SLOPE",
                     "GDSP_CORR_INTERCEPT", "GDSP_CORR_FIGURES"]
    assert tuple(gd().CORRELATION_FIGURES) == FIGURES and len(FIGURES) == 13
    assert "Agreement with stats" in text and "Symmetry" in text


def test_the_tile_is_what_the_shapes_assume():
    assert gd().xsum_pair_tile() == TILE


# ------------------------------------------------------------------------------------------------ GPU ----

def dev():
    g = gd()
    g.set_device(0)
    return g


def check(got, want, what=""):
    for k, w in zip(FIGURES, want):
        assert ref.same(got[k], w), (what, k, got[k], w)


def pair_of(g, x, y, ox=0, oy=0):
    """x and y as slices, at offsets ox and oy, of parent vectors: (0,0) and (1,1) are congruent modulo 16 bytes, (0,1)
    and (1,0) are not.  The window counts from the slice's first value."""
    n = x.size
    vx = g.DeviceVector.from_numpy(np.concatenate([np.full(ox, 1e9), x, [7e8]]))
    vy = g.DeviceVector.from_numpy(np.concatenate([np.full(oy, -1e9), y, [-7e8]]))
    return ((vx, ox, n, 0), (vy, oy, n, 0))


OFFSETS = [(0, 0), (1, 1), (0, 1), (1, 0)]
KIND_PAIRS = [("real", "real"), ("depth", "depth"), ("cancel", "real"), ("real", "cancel"), ("subnormal", "subnormal"),
              ("altmax", "depth"), ("depth", "altmax"), ("spread", "spread"), ("spread", "depth"), ("specials", "specials"),
              ("specials", "real"), ("depth", "specials")]


def two(kinds, n, seed):
    """x and y of the two kinds, drawn independently"""
    rng = np.random.default_rng(seed)
    return data(kinds[0], n, rng), data(kinds[1], n, rng)


@pytest.mark.gpu
@pytest.mark.parametrize("kinds", KIND_PAIRS, ids=lambda k: "-".join(k))
@pytest.mark.parametrize("n", [1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 300001])
def test_matches_the_checker(kinds, n):
    g = dev()
    x, y = two(kinds, n, n)
    want = cref.genome([(x, y)])
    for ox, oy in OFFSETS:
        check(g.genome_correlation([pair_of(g, x, y, ox, oy)]), want, (kinds, n, ox, oy))


def test_specials_land_in_x_only_in_y_only_and_in_both():
    x, y = two(("specials", "specials"), 300001, 300001)
    bx, by = ~np.isfinite(x), ~np.isfinite(y)
    assert (bx & ~by).any() and (~bx & by).any() and (bx & by).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kinds", [("real", "real"), ("depth", "real"), ("specials", "specials"), ("cancel", "depth")],
                         ids=lambda k: "-".join(k))
@pytest.mark.parametrize("window,lo,hi,ylo,yhi", [(1, -DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX), (7, -DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX),
                                                  (1, 0.5, 30.0, -DBL_MAX, DBL_MAX), (100, -DBL_MAX, DBL_MAX, -5.0, 1e301),
                                                  (3, -2.0, 25.0, 0.5, 30.0)])
def test_window_and_limits(kinds, window, lo, hi, ylo, yhi):
    g = dev()
    ps = [two(kinds, n, window * 1000 + n) for n in (100003, 77, 3 * TILE + 1)]
    for offs in ((0, 0), (1, 0)):
        got = g.genome_correlation([pair_of(g, x, y, *offs) for x, y in ps], window=window, lo=lo, hi=hi, ylo=ylo, yhi=yhi)
        check(got, cref.genome(ps, window, lo, hi, ylo, yhi), (kinds, window, offs))


@pytest.mark.gpu
def test_identities():
    g = dev()
    rng = np.random.default_rng(21)
    for kind in ("real", "depth", "wide"):
        n = 3 * TILE + 5
        x = data(kind, n, rng) if kind != "wide" else np.ldexp(rng.standard_normal(n), rng.integers(-400, 400, n))   # (squares stay finite)
        vx = g.DeviceVector.from_numpy(x)
        st = g.genome_stats([vx])
        # y = x
        got = g.genome_correlation([(vx, g.DeviceVector.from_numpy(x))])
        assert bits(got["covariance"]) == bits(got["varx"]) == bits(got["vary"]) == bits(st["variance"]), kind
        assert abs(got["correlation"] - 1.0) <= 2.0 ** -51, (kind, got["correlation"])      # one sqrt, one product, one division: half an ulp each
        check(got, cref.genome([(x, x)]), kind)
        # y = -x
        got = g.genome_correlation([(vx, g.DeviceVector.from_numpy(-x))])
        assert bits(got["covariance"]) == bits(-got["varx"]), kind
        assert abs(got["correlation"] + 1.0) <= 2.0 ** -51, (kind, got["correlation"])
        # swapped arguments, with limits: swapped figures, the same cov and r
        y = data("real", x.size, rng)
        vy = g.DeviceVector.from_numpy(y)
        lim = dict(lo=-1e300, hi=50.0, ylo=-15.0, yhi=12.0)
        a = g.genome_correlation([(vx, vy)], window=3, **lim)
        b = g.genome_correlation([(vy, vx)], window=3, lo=lim["ylo"], hi=lim["yhi"], ylo=lim["lo"], yhi=lim["hi"])
        for p, q in (("sumx", "sumy"), ("meanx", "meany"), ("varx", "vary"), ("sdx", "sdy")):
            assert ref.same(a[p], b[q]) and ref.same(a[q], b[p]), (kind, p)
        assert ref.same(a["covariance"], b["covariance"]) and ref.same(a["correlation"], b["correlation"]) and a["count"] == b["count"]
        assert not math.isnan(a["correlation"])
        # every sampled y admitted: x's figures are stats'
        for window, lo, hi in ((1, -DBL_MAX, DBL_MAX), (7, 0.5, 30.0)):
            a = g.genome_correlation([(vx, vy)], window=window, lo=lo, hi=hi)
            st = g.genome_stats([vx], window=window, lo=lo, hi=hi)
            for p, q in (("count", "count"), ("sumx", "sum"), ("meanx", "mean"), ("varx", "variance"), ("sdx", "stddev")):
                assert ref.same(a[p], st[q]), (kind, window, p)
    # constant x
    y = data("real", 5000, rng)
    got = g.genome_correlation([(g.DeviceVector.from_numpy(np.full(5000, 2.5)), g.DeviceVector.from_numpy(y))])
    assert bits(got["varx"]) == bits(0.0) and math.isnan(got["correlation"]) and math.isnan(got["slope"]) and math.isnan(got["intercept"])
    assert got["vary"] > 0
    # y = 2x + 3 on read depth
    x = data("depth", 100003, rng)
    y = 2 * x + 3
    got = g.genome_correlation([(g.DeviceVector.from_numpy(x), g.DeviceVector.from_numpy(y))])
    check(got, cref.genome([(x, y)]), "2x+3")
    assert abs(got["slope"] - 2.0) < 1e-12 and abs(got["intercept"] - 3.0) < 1e-9 and abs(got["correlation"] - 1.0) <= 2.0 ** -51


@pytest.mark.gpu
def test_overflow():
    """x alternating +-DBL_MAX: every qxx is +inf.  Against y = 1, 2, 1, 2, ... the deviations of y are -+0.5, so by the
    definition every qxy = fl(+-DBL_MAX * -+0.5) is the finite -DBL_MAX/2 and cov is exactly that (not NaN: a product
    of DBL_MAX overflows only against a |dy| above 1); against y = 1, 5, 1, 5, ... (dy = -+2) every qxy is -inf, is
    counted and not added, and cov is NaN.  r is NaN in both, varx being +inf."""
    g = dev()
    n = 1000
    x = np.where(np.arange(n) % 2 == 0, DBL_MAX, -DBL_MAX)
    y = np.where(np.arange(n) % 2 == 0, 1.0, 2.0)
    got = g.genome_correlation([(g.DeviceVector.from_numpy(x), g.DeviceVector.from_numpy(y))])
    assert got["varx"] == math.inf and math.isnan(got["correlation"]) and math.isnan(got["slope"])
    assert bits(got["covariance"]) == bits(-DBL_MAX / 2)
    assert bits(got["meanx"]) == bits(0.0) and got["meany"] == 1.5 and got["vary"] == 0.25
    last = g.genome_correlation_last()
    assert last["count"] == n and last["nonfinite_qxx"] == n and last["nonfinite_qxy"] == 0 and last["nonfinite_qyy"] == 0
    check(got, cref.genome([(x, y)]), "altmax, |dy| = 0.5")
    y = np.where(np.arange(n) % 2 == 0, 1.0, 5.0)
    got = g.genome_correlation([(g.DeviceVector.from_numpy(x), g.DeviceVector.from_numpy(y))])
    assert got["varx"] == math.inf and math.isnan(got["covariance"]) and math.isnan(got["correlation"])
    assert got["meany"] == 3.0 and got["vary"] == 4.0
    last = g.genome_correlation_last()
    assert last["count"] == n and last["nonfinite_qxx"] == n and last["nonfinite_qxy"] == n and last["nonfinite_qyy"] == 0
    check(got, cref.genome([(x, y)]), "altmax, |dy| = 2")
    x, y = np.array([1e308, 1.0, -1e308]), np.array([1.0, 2.0, 3.0])
    got = g.genome_correlation([(g.DeviceVector.from_numpy(x), g.DeviceVector.from_numpy(y))])
    assert got["meanx"] == 1.0 / 3 and got["sumx"] == 1.0 and got["meany"] == 2.0
    check(got, cref.genome([(x, y)]), "cancel")


@pytest.mark.gpu
def test_an_empty_sample():
    g = dev()
    x, y = np.array([np.nan, np.inf, 3.0]), np.array([1.0, 2.0, 3.0])
    for got in (g.genome_correlation([(g.DeviceVector.from_numpy(x), g.DeviceVector.from_numpy(y))], lo=5.0),
                g.genome_correlation([(g.DeviceVector.from_numpy(x), g.DeviceVector.from_numpy(y))], ylo=5.0),
                g.genome_correlation([])):
        assert got["count"] == 0 and bits(got["sumx"]) == bits(0.0) and bits(got["sumy"]) == bits(0.0)
        assert all(math.isnan(got[k]) for k in FIGURES[3:])


@pytest.mark.gpu
@pytest.mark.parametrize("window", [1, 3, 1000])
def test_the_cut_does_not_matter(window):
    """one pair of vectors whole and as 46 pieces at random cuts (odd offsets too): the same canonical images of both
    passes, word for word, and the same figures"""
    g = dev()
    rng = np.random.default_rng(11)
    x = np.concatenate([data("real", 200000, rng), data("spread", 50000, rng), data("depth", 60001, rng)])
    y = np.concatenate([data("depth", 200000, rng), data("spread", 50000, rng), data("real", 60001, rng)])
    assert x.size == 310001
    sx, sy = cref.pair_sample(x, y, window)
    want = cref.figures(sx, sy)
    vx, vy = g.DeviceVector.from_numpy(x), g.DeviceVector.from_numpy(y)
    cuts = sorted(set(int(c) for c in rng.integers(1, x.size - 1, 45)))
    edges = [0] + cuts + [x.size]
    parts = [((vx, a, b - a), (vy, a, b - a)) for a, b in zip(edges[:-1], edges[1:])]
    assert any(a % 2 for a in cuts)
    check(g.genome_correlation([(vx, vy)], window=window), want, "whole")
    check(g.genome_correlation(parts, window=window), want, "pieces")
    means = (want[3], want[4])
    for m in (None, means):
        a = g.xsum_pair_image([(vx, vy)], window=window, means=m)
        b = g.xsum_pair_image(parts, window=window, means=m)
        assert a.shape == (2 if m is None else 3, WORDS)
        assert np.array_equal(np.delete(a, 70, axis=1), np.delete(b, 70, axis=1))      # (word 70 counts flushes: it may differ)
        assert np.array_equal(np.delete(a, [70, 71], axis=1), np.delete(cref.images(sx, sy, m), [70, 71], axis=1))


@pytest.mark.gpu
def test_a_batch_of_many_pairs():
    g = dev()
    rng = np.random.default_rng(5)
    ps = []
    for i in range(70):
        n = int(rng.integers(1, 30000))
        ps.append((data(KIND_PAIRS[i % len(KIND_PAIRS)][0], n, rng), data(KIND_PAIRS[(i * 5 + 1) % len(KIND_PAIRS)][1], n, rng)))
    tab = [pair_of(g, x, y, i % 2, (i // 2) % 2) for i, (x, y) in enumerate(ps)]
    want = cref.genome(ps)
    check(g.genome_correlation(tab), want, "batch")
    for m in (None, (want[3], want[4])):
        total = np.zeros((2 if m is None else 3, WORDS), np.uint64)
        for t in tab:
            total += g.xsum_pair_image([t], means=m)
        all_ = g.xsum_pair_image(tab, means=m)
        for k in range(total.shape[0]):
            assert bits(g.xsum_round(total[k])) == bits(g.xsum_round(all_[k]))
            assert total[k][68] == all_[k][68] == want[0] and total[k][69] == all_[k][69]
        if m is None:
            assert bits(g.xsum_round(all_[0])) == bits(want[1]) and bits(g.xsum_round(all_[1])) == bits(want[2])


RANK_SCRIPT = r'''
import os, sys, json
import numpy as np
import torch
import torch.distributed as dist
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import genodsp_amd as g
import correlate_ref as cref
import xsum_ref as ref
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
g.set_device(0)
rng = np.random.default_rng(4)
ps = [(rng.standard_normal(n) * 10, rng.integers(0, 60, n).astype(np.float64)) for n in (50000, 70001, 3, 9000)]
ps.append((np.ldexp(rng.standard_normal(20000), rng.integers(-1074, 1000, 20000)), rng.standard_normal(20000)))
mine = [(g.DeviceVector.from_numpy(x), g.DeviceVector.from_numpy(y)) for i, (x, y) in enumerate(ps) if i % world == rank]
sizes = []
def allreduce(arr, op):
    assert op == "sum"
    sizes.append(int(arr.size))
    t = torch.from_numpy(arr.view(np.int64).copy())
    dist.all_reduce(t)
    return t.numpy().view(np.uint64)
got = g.genome_correlation(mine, window=3, allreduce=allreduce)
want = cref.genome(ps, 3)
ok = all(ref.same(got[k], w) for k, w in zip(cref.FIGURES, want)) and sizes == [144, 216]
with open(os.path.join(sys.argv[2], "rank%d.json" % rank), "w") as f:
    json.dump({"rank": rank, "ok": ok, "sizes": sizes, "got": [repr(got[k]) for k in cref.FIGURES]}, f)
dist.destroy_process_group()
'''


@pytest.mark.gpu
def test_the_reduction_hook_over_two_ranks(tmp_path):
    """two fresh processes on the one GPU, each with some of the pairs, their images summed by gloo: once per pass, over
    the images side by side (144 words, then 216)"""
    script = tmp_path / "ranks.py"
    script.write_text(RANK_SCRIPT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), str(script), ROOT, str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.load(open(tmp_path / ("rank%d.json" % r))) for r in (0, 1)]      # (each rank's own file: stdout interleaves)
    assert all(l["ok"] for l in lines), lines
    assert lines[0]["got"] == lines[1]["got"]


@pytest.mark.gpu
def test_a_long_chromosome():
    """2^26 + 1 bases of synthetic real-valued coverage and of read depth, x and y from two seeds.  (Not chr1's
    248,956,422: the checker sorts the sample five times per mode, which takes minutes on the host at that length.)"""
    g = dev()
    n = (1 << 26) + 1
    for mode in (1, 0):
        dx = g.synth_coverage(20240611, 0, 0, n, mode)
        dy = g.synth_coverage(19700101, 0, 0, n, mode)
        got = g.genome_correlation([(dx, dy)])
        x, y = dx.numpy(), dy.numpy()
        check(got, cref.figures(x, y), mode)
        assert g.genome_correlation_last()["count"] == n
        del dx, dy, x, y
