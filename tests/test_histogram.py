"""histogram (not in the reference) through the library: gdsp_histogram_* and gdsp_genome_histogram of
include/genodsp_hip.h against the checker tests/histogram_ref.py.  The result is integer counts, so every comparison is
equality of integers: the uniform table against a Fraction fma (no GPU), then the device pass on hot bins, values on
and next to every edge, non-finite values, windows, cuts and alignments, with the uniform hint on and off."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import histogram_ref as href
import xsum_ref
from conftest import ROOT

DBL_MAX = xsum_ref.DBL_MAX
TINY = 5e-324
BINS = [1, 2, 255, 256, 1024, 4096, 65536]


def gd():
    import genodsp_amd
    return genodsp_amd


def triples():
    """(lo, width, B): plain ones, widths that are not dyadic, large and negative lo, tiny and huge widths"""
    rng = np.random.default_rng(17)
    out = [(0.0, 1.0, 256), (0.0, 0.1, 1000), (0.1, 0.1, 100), (-3.7, 0.3, 4096), (1e15, 0.25, 1024), (1e15, 0.3, 64),
           (-1e9, 1e-3, 65536), (0.0, 1e-320, 10), (-DBL_MAX, DBL_MAX / 4, 7), (2.0 ** 52, 1.0, 65536), (-0.5, 1.0 / 3, 3),
           (1e-300, 1e-301, 999), (0.0, 1.0, 1), (123456.789, 0.01, 65536)]
    for _ in range(300):
        lo = float(rng.standard_normal() * 10.0 ** int(rng.integers(-3, 12)))
        width = float(abs(rng.standard_normal()) * 10.0 ** int(rng.integers(-4, 6)) + 1e-9)
        if rng.random() < 0.3:
            width = float(round(width, 1) or 0.1)                       # 0.1-type widths
        out.append((lo, width, int(rng.integers(1, 3000))))
    return out


def adversarial(edges, rng, n_extra=2000):
    """every edge and one ulp to either side, signed zeros, denormals, the largest doubles, NaN and the infinities"""
    e = np.asarray(edges, np.float64)
    special = np.array([0.0, -0.0, TINY, -TINY, 2.0 ** -1022, -2.0 ** -1022, DBL_MAX, -DBL_MAX, np.nan, np.inf, -np.inf])
    with np.errstate(all="ignore"):                                     # (a step beyond DBL_MAX is an infinity: never sampled)
        near = np.concatenate([e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf)])
        span = float(min(e[-1] - e[0], DBL_MAX / 4))
        inside = e[0] + rng.random(n_extra) * span
        x = np.concatenate([near, np.tile(special, 20), inside, inside - span, inside + span])
    rng.shuffle(x)
    return x


def some_tables():
    rng = np.random.default_rng(23)
    tables = [href.uniform_edges(0, 1, 256), href.uniform_edges(-5.5, 0.1, 110), href.uniform_edges(-3, 1, 6),
              np.array([-DBL_MAX, -1.0, -TINY, 0.0, TINY, 1.0, DBL_MAX]), np.array([0.0, 1.0]),
              np.unique(rng.standard_normal(700) * 30), np.cumsum(np.exp(rng.standard_normal(2000))) - 50.0,
              np.concatenate([[-1e300], np.arange(0.0, 50.0), [1e300]])]
    return tables


# ------------------------------------------------------------------------------------------------ CPU ----

def test_uniform_edges_are_the_fraction_fma():
    g = gd()
    seen = 0
    for lo, width, bins in triples():
        want = href.uniform_edges(lo, width, bins)
        if not href.table_ok(want):
            with pytest.raises(ValueError):
                g.histogram_uniform_edges(lo, width, bins)
            continue
        got = g.histogram_uniform_edges(lo, width, bins)
        assert got.tobytes() == want.tobytes(), (lo, width, bins)
        seen += 1
    assert seen >= 250


@pytest.mark.parametrize("lo,width,bins", [(0.0, 0.0, 4), (0.0, -1.0, 4), (1e17, 1.0, 8), (1e308, 1e308, 4), (math.nan, 1.0, 4),
                                           (0.0, math.inf, 2), (math.inf, 1.0, 2), (0.0, math.nan, 3), (0.0, 1e-330, 5)])
def test_uniform_edges_refuses(lo, width, bins):
    if math.isfinite(lo) and math.isfinite(width):
        assert not href.table_ok(href.uniform_edges(lo, width, bins))
    with pytest.raises(ValueError):
        gd().histogram_uniform_edges(lo, width, bins)
    e = np.zeros(bins + 1)
    assert gd().lib().gdsp_histogram_uniform_edges(lo, width, bins, e.ctypes.data) != 0


def test_wrapper_rejects_bad_shapes():
    g = gd()
    for bins in (0, -1, 65537):
        with pytest.raises(ValueError):
            g.histogram_uniform_edges(0.0, 1.0, bins)
        with pytest.raises(ValueError):
            g.genome_histogram([], bins=bins)
    for edges in ([1.0], [], [[0.0, 1.0], [2.0, 3.0]], [0.0, 0.0, 1.0], [2.0, 1.0], [0.0, math.nan], [0.0, math.inf],
                  np.arange(65538.0)):
        with pytest.raises(ValueError):
            g.genome_histogram([], edges=edges)
    with pytest.raises(ValueError):
        g.genome_histogram([], lo=0.0, width=0.0, bins=4)


def test_checker_is_self_consistent():
    rng = np.random.default_rng(5)
    for e in some_tables():
        x = adversarial(e, rng)
        for window, lo, hi in ((1, -DBL_MAX, DBL_MAX), (3, -1.0, 40.0), (7, 0.0, DBL_MAX)):
            w = href.words([x], e, window, lo, hi, [5])
            B = e.size - 1
            assert int(w[:B].sum()) + int(w[B]) + int(w[B + 1]) == int(w[B + 2])
            assert int(w[B + 2]) == xsum_ref.sample(x, window, lo, hi, 5).size
        w = href.words([e[:-1]], e)                                     # an edge belongs to the bin it opens
        assert w[:e.size - 1].tolist() == [1] * (e.size - 1) and w[e.size - 1] == 0 and w[e.size] == 0
        w = href.words([e[-1:], np.array([-0.0])], np.array([0.0, 1.0]))
        assert int(w[0]) == 1                                           # -0.0 falls where +0.0 falls
    assert href.words([], np.array([0.0, 1.0])).tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ GPU ----

def dev():
    g = gd()
    g.set_device(0)
    return g


def as_tuple(w):
    B = w.size - 3
    return w[:B], int(w[B]), int(w[B + 1]), int(w[B + 2])


def check(g, xs, edges, window=1, lo=-DBL_MAX, hi=DBL_MAX, vecs=None, firsts=None, what=None):
    """the words of xs over `edges`, with the hint on and off, against the checker"""
    want = href.words(xs, edges, window, lo, hi, firsts)
    vecs = vecs if vecs is not None else [g.DeviceVector.from_numpy(x) for x in xs]
    B = len(edges) - 1
    for hint in (True, False):
        counts, below, above, n = g.genome_histogram(vecs, edges=edges, window=window, min=lo, max=hi, uniform=hint)
        assert (below, above, n) == (int(want[B]), int(want[B + 1]), int(want[B + 2])), (what, hint)
        assert np.array_equal(counts, want[:B]), (what, hint, np.flatnonzero(counts != want[:B])[:5])
        assert int(counts.sum()) + below + above == n
    return want


_hot = {}


def hot(g, value):
    """2^24 + 77 copies of one value, on the device (kept for the module)"""
    key = repr(float(value))                                            # (-0.0 and 0.0 are different signals)
    if key not in _hot:
        x = np.full((1 << 24) + 77, value)
        _hot[key] = (x, g.DeviceVector.from_numpy(x))
    return _hot[key]


@pytest.mark.gpu
@pytest.mark.parametrize("bins", BINS)
def test_hot_bins(bins):
    """all zeros, and all one value: every lane of every wave aims at one counter"""
    g = dev()
    for value, lo, width in ((0.0, 0.0, 1.0), (7.0, 0.0, 1.0), (-0.0, -3.0, 0.5), (7.0, 8.0, 1.0), (7.0, -100000.0, 1.0)):
        x, v = hot(g, value)
        e = href.uniform_edges(lo, width, bins)
        want = check(g, [x], e, vecs=[v], what=(value, lo, width))
        assert int(want.max()) == x.size
    x, v = hot(g, 7.0)
    assert v.numpy().tobytes() == x.tobytes()                           # the signal is only read


@pytest.mark.gpu
@pytest.mark.parametrize("bins", BINS)
def test_depth_and_real_signals(bins):
    g = dev()
    rng = np.random.default_rng(bins)
    d = g.synth_coverage(20240611, 3, 1000, 3000001, 0)                 # piecewise-constant integer depth
    x = d.numpy()
    check(g, [x], href.uniform_edges(0, 1, bins), vecs=[d], what="depth")
    check(g, [x], href.uniform_edges(1, 2, bins), vecs=[d], what="depth, lo=1 width=2")
    assert d.numpy().tobytes() == x.tobytes()
    r = g.synth_coverage(20240611, 3, 1000, 1000003, 1)                 # real-valued coverage
    y = r.numpy()
    width = float((y.max() - y.min()) / bins * 0.9)
    check(g, [y], href.uniform_edges(float(y.min()) + width, width, bins), vecs=[r], what="real")
    z = rng.standard_normal(500001) * 10
    check(g, [z], href.uniform_edges(-bins / 20, 0.1, bins), what="normal, 0.1-wide bins")
    check(g, [z], href.uniform_edges(-0.5 * bins, 1.0, bins), what="normal, unit bins")


@pytest.mark.gpu
@pytest.mark.parametrize("bins", BINS)
def test_values_on_and_next_to_every_edge(bins):
    g = dev()
    rng = np.random.default_rng(100 + bins)
    for lo, width in ((0.0, 1.0), (-7.3, 0.1), (1e15, 0.25), (-1e-300, 1e-303), (-DBL_MAX, DBL_MAX / 40000)):
        e = href.uniform_edges(lo, width, bins)
        assert href.table_ok(e)
        assert gd().histogram_uniform_edges(lo, width, bins).tobytes() == e.tobytes()
        check(g, [adversarial(e, rng)], e, what=(lo, width))


@pytest.mark.gpu
def test_tables_that_are_not_uniform():
    """searched, and with a hint that is wrong: the comparisons against the table decide"""
    g = dev()
    rng = np.random.default_rng(31)
    for i, e in enumerate(some_tables()):
        x = np.concatenate([adversarial(e, rng), rng.standard_normal(100000) * 30, rng.integers(0, 60, 100000).astype(np.float64)])
        check(g, [x], e, what=("table", i))
    e = np.sort(np.concatenate([np.unique(rng.standard_normal(65000)), [1e6, 2e6, 3e6]]))     # 65 000 bins near 0, 3 far away
    check(g, [np.concatenate([adversarial(e, rng, 500), rng.standard_normal(200000) * 2, rng.random(5000) * 3e6])], e, what="lopsided")


@pytest.mark.gpu
@pytest.mark.parametrize("window", [1, 3, 7, 1000])
def test_window_first_and_range(window):
    g = dev()
    rng = np.random.default_rng(window)
    xs = [rng.integers(0, 40, n).astype(np.float64) for n in (100003, 77, 4096 * 3 + 1, 20000)]
    xs[1][::5] = np.nan
    firsts = [0, 12345, 7, 999999]
    vs = [g.DeviceVector.from_numpy(x) for x in xs]
    vecs = [(v, 0, v.n, f) for v, f in zip(vs, firsts)]
    e = href.uniform_edges(0, 1, 32)
    check(g, xs, e, window=window, vecs=vecs, firsts=firsts, what="window")
    check(g, xs, e, window=window, lo=1.0, hi=30.5, vecs=vecs, firsts=firsts, what="window, min and max")
    check(g, xs, e, window=window, lo=50.0, vecs=vecs, firsts=firsts, what="an empty sample")
    e = np.array([-1.0, 2.5, 2.75, 17.0, 39.0])
    check(g, xs, e, window=window, lo=0.5, vecs=vecs, firsts=firsts, what="searched")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4097])
def test_short_vectors_and_odd_alignments(n):
    g = dev()
    rng = np.random.default_rng(n)
    e = href.uniform_edges(-2, 0.5, 16)
    x = rng.standard_normal(n + 8) * 3
    v = g.DeviceVector.from_numpy(x)
    check(g, [x[:n]], e, vecs=[(v, 0, n)], what="aligned")
    for start in (1, 3, 4, 7):                                          # 8-byte aligned sources that are not 16-byte aligned
        check(g, [x[start:start + n]], e, vecs=[(v, start, n, 0)], what=("start", start))
        check(g, [x[start:start + n]], e, window=3, vecs=[(v, start, n, 100 + start)], firsts=[100 + start], what=("start, window", start))
    assert v.numpy().tobytes() == x.tobytes()
    assert g.genome_histogram([])[3] == 0 and g.genome_histogram([], bins=5)[0].tolist() == [0] * 5


@pytest.mark.gpu
def test_a_batch_of_forty_sources_and_other_cuts():
    """40 vectors (two tables of sources); then one genome cut in different ways, piece by piece into one set of words"""
    g = dev()
    rng = np.random.default_rng(41)
    xs = [rng.integers(0, 300, int(rng.integers(1, 30000))).astype(np.float64) for _ in range(40)]
    xs[7] = rng.standard_normal(20011) * 50
    e = href.uniform_edges(0, 1, 256)
    check(g, xs, e, what="forty")
    x = np.concatenate(xs)
    v = g.DeviceVector.from_numpy(x)
    whole = g.histogram_words([v], e, uniform=True)
    assert np.array_equal(whole, href.words([x], e))
    for pieces in (3, 45):
        cuts = [0] + sorted(set(int(c) for c in rng.integers(1, x.size - 1, pieces))) + [x.size]
        parts = [(v, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(g.histogram_words(parts, e, uniform=True), whole)
        assert np.array_equal(g.histogram_words(parts, e, uniform=False), whole)
        assert np.array_equal(g.histogram_words(parts, e, window=7), href.words([x], e, 7))      # (first defaults to start)
        acc = g.DeviceBuffer((e.size + 2) * 8)                          # one call per piece into one set of words
        g.call("gdsp_histogram_init", acc.ptr, e.size - 1, None)
        g.sync(None)
        for p in parts:
            g.histogram_accumulate([p], acc, e, uniform=bool(p[1] % 2))
        assert np.array_equal(acc.download(np.uint64, e.size + 2), whole)
    assert v.numpy().tobytes() == x.tobytes()


@pytest.mark.gpu
def test_a_whole_chromosome():
    """chr1, 248,956,422 bases of synthetic read depth"""
    g = dev()
    n = 248956422
    d = g.synth_coverage(20240611, 0, 0, n, 0)
    x = d.numpy()
    e = href.uniform_edges(0, 1, 256)
    want = href.words([x], e)
    del x
    for hint in (True, False):
        counts, below, above, total = g.genome_histogram([d], edges=e, uniform=hint)
        assert total == n and (below, above) == (int(want[256]), int(want[257]))
        assert np.array_equal(counts, want[:256])
    e = href.uniform_edges(0, 1, 65536)
    counts, below, above, total = g.genome_histogram([d], edges=e, uniform=True)
    assert total == n and np.array_equal(counts[:256], want[:256]) and int(counts[256:].sum()) + above == int(want[257])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


RANK_SCRIPT = r'''
import os, sys, json
import numpy as np
import torch
import torch.distributed as dist
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import genodsp_amd as g
import histogram_ref as href
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
g.set_device(0)
rng = np.random.default_rng(4)
xs = [rng.integers(0, 90, n).astype(np.float64) for n in (50000, 70001, 3, 9000)] + [rng.standard_normal(20000) * 40]
mine = [g.DeviceVector.from_numpy(x) for i, x in enumerate(xs) if i % world == rank]
def allreduce(arr, op):
    assert op == "sum"
    t = torch.from_numpy(arr.view(np.int64).copy())
    dist.all_reduce(t)
    return t.numpy().view(np.uint64)
counts, below, above, n = g.genome_histogram(mine, lo=0.0, width=1.0, bins=64, window=3, allreduce=allreduce)
want = href.words(xs, href.uniform_edges(0, 1, 64), 3)
got = [int(c) for c in counts] + [below, above, n]
with open(os.path.join(sys.argv[2], "rank%d.json" % rank), "w") as f:
    json.dump({"rank": rank, "ok": got == [int(w) for w in want], "got": got}, f)
dist.destroy_process_group()
'''


@pytest.mark.gpu
def test_the_reduction_hook_over_two_ranks(tmp_path):
    """two processes on the one GPU, each with some of the chromosomes, their words summed by gloo"""
    script = tmp_path / "ranks.py"
    script.write_text(RANK_SCRIPT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), str(script), ROOT, str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.load(open(tmp_path / ("rank%d.json" % r))) for r in (0, 1)]
    assert all(l["ok"] for l in lines), lines
    assert lines[0]["got"] == lines[1]["got"]
