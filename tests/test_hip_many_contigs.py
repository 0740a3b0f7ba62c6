"""GPU: an assembly of 300 sequences (tests/contig_cases.py) through every batched and genome-wide entry point the Python
face reaches, each compared per vector, bit for bit, with the CPU checker the suite already has for that operator
(oracle.cpu, or the tests/*_ref.py module).  No expected value comes from a HIP call.

What 300 vectors reach and 41 do not: ten 32-entry launch tables in one call -- cut by gdsp_batch_run and, each by its own
rule, by the piece kernel of segments, intervalstats, the anchor tables, the sampled-genome walk, the sliding FIR, peaks and
the workspace sizing of distance, fillgaps and localcorrelate -- with a vector shorter than the half window on either side
of every cut; percentile's tables of 32 sources and its 256 position strips.  Every call is made twice: on the assembly, and
on the assembly with zero-length vectors let in at index 0, 31, 32 and last and forty in a row, which must give the other
vectors the same bits and leave the empty ones' buffers (two guard words each) alone.  Outputs are filled with NaN before
a call, so a vector that a launch table lost shows.

On a vector shorter than the half window the reference reads out of bounds; DESIGN documents zero padding, which is
what oracle.cpu's loops do for every length (tests/test_contig_cases.py holds them to a numpy form of that meaning), so
cpu.smooth and its kin are the expected values at every length here.

The windows are 3, 101 and 1001 (above the longest short contig).  The operators whose results on real values are only
bounded -- localstats, localcorrelate -- take the integer depth, on which their checkers are exact; hann and fma `smooth`
keep the bound of tests/test_hip_parity.py (one rounding per operation), on the depth as well.

The image-level halves underneath the genome-wide calls (gdsp_xsum_accumulate_batch and its kin) get one call each too."""
import ctypes as C

import numpy as np
import pytest

import chain_model as cm
import contig_cases as cc
import correlate_ref
import distance_ref
import fillgaps_ref
import histogram_ref
import keepsegments_ref
import lagcorr_ref
import localmad_ref
import matrixover_ref
import percentilesover_ref
import profileover_ref
import prominence_ref
import segments_ref
import sliding_percentile_ref
import xsum_ref
from oracle import cpu
from test_hip_percentile_binarize import ROUTES

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
ROUTE_KEYS = sorted({k for env in ROUTES.values() for k in env})


@pytest.fixture(scope="module")
def gd():
    import genodsp_amd
    return genodsp_amd


@pytest.fixture(scope="module")
def asm():
    return cc.assembly(cc.MAIN, 0)


GUARD = cc.guard_words()


def up(gd, x):
    """a vector on the device; an empty one gets its guard words"""
    v = gd.DeviceVector.from_numpy(x)
    if v.n == 0:
        v.buf.upload(GUARD)
    return v


def down(v):
    return v.numpy() if v.n else v.buf.download(np.float64, 2)


def held(x):
    """what `down` must give for a vector the call only read, or an empty one"""
    return x if x.size else GUARD


class Case:
    """one call of a batched entry point: device(gd, ins, outs, origin) runs it -- outs is None for an operator that works
    in place, origin[j] the assembly's index of vector j (None: an empty one) -- and cpu(i) is the checker's vector i"""

    def __init__(self, name, source, device, cpu_fn, in_place=False):
        self.name, self.source, self.device, self.cpu, self.in_place = name, source, device, cpu_fn, in_place

    def run(self, gd, host, origin):
        ins = [up(gd, x) for x in host]
        outs = None if self.in_place else [up(gd, np.full(x.size, np.nan)) for x in host]
        self.device(gd, ins, outs, origin)
        gd.sync()
        if not self.in_place:
            cc.assert_same([down(v) for v in ins], [held(x) for x in host], self.name + ": the inputs")
        return [down(v) for v in (ins if self.in_place else outs)]


def cases(asm):
    sig, cnt, trk = asm.signals, asm.counts, asm.track
    out = []

    def add(name, source, device, cpu_fn, in_place=False):
        out.append(Case(name, source, device, cpu_fn, in_place))

    for W in cc.WINDOWS:
        add("smooth exact W=%d" % W, sig, lambda g, i, o, _, W=W: g.smooth_batch(i, W, outs=o), lambda i, W=W: cpu.smooth(sig[i], W))
        for want_max, fill in ((True, 0.0), (False, 9e99)):
            add("local_extrema N=%d max=%d" % (W, want_max), sig,
                lambda g, i, o, _, W=W, m=want_max, f=fill: g.local_extrema_batch(i, W, m, f, outs=o),
                lambda i, W=W, m=want_max, f=fill: cpu.local_extrema(sig[i], W, int(m), f))
            add("best_extrema W=%d max=%d" % (W + want_max, want_max), sig,
                lambda g, i, o, _, W=W + want_max, m=want_max: g.best_extrema_batch(i, W, m, outs=o),
                lambda i, W=W + want_max, m=want_max: cpu.best_extrema(sig[i], W, int(m)))
        add("sliding_percentile 50 W=%d" % W, sig, lambda g, i, o, _, W=W: g.sliding_percentile_batch(i, W, 50000, outs=o),
            lambda i, W=W: sliding_percentile_ref.sliding_percentile(sig[i], W, 50000))
        add("prominence W=%d" % W, sig, lambda g, i, o, _, W=W: g.prominence_batch(i, W, outs=o),
            lambda i, W=W: prominence_ref.prominence(sig[i], W)[0])
        what = {3: "zscore", 101: "mean", 1001: "stddev"}[W]
        add("localstats W=%d %s" % (W, what), cnt, lambda g, i, o, _, W=W, a=what: g.local_stats_batch(i, W, as_=a, outs=o),
            lambda i, W=W, a=what: cm.model_localstats(cnt[i], W, a))
        what = {3: "zscore", 101: "clean", 1001: "mad"}[W]
        add("localmad W=%d %s" % (W, what), sig, lambda g, i, o, _, W=W, a=what: g.local_mad_batch(i, W, as_=a, outs=o),
            lambda i, W=W, a=what: localmad_ref.figures(sig[i], W)[a])
        what = {3: "covariance", 101: "correlation", 1001: "slope"}[W]

        def localcorr(g, ys, _o, origin, W=W, a=what):
            xs = [up(g, cnt[k] if k is not None else np.empty(0)) for k in origin]
            g.local_correlation_batch(xs, ys, W, as_=a)
            g.sync()
            cc.assert_same([down(v) for v in xs], [held(cnt[k] if k is not None else np.empty(0)) for k in origin], "localcorrelate: x")
        add("localcorrelate W=%d %s" % (W, what), trk, localcorr, lambda i, W=W, a=what: cm.model_localcorrelate(cnt[i], trk[i], W, a),
            in_place=True)
        left, right = (W - 1) // 2, W - (W - 1) // 2                  # the driver's split of a length
        add("dilate %d" % W, sig, lambda g, i, o, _, l=left, r=right: g.dilate_batch(i, l, r, T=2.0, outs=o),
            lambda i, l=left, r=right: cpu.dilate(sig[i], l, r, T=2.0))
        add("erode %d" % W, sig, lambda g, i, o, _, l=left, r=right: g.erode_batch(i, l, r, T=0.5, one=2.0, zero=-1.0, outs=o),
            lambda i, l=left, r=right: cpu.erode(sig[i], l, r, T=0.5, one=2.0, zero=-1.0))
        add("dilate=erode=binarize %d" % W, sig,
            lambda g, i, o, _, l=left, r=right: g.dilate_erode_batch(i, l, r, l, r, d_T=2.0, binarize=(0.0, False, 3.0, -1.0), outs=o),
            lambda i, l=left, r=right: cpu.binarize(cpu.erode(cpu.dilate(sig[i], l, r, T=2.0), l, r), 0.0, False, 3.0, -1.0))
    add("sliding_percentile 90 W=101", sig, lambda g, i, o, _: g.sliding_percentile_batch(i, 101, 90000, outs=o),
        lambda i: sliding_percentile_ref.sliding_percentile(sig[i], 101, 90000))
    for want_max, fill in ((True, 0.0), (False, 1.7976931348623157e308)):
        add("smooth=localextremum max=%d" % want_max, sig,
            lambda g, i, o, _, m=want_max, f=fill: g.smooth_local_extrema_batch(i, 101, 11, m, f, outs=o),
            lambda i, m=want_max, f=fill: cpu.local_extrema(cpu.smooth(sig[i], 101), 11, int(m), f))
    for kw in ({}, {"T": 2.0, "to": "left", "signed": True, "cap": 50}, {"T": 1.0, "ties_above": True, "to": "right"}):
        add("distance %r" % kw, sig, lambda g, i, _o, _, kw=kw: g.distance_batch(i, **kw), lambda i, kw=kw: distance_ref.distance(sig[i], **kw),
            in_place=True)
    for kw in ({}, {"how": "nearest", "maxgap": 40}, {"known": "nonzero", "how": "left", "ends": "keep"}):
        add("fillgaps %r" % kw, sig, lambda g, i, _o, _, kw=kw: g.fill_gaps_batch(i, **kw), lambda i, kw=kw: fillgaps_ref.fill_gaps(sig[i], **kw),
            in_place=True)
    add("binarize", sig, lambda g, i, _o, _: g.binarize_batch(i, 2.0, True, 2.0, -1.0), lambda i: cpu.binarize(sig[i], 2.0, True, 2.0, -1.0), True)
    add("clip", sig, lambda g, i, _o, _: g.clip_batch(i, lo=1.0, hi=4.5), lambda i: cpu.clip(sig[i], lo=1.0, hi=4.5), True)
    add("erase", sig, lambda g, i, _o, _: g.erase_batch(i, lo=2.0, hi=20.0, keep_inside=True, zero=-1.0),
        lambda i: cpu.erase(sig[i], lo=2.0, hi=20.0, keep_inside=True, zero=-1.0), True)
    add("addconst", sig, lambda g, i, _o, _: g.add_constant_batch(i, 0.1), lambda i: cpu.add_constant(sig[i], 0.1), True)
    add("abs", sig, lambda g, i, _o, _: g.abs_batch(i), lambda i: cpu.abs_(sig[i]), True)
    add("multiplyconst", sig, lambda g, i, _o, _: g.multiply_constant(i, 0.1), lambda i: sig[i] * np.float64(0.1), True)
    add("divideconst", sig, lambda g, i, _o, _: g.divide_constant(i, 3.0), lambda i: sig[i] / np.float64(3.0), True)
    add("standardize", sig, lambda g, i, _o, _: g.standardize(i, 1.25, 0.3), lambda i: (sig[i] - np.float64(1.25)) / np.float64(0.3), True)
    return out


CASE_NAMES = [c.name for c in cases(cc.assembly(cc.MAIN, 0))]


@pytest.fixture(scope="module")
def case_table(asm):
    return {c.name: c for c in cases(asm)}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_vector_of_the_assembly_is_the_checkers(gd, asm, case_table, name):
    case = case_table[name]
    want = [np.ascontiguousarray(case.cpu(i), np.float64) for i in range(asm.K)]
    assert any(not np.array_equal(w, x) for w, x in zip(want, case.source)), "the operator changes nothing here"
    got = case.run(gd, case.source, list(range(asm.K)))
    cc.assert_same(got, want, name)
    host, origin = cc.with_empties(case.source)
    got = case.run(gd, host, origin)
    cc.assert_same(got, [want[k] if k is not None else GUARD for k in origin], name + " with empty vectors")


@pytest.mark.parametrize("mode", ["hann", "fma"])
def test_hann_and_fma_smooth_keep_their_bound_on_every_vector(gd, asm, mode):
    """not the reference's bits: one rounding per operation, W 2^-52 sum |w_k v_k| (tests/test_hip_parity.py), on the depth"""
    W, taps = 101, cpu.hann_window(101)
    m = {"hann": gd.FIR_HANN, "fma": gd.FIR_FMA}[mode]
    for host, origin in ((asm.counts, list(range(asm.K))), cc.with_empties(asm.counts)):
        ins = [up(gd, x) for x in host]
        outs = [up(gd, np.full(x.size, np.nan)) for x in host]
        gd.smooth_batch(ins, W, outs=outs, mode=m)
        gd.sync()
        for j, k in enumerate(origin):
            got = down(outs[j])
            if k is None:
                assert cc.first_difference([got], [GUARD]) is None, j
                continue
            x = asm.counts[k]
            bound = W * 2 * EPS * cpu.fir(np.abs(x), taps)
            assert np.all(np.abs(got - cpu.smooth(x, W)) <= bound), (mode, j, k, x.size)


# ------------------------------------------------------------------------------- the genome-wide calls ----

def both_layouts(gd, vectors):
    """the device vectors of the assembly and of its variant with empty vectors, each with the index map old -> new"""
    plain = ([up(gd, x) for x in vectors], list(range(len(vectors))))
    host, origin = cc.with_empties(vectors)
    where = [None] * len(vectors)
    for j, k in enumerate(origin):
        if k is not None:
            where[k] = j
    return plain, ([up(gd, x) for x in host], where)


def same_figures(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert xsum_ref.same(g, w), (what, k, g, w)


def test_genome_stats_minmax_and_histogram(gd, asm):
    sig = asm.signals
    edges = histogram_ref.uniform_edges(-40.0, 0.5, 160)
    for window in (1, 3):
        want = xsum_ref.genome(sig, window)
        words = histogram_ref.words(sig, edges, window)
        for vecs, _ in both_layouts(gd, sig):
            got = gd.genome_stats(vecs, window=window)
            same_figures([got[k] for k in ("count", "sum", "mean", "variance", "stddev")], want, ("stats", window, len(vecs)))
            counts, below, above, n = gd.genome_histogram(vecs, lo=-40.0, width=0.5, bins=160, window=window)
            assert np.array_equal(counts, words[:160]) and (below, above, n) == tuple(int(x) for x in words[160:]), (window, len(vecs))
            lo, hi, count = gd.genome_minmax(vecs, window=window)
            smp = np.concatenate([xsum_ref.sample(x, window) for x in sig])
            assert (lo, hi, count) == (float(smp.min()), float(smp.max()), smp.size), (window, len(vecs))
    assert (float(min(x.min() for x in sig)), float(max(x.max() for x in sig))) == cpu.genome_minmax(sig)


def test_genome_correlation_and_lag_correlation(gd, asm):
    pairs = list(zip(asm.signals, asm.track))
    want = correlate_ref.genome(pairs)
    fig, counts, cov, corr = lagcorr_ref.curve(pairs, -20, 41)
    (xs, _), (xs2, _) = both_layouts(gd, asm.signals)
    (ys, _), (ys2, _) = both_layouts(gd, asm.track)
    for a, b in ((xs, ys), (xs2, ys2)):
        got = gd.genome_correlation(list(zip(a, b)))
        same_figures([got[k] for k in correlate_ref.FIGURES], want, ("correlate", len(a)))
        got = gd.genome_lag_correlation(list(zip(a, b)), -20, 41)
        same_figures([got[k] for k in lagcorr_ref.FIGURES], fig, ("crosscorrelate", len(a)))
        assert [int(x) for x in got["pairs"]] == [int(x) for x in counts]
        same_figures(got["covariances"], cov, "covariance per lag")
        same_figures(got["correlations"], corr, "correlation per lag")


def moved(rows, where):
    out = np.array(rows, np.int64).copy()
    out[:, 0] = [where[k] for k in out[:, 0].tolist()]
    return out


def test_genome_profile_and_matrix(gd, asm):
    sig, anchors = asm.signals, cc.anchors(asm)
    for off_lo, noffsets, bin in ((-50, 101, 1), (-1001, 2002, 2)):
        want = profileover_ref.profile(sig, anchors, off_lo, noffsets, bin)
        cells = matrixover_ref.figures(sig, anchors, off_lo, noffsets, bin) if noffsets == 101 else None
        for vecs, where in both_layouts(gd, sig):
            got = gd.genome_profile(vecs, moved(anchors, where), off_lo, noffsets, bin)
            assert [int(x) for x in got["count"]] == [int(f[0]) for f in want]
            for col, name in ((1, "sum"), (2, "mean"), (3, "variance"), (4, "stddev")):
                same_figures(got[name], [f[col] for f in want], (name, off_lo, len(vecs)))
            if cells is not None:
                for what in matrixover_ref.FIGURES:
                    rows = gd.genome_matrix(vecs, moved(anchors, where), off_lo, noffsets, bin, what=what)
                    assert matrixover_ref.same_bits(rows, cells[what]), (what, len(vecs))


def test_segments_and_keepsegments(gd, asm):
    sig = asm.signals
    for T, kw in ((2.0, {}), (1.0, {"ties_above": True, "merge_gap": 3, "min_length": 2}), (0.0, {"min_height": 4.0})):
        want = segments_ref.genome(sig, T, **kw)
        assert len({w[0] for w in want}) > 100
        for vecs, where in both_layouts(gd, sig):
            back = {j: k for k, j in enumerate(where)}
            got = gd.segments(vecs, T, **kw)
            got["vec"] = np.array([back[int(j)] for j in got["vec"]], np.uint32)
            segments_ref.same_table(got, want)
            for mode in ("one", "max"):
                outs = [up(gd, np.full(v.n, np.nan)) for v in vecs]
                gd.keep_segments(vecs, outs, T, as_=mode, one=2.0, zero=-1.0, **kw)
                painted = [keepsegments_ref.paint(x, segments_ref.segments(x, T, **kw), mode, 2.0, -1.0) for x in sig]
                cc.assert_same([down(outs[where[k]]) for k in range(asm.K)], painted, "keepsegments %s" % mode)
                cc.assert_same([down(o) for o in outs if o.n == 0], [GUARD] * sum(o.n == 0 for o in outs), "keepsegments: empty vectors")


def test_interval_stats_and_percentiles(gd, asm):
    sig = asm.signals
    vec, start, end = cc.intervals(asm)
    ps = [0, 25000, 50000, 99500, 100000]
    want = [segments_ref.figures(sig[v], np.ones(sig[v].size, bool), s, e) for v, s, e in zip(vec.tolist(), start.tolist(), end.tolist())]
    pct = [percentilesover_ref.interval_percentiles(sig[v], [s], [e], ps) for v, s, e in zip(vec.tolist(), start.tolist(), end.tolist())]
    for vecs, where in both_layouts(gd, sig):
        which = np.array([where[v] for v in vec.tolist()])
        got = gd.interval_stats(vecs, start, end, vec=which)
        for i, w in enumerate(want):
            assert (int(got["count"][i]), int(got["maxpos"][i])) == (w[0], w[5]), (i, vec[i], start[i], end[i])
            same_figures([got[k][i] for k in ("sum", "mean", "min", "max")], w[1:5], ("statsover", i))
        got = gd.interval_percentiles(vecs, start, end, ps, vec=which)
        for i, (count, values) in enumerate(pct):
            assert int(got["count"][i]) == int(count[0])
            same_figures(got["values"][i], values[0], ("percentilesover", i))


def same_images(a, b):
    """word for word but for the flush count and the spare word (tests/test_profileover.py)"""
    return np.array_equal(np.delete(a, [70, 71], axis=-1), np.delete(b, [70, 71], axis=-1))


def test_the_image_level_halves_over_ten_tables(gd, asm):
    """the batched calls underneath the genome-wide ones, each on its own: gdsp_xsum_accumulate(_sq)_batch,
    gdsp_xsum_pair_accumulate(_dev)_batch, gdsp_lag_products_batch, gdsp_profile_accumulate_batch, gdsp_matrix_rows_batch,
    gdsp_histogram_accumulate_batch, gdsp_run_pieces_batch and gdsp_paint_spans_batch, against the checkers' images"""
    sig, trk = asm.signals, asm.track
    host_pairs = list(zip(sig, trk))
    x, y = np.concatenate(sig), np.concatenate(trk)
    fig = dict(zip(correlate_ref.FIGURES, correlate_ref.genome(host_pairs)))
    means = (fig["meanx"], fig["meany"])
    d = x - np.float64(means[0])
    anchors = cc.anchors(asm)
    edges = histogram_ref.uniform_edges(-40.0, 0.5, 160)
    cells = matrixover_ref.matrix(sig, anchors, -50, 100, 4, "sum")
    segs = segments_ref.genome(sig, 1.0, merge_gap=2)
    spans = [(w[0], w[1], w[2], float(w[3])) for w in segments_ref.genome(sig, 2.0)]
    painted = [np.full(v.size, -1.0) for v in sig]
    for k, s, e, value in spans:
        painted[k][s:e] = value
    for (xs, where), (ys, _) in zip(both_layouts(gd, sig), both_layouts(gd, trk)):
        back = {j: k for k, j in enumerate(where)}
        for got, want in ((gd.xsum_image(xs), xsum_ref.image(x)), (gd.xsum_image(xs, mean=means[0]), xsum_ref.image(d * d))):
            assert np.array_equal(np.delete(got, [69, 70, 71]), np.delete(want, [69, 70, 71]))       # (as tests/test_genome_stats.py)
        pairs = list(zip(xs, ys))
        assert same_images(gd.xsum_pair_image(pairs), correlate_ref.images(x, y))
        assert same_images(gd.xsum_pair_image(pairs, means=means), correlate_ref.images(x, y, means))
        assert same_images(gd.lag_products(pairs, -20, 41, *means), lagcorr_ref.images(host_pairs, -20, 41, *means))
        there = moved(anchors, where)
        assert same_images(gd.profile_images(xs, there, -50, 101), profileover_ref.images(sig, anchors, -50, 101))
        rows, todo = gd.matrix_rows(xs, there, -50, 100, bin=4, what="sum")
        keep = np.ones(rows.size, bool)
        keep[todo] = False
        assert keep.any() and matrixover_ref.same_bits(rows.ravel()[keep], cells.ravel()[keep])
        assert np.array_equal(gd.histogram_words(xs, edges, uniform=True), histogram_ref.words(sig, edges))
        table, _ = gd.segments_from_pieces(gd.run_pieces(xs, 1.0), merge_gap=2)
        table["vec"] = np.array([back[int(j)] for j in table["vec"]], np.uint32)
        segments_ref.same_table(table, segs)
        outs = [up(gd, np.full(v.n, np.nan)) for v in xs]
        gd.paint_spans(None, outs, [(where[k], s, e, value) for k, s, e, value in spans], outside=-1.0)
        cc.assert_same([down(outs[where[k]]) for k in range(asm.K)], painted, "paint_spans")
        cc.assert_same([down(o) for o in outs if o.n == 0], [GUARD] * sum(o.n == 0 for o in outs), "paint_spans: empty vectors")


def test_an_interval_past_a_contigs_end_is_refused(gd, asm):
    """start < end <= n or GDSP_EINVAL (include/genodsp_hip.h), also for a vector of a later table than the first"""
    vecs = [up(gd, x) for x in asm.signals]
    v, s, e = cc.past_the_end(asm)
    assert v > cc.TABLE and s < asm.lengths[v] < e
    with pytest.raises(gd.GdspError):
        gd.interval_stats(vecs, [0, s], [1, e], vec=[0, v])
    with pytest.raises(gd.GdspError):
        gd.interval_percentiles(vecs, [0, s], [1, e], [50000], vec=[0, v])


# ------------------------------------------------------------------------------------------- percentile ----

def set_route(monkeypatch, route):
    for k in ROUTE_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)


def check_percentile(gd, host, vecs, window, what, outs=None):
    """percentile and the fused percentile = binarize over `vecs` (the host vectors `host`) against cpu.percentile and
    cpu.binarize, every source's output; brackets forced at this size by a small sample target"""
    pts = [50000, 99000]
    wcnt, wvals = cpu.percentile([x for x in host if x.size], pts, window)
    cnt, vals = gd.percentile(vecs, pts, window=window, strategy=gd.SELECT_BRACKET, sample_target=300)
    assert gd.percentile_stats()["population"] == wcnt and gd.percentile_stats()["route"] == gd.SELECT_BRACKET, (what, gd.percentile_stats())
    assert cnt == wcnt and cc.first_difference([np.array(vals)], [wvals]) is None, (what, vals, wvals)
    outs = outs if outs is not None else [up(gd, np.full(x.size, np.nan)) for x in host]
    cnt, vals, outs, _ = gd.percentile_binarize(vecs, pts, which=1, outs=outs, one=2.0, zero=-1.0, window=window,
                                               strategy=gd.SELECT_BRACKET, sample_target=300)
    assert gd.percentile_stats()["population"] == wcnt, (what, gd.percentile_stats())
    assert cnt == wcnt and cc.first_difference([np.array(vals)], [wvals]) is None, (what, vals, wvals)
    gd.sync()
    cc.assert_same([down(o) for o in outs], [cpu.binarize(x, wvals[1], False, 2.0, -1.0) if x.size else GUARD for x in host], what)
    cc.assert_same([down(v) for v in vecs], [held(x) for x in host], what + ": the sources")


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_percentile_of_300_sources_on_every_route(gd, asm, monkeypatch, route):
    """ten tables of PC_TAB sources per sample, counting and fix-up launch; sources 257 to 300 have no position strip and
    are binarized by a pass of their own"""
    set_route(monkeypatch, route)
    for host, _ in ((asm.signals, None), cc.with_empties(asm.signals)):
        for window in (1, 3):
            check_percentile(gd, host, [up(gd, x) for x in host], window, "%s window %d of %d" % (route, window, len(host)))


class Odd:
    """a vector 8 bytes off a 16-byte boundary, for the entry points that take any source the face can name"""

    def __init__(self, gd, x):
        self.n = x.size
        self.buf = gd.DeviceBuffer((x.size + 4) * 8)
        self.buf.upload(np.ascontiguousarray(x, np.float64), 8)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.ptr + 8)

    def numpy(self):
        return self.buf.download(np.float64, self.n, 8)


def test_percentile_of_sources_of_three_flavours_in_one_call(gd, asm, monkeypatch):
    """aligned sources with a strip (fused), aligned ones past the 256th strip or with a misaligned output (dense), and
    sources 8 bytes off a 16-byte boundary (strided), mixed so that every launch table of a flavour is cut more than once.
    percentile and percentile_binarize read `ptr` and `n` of what they are given, so a misaligned source is a buffer's
    address + 8 (the DeviceVector class itself asserts 16-byte offsets)."""
    set_route(monkeypatch, "resident")
    host = asm.signals + asm.signals[:100]                # 400 sources: more than 256 with a strip AND tables of the other two
    odd_in = {k for k in range(len(host)) if k % 5 == 2} | {31, 32, 255, 256, 299}
    odd_out = {k for k in range(len(host)) if k % 7 == 3}
    assert len(odd_in) > 2 * cc.TABLE and len(odd_out - odd_in) > cc.TABLE and len(host) - len(odd_in | odd_out) > 256 + 8
    vecs = [Odd(gd, x) if k in odd_in else up(gd, x) for k, x in enumerate(host)]
    outs = [Odd(gd, np.full(x.size, np.nan)) if k in odd_out else up(gd, np.full(x.size, np.nan)) for k, x in enumerate(host)]
    check_percentile(gd, host, vecs, 1, "three flavours", outs=outs)


# ------------------------------------------------------------------------------- the boundary values of K ----

@pytest.mark.parametrize("K", cc.BOUNDARY)
def test_exactly_a_table_and_one_more(gd, monkeypatch, K):
    """K = 32, 33, 64, 65, 256, 257: gdsp_batch_run through its cheapest user, the hand-rolled chunkers of segments,
    interval_stats, genome_stats and genome_profile, and percentile's tables"""
    set_route(monkeypatch, "resident")
    a = cc.assembly(K, K)
    sig = a.signals
    vecs = [up(gd, x) for x in sig]
    gd.binarize_batch(vecs, 2.0, True, 2.0, -1.0)
    cc.assert_same([down(v) for v in vecs], [cpu.binarize(x, 2.0, True, 2.0, -1.0) for x in sig], "binarize")
    vecs = [up(gd, x) for x in sig]
    segments_ref.same_table(gd.segments(vecs, 1.0, merge_gap=2), segments_ref.genome(sig, 1.0, merge_gap=2))
    vec, start, end = cc.intervals(a)
    got = gd.interval_stats(vecs, start, end, vec=vec)
    for i, (v, s, e) in enumerate(zip(vec.tolist(), start.tolist(), end.tolist())):
        w = segments_ref.figures(sig[v], np.ones(sig[v].size, bool), s, e)
        assert (int(got["count"][i]), int(got["maxpos"][i])) == (w[0], w[5]), (i, v, s, e)
        same_figures([got[k][i] for k in ("sum", "mean", "min", "max")], w[1:5], ("statsover", i))
    got = gd.genome_stats(vecs)
    same_figures([got[k] for k in ("count", "sum", "mean", "variance", "stddev")], xsum_ref.genome(sig), "stats")
    anchors = cc.anchors(a)
    want = profileover_ref.profile(sig, anchors, -60, 121, 1)
    got = gd.genome_profile(vecs, anchors, -60, 121, 1)
    assert [int(x) for x in got["count"]] == [int(f[0]) for f in want]
    for col, name in ((1, "sum"), (2, "mean"), (3, "variance"), (4, "stddev")):
        same_figures(got[name], [f[col] for f in want], name)
    for window in (1, 3):
        check_percentile(gd, sig, vecs, window, "K=%d window %d" % (K, window))
