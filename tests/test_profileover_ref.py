"""The checker of profileover (tests/profileover_ref.py) held to a literal double loop over (anchor, offset) with
fractions.Fraction, and shown to tell the definition from three near misses.  No GPU."""
import math
import os
import random
from fractions import Fraction

import numpy as np

import profileover_ref as pref
import xsum_ref as ref
from conftest import ROOT


def small_cases():
    """120 small genomes of one to three chromosomes of 1 .. 30 bases with anchors on both strands (first and last base
    among them, some twice), an offset range that leaves most chromosomes, and a bin that divides it"""
    rnd = random.Random(41)
    out = []
    for i in range(120):
        vectors = []
        for _ in range(1 + i % 3):
            n = 1 if i < 3 else rnd.randint(1, 30)
            kind = i % 4
            if kind == 0:
                x = [rnd.gauss(0, 10) for _ in range(n)]
            elif kind == 1:
                x = [float(rnd.randint(0, 60)) for _ in range(n)]
            elif kind == 2:
                x = [math.ldexp(rnd.gauss(0, 1), rnd.randint(-300, 300)) for _ in range(n)]
            else:
                x = [rnd.choice([math.nan, math.inf, -math.inf]) if rnd.random() < 0.15 else rnd.gauss(1e6, 1e-3) for _ in range(n)]
            vectors.append(np.array(x, np.float64))
        anchors = []
        for c, v in enumerate(vectors):
            anchors += [(c, 0, 1), (c, v.size - 1, -1)]
            for _ in range(rnd.randint(0, 6)):
                anchors.append((c, rnd.randrange(v.size), rnd.choice([1, -1])))
        anchors.append(anchors[-1])
        rnd.shuffle(anchors)
        bin = rnd.choice([1, 1, 2, 3, 4])
        noffsets = bin * rnd.randint(1, 5)
        off_lo = rnd.randint(-8, 4)
        lo, hi = (-DBL_MAX, DBL_MAX) if i % 5 else (-5.0, 1e6)
        out.append((vectors, anchors, off_lo, noffsets, bin, lo, hi))
    return out


DBL_MAX = ref.DBL_MAX


def rounded(fr):
    """a Fraction rounded once (Fraction.__float__ is a correctly rounded int / int), +-inf beyond DBL_MAX"""
    try:
        return float(fr)
    except OverflowError:
        return math.inf if fr > 0 else -math.inf


def literal(vectors, anchors, off_lo, noffsets, bin, lo, hi):
    """the definition, pair by pair"""
    cols = [[] for _ in range(noffsets // bin)]
    for c, p, s in anchors:
        v = vectors[c]
        for k in range(off_lo, off_lo + noffsets):
            g = p + s * k
            if not 0 <= g < len(v):
                continue
            x = float(v[g])
            if math.isnan(x) or math.isinf(x) or x < lo or x > hi:
                continue
            cols[(k - off_lo) // bin].append(x)
    out = []
    for xs in cols:
        n = len(xs)
        total = sum((Fraction(x) for x in xs), Fraction(0))
        if n == 0:
            out.append((0.0, 0.0, math.nan, math.nan, math.nan, math.nan))
            continue
        mean = rounded(total / n)
        qs = []
        for x in xs:
            d = x - mean
            qs.append(d * d)
        var = math.inf if any(math.isinf(q) for q in qs) else rounded(sum((Fraction(q) for q in qs), Fraction(0)) / n)
        sd = math.sqrt(var)
        out.append((float(n), rounded(total), mean, var, sd, sd / math.sqrt(float(n))))
    return out


def same_figures(a, b):
    return len(a) == len(b) and all(ref.same(x, y) for fa, fb in zip(a, b) for x, y in zip(fa, fb))


def test_checker_agrees_with_the_literal_definition():
    columns = 0
    for case in small_cases():
        got, want = pref.profile(*case), literal(*case)
        assert same_figures(got, want), (case, got, want)
        columns += sum(1 for f in want if f[0] > 1)
    assert columns > 150


def test_each_mutant_is_caught():
    """strand ignored, window not cut at the chromosome's end, q against the offset's mean: each gives other figures
    than the definition on many of these inputs"""
    caught = {"nostrand": 0, "nocut": 0, "offsetmean": 0}
    cases = small_cases()
    for case in cases:
        want = literal(*case)
        for m in caught:
            if not same_figures(pref.profile(*case, mutant=m), want):
                caught[m] += 1
    assert all(c >= 10 for c in caught.values()), caught


def test_offset_mean_mutant_differs_only_in_the_variance():
    rng = np.random.default_rng(5)
    v = [rng.standard_normal(50) * 10 + np.arange(50)]
    anchors = [(0, p, 1) for p in range(10, 40)]
    a = pref.profile(v, anchors, -4, 8, bin=4)
    b = pref.profile(v, anchors, -4, 8, bin=4, mutant="offsetmean")
    for fa, fb in zip(a, b):
        assert all(ref.same(x, y) for x, y in zip(fa[:3], fb[:3]))
        assert fb[3] < fa[3]                                      # (a trend inside the bin is variance only against the bin's mean)


def test_images_are_the_samples_images():
    for vectors, anchors, off_lo, noffsets, bin, lo, hi in small_cases()[:40]:
        img = pref.images(vectors, anchors, off_lo, noffsets, lo, hi)
        figs = pref.profile(vectors, anchors, off_lo, noffsets, 1, lo, hi)
        assert img[:, 68].tolist() == [f[0] for f in figs]
        means = pref.offset_means(pref.profile(vectors, anchors, off_lo, noffsets, bin, lo, hi), bin)
        sq = pref.images(vectors, anchors, off_lo, noffsets, lo, hi, mean=means)
        assert sq[:, 68].tolist() == img[:, 68].tolist()


def test_duplicates_count_twice_and_order_does_not_matter():
    rng = np.random.default_rng(9)
    v = [rng.standard_normal(40), rng.standard_normal(17)]
    anchors = [(0, 5, 1), (1, 16, -1), (0, 39, -1), (1, 0, 1)]
    once = pref.profile(v, anchors, -3, 9, bin=3)
    twice = pref.profile(v, anchors + anchors, -3, 9, bin=3)
    for a, b in zip(once, twice):
        assert b[0] == 2 * a[0] and ref.same(a[2], b[2])
    assert same_figures(once, pref.profile(v, anchors[::-1], -3, 9, bin=3))
    swapped = [(1 - c, p, s) for c, p, s in anchors]
    assert same_figures(once, pref.profile(v[::-1], swapped, -3, 9, bin=3))


def test_a_single_plus_anchor_reads_the_values_themselves():
    v = [np.arange(10, dtype=np.float64) * 1.5]
    figs = pref.profile(v, [(0, 4, 1)], -6, 13)
    assert [f[0] for f in figs] == [0, 0] + [1] * 10 + [0]
    assert [f[1] for f in figs[2:12]] == v[0].tolist()
    minus = pref.profile(v, [(0, 4, -1)], -6, 13)
    assert [f[1] for f in minus[1:11]] == v[0][::-1].tolist() and minus[0][0] == 0


def test_best_column():
    assert pref.best([-2, -1, 0, 1], [math.nan, 3.0, 5.0, 5.0]) == (0, 5.0)
    assert pref.best([0, 1], [math.nan, math.nan]) is None
    assert pref.best([7], [-1.0]) == (7, -1.0)


def test_anchor_positions():
    """[s, e) zero-based half-open, per --anchor and strand"""
    table = {("start", False): 10, ("start", True): 19, ("end", False): 19, ("end", True): 10,
             ("center", False): 14, ("center", True): 15}
    for (mode, minus), want in table.items():
        assert pref.anchor_position(10, 20, minus, mode) == want, (mode, minus)
    for mode in ("start", "end", "center"):
        for minus in (False, True):
            assert pref.anchor_position(7, 8, minus, mode) == 7                     # one base
            assert pref.anchor_position(10, 21, minus, "center") == 15              # an odd length has one middle
    # the minus strand's anchor is the plus strand's of the mirrored interval
    L = 100
    for s, e in ((0, 1), (3, 9), (3, 10), (50, 100)):
        for mode in ("start", "end", "center"):
            assert pref.anchor_position(s, e, True, mode) == L - 1 - pref.anchor_position(L - e, L - s, False, mode)


def test_header_declares_the_profile_calls():
    text = open(os.path.join(ROOT, "include", "genodsp_hip.h")).read()
    for call in ("gdsp_profile_block", "gdsp_profile_accumulate_batch", "gdsp_genome_profile (", "gdsp_genome_profile_use_comm",
                 "gdsp_genome_profile_last", "gdsp_profile_set_launch_anchors", "GDSP_PROFILE_MAX_OFFSETS 16384",
                 "typedef struct gdsp_profile_source"):
        assert call in text, call
    import genodsp_amd as g
    from genodsp_amd import _lib
    for name in ("gdsp_profile_block", "gdsp_profile_set_launch_anchors", "gdsp_profile_accumulate_batch", "gdsp_genome_profile",
                 "gdsp_genome_profile_use_comm", "gdsp_genome_profile_last"):
        assert name in _lib.SIGNATURES, name
    for name in ("genome_profile", "profile_images", "profile_block", "genome_profile_last", "profile_set_launch_anchors"):
        assert callable(getattr(g, name)), name
    assert g.PROFILE_MAX_OFFSETS == pref.MAX_OFFSETS
