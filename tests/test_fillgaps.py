"""fillgaps (not in the reference; gdsp_fillgaps in include/genodsp_hip.h) against the checker tests/fillgaps_ref.py, bit
for bit.  Lengths and contents aim at the seams of the three launches (gdsp_fillgaps.hip): the 64-base mask word, the pair
of bases a lane stores, the workgroup tile (gdsp_fillgaps_tile), tiles that are skipped because they hold nothing unknown
or nothing to fill, gaps that run across whole tiles so that both neighbours come from the join, the longest gap, and the
vectors of a batch, across which nothing may be carried.

Run as a program it prints a digest of a fixed set of calls (the poison test starts it with GDSP_POISON set)."""
import hashlib
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import distance_ref
import fillgaps_ref as ref

EINVAL = 1
CONTENTS = ("none", "every", "first", "last", "lonely", "tile_seam", "word_seam", "across_tiles", "nonfinite", "half", "sparse",
            "rare", "ties", "negative")
BOTH_TESTS = ("nonfinite", "half", "sparse", "rare")                # contents with non-positive values: both `known` tests


def gd_mod():
    import genodsp_amd as gd
    gd.set_device(0)
    return gd


def tile():
    """bases per workgroup tile, as the library reports it (host code)"""
    import genodsp_amd as gd
    return gd.lib().gdsp_fillgaps_tile()


def lengths():
    Tl = tile()
    return [1, 2, 63, 64, 65, Tl - 1, Tl, Tl + 1, 2 * Tl + 1, 3 * Tl - 1, 4 * Tl + 5]


def options():
    return list(itertools.product(ref.HOW, ref.ENDS, (None, 1, 100, tile() + 1)))


def content(name, n):
    """-> (v, T), or None where a vector of n bases cannot hold it"""
    Tl = tile()
    rng = np.random.default_rng(sum(map(ord, name)) * 100003 + n)
    v = np.zeros(n)
    if name == "none":                                            # nothing known: the output is the input
        return -rng.random(n), 0.0
    if name == "every":
        return rng.random(n) + 2.5, 0.0
    if name in ("first", "last"):
        v = -rng.random(n)
        v[0 if name == "first" else n - 1] = 1.25
        return v, 0.0
    if name == "lonely":                                          # one known base: both ends extend over whole empty tiles
        if n != 4 * Tl + 5:
            return None
        v[Tl + 3] = 1.75
        return v, 0.0
    if name == "tile_seam":
        if n <= Tl:
            return None
        v[Tl - 1], v[Tl] = 1.0, 3.0
        return v, 0.0
    if name == "word_seam":
        if n <= 64:
            return None
        v[63], v[64] = 1.0, 3.0
        return v, 0.0
    if name == "across_tiles":                                    # one gap from inside tile 0 to inside tile 3: l and r both
        if n != 4 * Tl + 5:                                       # come from the carry in the tiles between
            return None
        v = rng.random(n) + 0.5
        v[Tl // 2 + 1: 3 * Tl + 101] = -rng.random(3 * Tl + 101 - (Tl // 2 + 1))
        return v, 0.0
    if name == "nonfinite":                                       # unknown NaNs are filled, known infinities are kept
        v = rng.choice([0.0, 1.0, np.nan, np.inf, -np.inf, -0.0], n, p=[0.55, 0.15, 0.1, 0.05, 0.05, 0.1])
        return v, 0.0
    if name in ("half", "sparse", "rare"):
        density = {"half": 0.5, "sparse": 1 / 64.0, "rare": 1 / 5000.0}[name]
        return np.where(rng.random(n) < density, rng.random(n) + 0.5, -rng.random(n)), 0.0
    if name == "ties":                                            # values equal to the threshold, taken either way
        return rng.choice([1.0, 2.0, 3.0], n, p=[0.6, 0.3, 0.1]), 2.0
    if name == "negative":                                        # known="nonzero": negative values count
        return np.where(rng.random(n) < 0.1, rng.standard_normal(n), rng.choice([0.0, -0.0], n)), 0.0
    raise ValueError(name)


def library(gd, v, T=0.0, ties=False, known="above", how="linear", ends="extend", maxgap=None):
    d = gd.DeviceVector.from_numpy(v)
    out = gd.fill_gaps(d, T, ties, known, how, ends, maxgap)
    assert out is d                                               # in place, and it returns its argument
    return d.numpy()


def same(got, want, what):
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (what, bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONTENTS)
def test_matches_the_checker(name):
    gd = gd_mod()
    calls = 0
    for n in lengths():
        made = content(name, n)
        if made is None:
            continue
        v, T = made
        tests = [("above", False)]
        if name == "ties":
            tests.append(("above", True))
        if name in BOTH_TESTS:
            tests.append(("nonzero", False))
        if name == "negative":
            tests = [("nonzero", False)]
        for known, ties in tests:
            for how, ends, maxgap in options():
                got = library(gd, v, T, ties, known, how, ends, maxgap)
                same(got, ref.fill_gaps(v, T, ties, known, how, ends, maxgap), (name, n, known, ties, how, ends, maxgap))
                if name == "none":
                    same(got, v, (name, n, "untouched"))
                calls += 1
    assert calls >= 32


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 100, "tile+1"])
def test_gaps_of_exactly_the_longest_and_one_more(G):
    """in the interior and at either end, in a vector of no more than four tiles: the gap of G bases is filled, the one of
    G + 1 stays as it is"""
    gd = gd_mod()
    G = tile() + 1 if G == "tile+1" else G
    n = 4 * tile() + 5
    rng = np.random.default_rng(G)
    for front, inner, back in ((G, G + 1, G + 1), (G + 1, G, G), (G + 1, G + 1, G), (G, G, G + 1)):
        v = rng.random(n) + 0.5
        for s, e in ((0, front), (front + 8, front + 8 + inner), (n - back, n)):     # an end gap, an interior one, an end gap
            v[s:e] = -rng.random(e - s)
        L, R = ref.neighbours(v > 0)
        assert sorted(set((R - L - 1)[v <= 0].tolist())) == [G, G + 1] and np.count_nonzero(v <= 0) == front + inner + back
        long_gap = (v <= 0) & (R - L - 1 > G)
        for how, ends in itertools.product(ref.HOW, ref.ENDS):
            got = library(gd, v, how=how, ends=ends, maxgap=G)
            same(got, ref.fill_gaps(v, how=how, ends=ends, maxgap=G), (G, front, inner, back, how, ends))
            same(got[long_gap], v[long_gap], (G, front, inner, back, how, ends, "the long gaps"))
            if inner == G:
                assert (got[front + 8: front + 8 + inner] > 0).all()


@pytest.mark.gpu
def test_arguments():
    gd = gd_mod()
    L = gd.lib()
    start = np.arange(10.0) - 4.0
    d = gd.DeviceVector.from_numpy(start)
    for known, how, ends in ((2, 0, 0), (-1, 0, 0), (0, 4, 0), (0, -1, 0), (0, 0, 2), (1, 0, -1)):
        assert L.gdsp_fillgaps(d.ptr, 10, 0.0, 0, known, how, ends, 0, None) == EINVAL, (known, how, ends)
        assert b"unknown" in L.gdsp_last_error()
    assert L.gdsp_fillgaps(d.ptr, 10, float("nan"), 0, 0, 0, 0, 0, None) == EINVAL and b"NaN" in L.gdsp_last_error()
    assert d.numpy().tobytes() == start.tobytes()                 # a refused call writes nothing
    assert L.gdsp_fillgaps(None, 0, 0.0, 0, 0, 0, 0, 0, None) == 0   # n == 0: a no-op
    for bad in (dict(how="cubic"), dict(known="positive"), dict(ends="wrap"), dict(maxgap=0), dict(maxgap=-3)):
        with pytest.raises(ValueError):
            gd.fill_gaps(d, **bad)
        with pytest.raises(ValueError):
            gd.fill_gaps_batch([d], **bad)
    assert d.numpy().tobytes() == start.tobytes()
    assert gd.fill_gaps(d, float("nan"), known="nonzero").numpy().tolist() == [-4, -3, -2, -1, 0, 1, 2, 3, 4, 5]   # T is not used
    e = gd.DeviceVector.from_numpy(np.array([0.0, 0, 2, 0, 0, 0, 6, 0]))
    assert gd.fill_gaps(e) is e and e.numpy().tolist() == [2, 2, 2, 3, 4, 5, 6, 6]
    assert tile() % 128 == 0 and tile() == L.gdsp_distance_tile()


def batch_vectors(count):
    """mixed lengths, 0, 1 and the tile among them; vectors without any known base between vectors with known bases at
    their very ends: a carry that leaked across vectors would fill what has to stay as it is"""
    Tl = tile()
    sizes = [Tl, 1, 2 * Tl + 1, 65, 0, 3 * Tl - 1, Tl + 1, 64, 4 * Tl + 5, 63, Tl - 1]
    rng = np.random.default_rng(77 + count)
    vecs = []
    for k in range(count):
        n = sizes[k % len(sizes)]
        v = -rng.random(n)
        if k % 3 == 0 and n > 0:
            v[0], v[n - 1] = 1.5, 2.5                             # known bases at both ends,
        elif k % 3 == 2:
            v = np.where(rng.random(n) < 1 / 300.0, rng.random(n) + 1.0, v)      # (and some noise)
        vecs.append(v)                                            # k % 3 == 1: nothing known
    return vecs


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 5, 35])
def test_a_batch_is_its_vectors(count):
    gd = gd_mod()
    vecs = batch_vectors(count)
    assert count < 5 or any(v.size == 0 for v in vecs)
    for how, ends, maxgap in [("linear", "extend", None), ("nearest", "keep", None), ("left", "extend", 100),
                              ("right", "extend", None), ("linear", "keep", tile() + 1)]:
        ds = [gd.DeviceVector.from_numpy(v) for v in vecs]
        outs = gd.fill_gaps_batch(ds, how=how, ends=ends, maxgap=maxgap)
        gd.sync()
        for k, v in enumerate(vecs):
            got = outs[k].numpy()
            assert got.tobytes() == ref.fill_gaps(v, how=how, ends=ends, maxgap=maxgap).tobytes(), (count, k, v.size, how, ends, maxgap)
            if v.size:
                assert got.tobytes() == library(gd, v, how=how, ends=ends, maxgap=maxgap).tobytes()
            if k % 3 == 1:
                assert got.tobytes() == v.tobytes()               # nothing came in from the neighbours


@pytest.mark.gpu
def test_two_streams_take_the_workspace_in_turn():
    """calls on two streams of the device, fillgaps' and distance's, which share the workspace, none waited for"""
    gd = gd_mod()
    n = 4 * tile() + 5
    streams = [gd.Stream(), gd.Stream()]
    made, wants = [], []
    for k in range(12):
        v = content(("sparse", "half", "rare", "across_tiles")[k % 4], n - 7 * k)[0] if k % 4 != 3 else content("across_tiles", n)[0]
        d = gd.DeviceVector.from_numpy(v)
        if k % 3 == 2:
            gd.distance(d, stream=streams[k % 2].handle)
            wants.append(distance_ref.distance(v))
        else:
            how = ref.HOW[k % 4]
            gd.fill_gaps(d, how=how, stream=streams[k % 2].handle)
            wants.append(ref.fill_gaps(v, how=how))
        made.append(d)
    for S in streams:
        gd.sync(S.handle)
    for k, (d, want) in enumerate(zip(made, wants)):
        same(d.numpy(), want, k)


def digest():
    """the bytes of a fixed set of calls, the workspace growing on the way (small vector first, batches last)"""
    gd = gd_mod()
    h = hashlib.sha256()
    for n in (65, tile() + 1, 4 * tile() + 5):
        for name in ("lonely", "across_tiles", "sparse", "nonfinite"):
            made = content(name, n)
            if made is None:
                continue
            for how, ends, maxgap in (("linear", "extend", None), ("nearest", "keep", None), ("left", "extend", 100)):
                h.update(library(gd, made[0], made[1], False, "above", how, ends, maxgap).tobytes())
    for count in (5, 35):
        outs = gd.fill_gaps_batch([gd.DeviceVector.from_numpy(v) for v in batch_vectors(count)])
        gd.sync()
        for o in outs:
            h.update(o.numpy().tobytes())
    return h.hexdigest()


@pytest.mark.gpu
def test_poisoned_workspace_changes_nothing():
    """GDSP_POISON fills every device allocation (the library's own mask words, extents and carries among them) before
    it is handed out; every word is written before it is read, so the results stay the same"""
    want = digest()
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GDSP_POISON="nan"),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.strip() == want


if __name__ == "__main__":
    print(digest())
