"""distance (not in the reference; gdsp_distance in include/genodsp_hip.h) against the checker tests/distance_ref.py, bit
for bit.  Lengths and contents aim at the seams of the three launches (gdsp_distance.hip): the 64-base mask word, the
workgroup tile (gdsp_distance_tile), tiles without any member between tiles that have one (the join carries across
them, both ways), runs longer than a tile (the same for the complement), and the vectors of a batch, across which nothing
may be carried.

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
import distance_ref as ref

EINVAL = 1
CONTENTS = ("none", "every", "first", "last", "lonely", "tile_seam", "word_seam", "long_runs", "nonfinite", "half", "sparse",
            "rare", "ties")


def gd_mod():
    import genodsp_amd as gd
    gd.set_device(0)
    return gd


def tile():
    """bases per workgroup tile, as the library reports it (host code)"""
    import genodsp_amd as gd
    return gd.lib().gdsp_distance_tile()


def lengths():
    Tl = tile()
    return [1, 63, 64, 65, Tl - 1, Tl, Tl + 1, 2 * Tl + 1, 3 * Tl - 1, 4 * Tl + 5]


def options():
    return list(itertools.product(ref.SIDES, (False, True), (None, 1, 100, tile() + 1)))


def content(name, n):
    """-> (v, T), or None where a vector of n bases cannot hold it"""
    Tl = tile()
    rng = np.random.default_rng(sum(map(ord, name)) * 100003 + n)
    v = np.zeros(n)
    if name == "none":
        return v - 1.0, 0.0
    if name == "every":
        return v + 2.5, 0.0
    if name in ("first", "last"):
        v[0 if name == "first" else n - 1] = 1.0
        return v, 0.0
    if name == "lonely":                                          # one member, whole tiles without any on both sides of it
        if n != 4 * Tl + 5:
            return None
        v[Tl + 3] = 1.0
        return v, 0.0
    if name == "tile_seam":
        if n <= Tl:
            return None
        v[Tl - 1] = v[Tl] = 1.0
        return v, 0.0
    if name == "word_seam":
        if n <= 64:
            return None
        v[63] = v[64] = 1.0
        return v, 0.0
    if name == "long_runs":                                       # runs that span whole tiles: the depth inside them goes beyond a tile
        if n <= Tl:
            return None
        v[:] = 1.0
        v[n // 7] = 0.0
        if n > 3 * Tl:
            v[3 * Tl + 2: 3 * Tl + 40] = 0.0
        return v, 0.0
    if name == "nonfinite":
        v = rng.choice([0.0, 1.0, np.nan, np.inf, -np.inf, -0.0], n, p=[0.55, 0.15, 0.1, 0.05, 0.05, 0.1])
        return v, 0.0
    if name in ("half", "sparse", "rare"):
        density = {"half": 0.5, "sparse": 1 / 64.0, "rare": 1 / 5000.0}[name]
        return np.where(rng.random(n) < density, rng.random(n) + 0.5, -rng.random(n)), 0.0
    if name == "ties":                                            # values equal to the threshold, taken either way
        return rng.choice([1.0, 2.0, 3.0], n, p=[0.6, 0.3, 0.1]), 2.0
    raise ValueError(name)


def library(gd, v, T, ties, to, signed, cap):
    d = gd.DeviceVector.from_numpy(v)
    out = gd.distance(d, T, ties, to, signed, cap)
    assert out is d                                               # in place
    return d.numpy()


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
        for ties in ((False, True) if name == "ties" else (False,)):
            for to, signed, cap in options():
                got = library(gd, v, T, ties, to, signed, cap)
                want = ref.distance(v, T, ties, to, signed, cap)
                bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
                assert bad.size == 0, (name, n, ties, to, signed, cap, bad[:5], got[bad[:5]], want[bad[:5]])
                calls += 1
    assert calls >= 24


@pytest.mark.gpu
def test_arguments():
    gd = gd_mod()
    L = gd.lib()
    d = gd.DeviceVector.from_numpy(np.arange(10.0))
    assert L.gdsp_distance(d.ptr, 10, 0.0, 0, 3, 0, 0, None) == EINVAL and b"unknown side" in L.gdsp_last_error()
    assert L.gdsp_distance(d.ptr, 10, 0.0, 0, -1, 0, 0, None) == EINVAL
    assert L.gdsp_distance(d.ptr, 10, float("nan"), 0, 0, 0, 0, None) == EINVAL and b"NaN" in L.gdsp_last_error()
    assert d.numpy().tobytes() == np.arange(10.0).tobytes()      # a refused call writes nothing
    assert L.gdsp_distance(None, 0, 0.0, 0, 0, 0, 0, None) == 0   # n == 0: a no-op
    with pytest.raises(ValueError):
        gd.distance(d, to="up")
    with pytest.raises(ValueError):
        gd.distance(d, cap=0)
    assert gd.distance(d, 3.0, cap=2).numpy().tolist() == [2, 2, 2, 1, 0, 0, 0, 0, 0, 0]
    assert tile() % 128 == 0


def batch_vectors(count):
    """mixed lengths, 1 and the tile among them; vectors without any member between vectors with members at their very
    ends: a carry that leaked across vectors would put a distance where the vector's length belongs"""
    Tl = tile()
    sizes = [Tl, 1, 2 * Tl + 1, 65, 3 * Tl - 1, Tl + 1, 64, 4 * Tl + 5, 63, Tl - 1]
    rng = np.random.default_rng(99 + count)
    vecs = []
    for k in range(count):
        n = sizes[k % len(sizes)]
        v = np.zeros(n)
        if k % 3 == 0:
            v[0] = v[n - 1] = 1.0                                 # members at both ends,
        elif k % 3 == 2:
            v = (rng.random(n) < 1 / 300.0) * 1.0                 # (and some noise)
        vecs.append(v)                                            # k % 3 == 1: no member at all
    return vecs


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 3, 33])
def test_a_batch_is_its_vectors(count):
    gd = gd_mod()
    vecs = batch_vectors(count)
    for to, signed, cap in [("nearest", False, None), ("nearest", True, None), ("left", False, None), ("right", True, 100),
                            ("right", False, None), ("left", True, tile() + 1)]:
        ds = [gd.DeviceVector.from_numpy(v) for v in vecs]
        outs = gd.distance_batch(ds, 0.0, False, to, signed, cap)
        gd.sync()
        for k, v in enumerate(vecs):
            got = outs[k].numpy()
            assert got.tobytes() == ref.distance(v, 0.0, False, to, signed, cap).tobytes(), (count, k, v.size, to, signed, cap)
            assert got.tobytes() == library(gd, v, 0.0, False, to, signed, cap).tobytes()
            if k % 3 == 1 and not signed and cap is None:
                assert (got == v.size).all()                      # nothing came in from the neighbours


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 500])
def test_dilate_and_erode_are_one_radius_of_it(r):
    """on the device: gd.dilate with left = right = r is distance <= r, gd.erode is signed distance <= -(r+1)"""
    gd = gd_mod()
    n = 3 * tile() - 1
    rng = np.random.default_rng(5)
    v = np.where(rng.random(n) < 1 / 700.0, 1.0, 0.0)
    v[n // 3: n // 3 + 2500] = 1.0                                # (and something for erode to leave)
    d = gd.DeviceVector.from_numpy(v)
    dil = gd.dilate(d, r, r).numpy()
    ero = gd.erode(d, r, r).numpy()
    near = gd.distance(gd.DeviceVector.from_numpy(v)).numpy()
    deep = gd.distance(gd.DeviceVector.from_numpy(v), signed=True).numpy()
    assert ((near <= r) == (dil == 1.0)).all() and 0 < np.count_nonzero(dil) < n
    assert ((deep <= -(r + 1)) == (ero == 1.0)).all() and np.count_nonzero(ero) > 0
    capped = gd.distance(gd.DeviceVector.from_numpy(v), signed=True, cap=r + 1).numpy()
    assert ((capped <= r) == (dil == 1.0)).all() and ((capped <= -(r + 1)) == (ero == 1.0)).all()      # both from one pass


def digest():
    """the bytes of a fixed set of calls, the workspace growing on the way (small vector first, batches last)"""
    gd = gd_mod()
    h = hashlib.sha256()
    for n in (65, tile() + 1, 4 * tile() + 5):
        for name in ("lonely", "long_runs", "sparse", "nonfinite"):
            made = content(name, n)
            if made is None:
                continue
            for to, signed, cap in (("nearest", False, None), ("nearest", True, None), ("left", True, 100)):
                h.update(library(gd, made[0], made[1], False, to, signed, cap).tobytes())
    for count in (3, 33):
        outs = gd.distance_batch([gd.DeviceVector.from_numpy(v) for v in batch_vectors(count)], signed=True)
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
