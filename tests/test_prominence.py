"""prominence (not in the reference; gdsp_prominence in include/genodsp_hip.h) against the numpy checker
tests/prominence_ref.py: the prominence bit for bit, the base level by value (it is an input value; the sign of a zero is
open).  Sizes and crafted vectors aim at the kernel's seams: the tile (gdsp_prominence_tile), its halos of wL and wR
bases, and the summary blocks of 8, 64 and 512 staged positions the walks skip over: tile k stages base b of the vector
at position HL + b - k*T, HL = wL rounded up to even, and the blocks are aligned in staged positions."""
import numpy as np
import pytest

import prominence_ref as ref
from test_prominence_ref import KINDS, data

MAXW = 4095
WINDOWS = [1, 2, 3, 4, 11, 100, 101, 1000, 1001, 4094, 4095]
EINVAL = 1


def tile_of(W):
    """outputs per workgroup of the kernel for window W, as the library reports it (host code)"""
    import genodsp_amd as gd
    return gd.lib().gdsp_prominence_tile(W)


def gd_mod():
    import genodsp_amd as gd
    gd.set_device(0)
    return gd


def check(gd, v, W, tag, where=None):
    """both outputs of the library on v against the checker (at the bases `where`, default all)"""
    with np.errstate(over="ignore", invalid="ignore"):
        want_p, want_b = ref.prominence(v, W)
    d = gd.DeviceVector.from_numpy(v)
    got_p = gd.prominence(d, W).numpy()
    got_b = gd.prominence(d, W, as_="base").numpy()
    assert d.numpy().tobytes() == v.tobytes(), tag                      # out of place
    sel = slice(None) if where is None else where
    bad = np.flatnonzero(got_p[sel].view(np.uint64) != want_p[sel].view(np.uint64))
    assert bad.size == 0, (tag, "prominence", bad[:5], got_p[sel][bad[:5]], want_p[sel][bad[:5]])
    bad = np.flatnonzero(~(got_b[sel] == want_b[sel]))
    assert bad.size == 0, (tag, "base", bad[:5], got_b[sel][bad[:5]], want_b[sel][bad[:5]])


def lengths_for(W):
    T = tile_of(W)
    wL, wR = ref.reach(W)
    return sorted(set(n for n in (1, 2, wL, W, T - 1, T, T + 1, 2 * T + wR + 3) if 1 <= n < 40000))


@pytest.mark.gpu
@pytest.mark.parametrize("W", WINDOWS)
def test_matches_the_checker(W):
    gd = gd_mod()
    for n in lengths_for(W):
        for kind in KINDS:
            rng = np.random.default_rng([W, n, KINDS.index(kind)])
            check(gd, data(kind, n, rng), W, (W, n, kind))


def crafted(W, T):
    """-> [(name, vector)]: a floor of 2 with one peak of 5 whose other side holds a 1, so that the crafted side decides"""
    wL, wR = ref.reach(W)
    n = 2 * T + wR + 40
    out = []

    def vec(peak, marks, far):
        v = np.full(n, 2.0)
        v[peak] = 5.0
        v[peak + far] = 1.0
        for pos, val in marks:
            v[pos] = val
        return v

    for peak in (T + 7, T, T - 1, wL + 3, n - wR - 4):                  # (T, T-1: the first base of a tile, the last)
        if peak - wL - 2 >= 0 and peak + 2 < n:
            out += [("high at wL left of %d" % peak, vec(peak, [(peak - wL, 9.0)], 2)),
                    ("high at wL+1 left of %d" % peak, vec(peak, [(peak - wL - 1, 9.0)], 2)),
                    ("low at wL left of %d" % peak, vec(peak, [(peak - wL, 0.0)], 2)),
                    ("low at wL+1 left of %d" % peak, vec(peak, [(peak - wL - 1, 0.0)], 2))]
            if wL >= 2:
                out.append(("low behind a high left of %d" % peak, vec(peak, [(peak - wL + 1, 9.0), (peak - wL, 0.0)], 2)))
        if peak + wR + 2 < n and peak - 2 >= 0:
            out += [("high at wR right of %d" % peak, vec(peak, [(peak + wR, 9.0)], -2)),
                    ("high at wR+1 right of %d" % peak, vec(peak, [(peak + wR + 1, 9.0)], -2)),
                    ("low at wR right of %d" % peak, vec(peak, [(peak + wR, 0.0)], -2)),
                    ("low at wR+1 right of %d" % peak, vec(peak, [(peak + wR + 1, 0.0)], -2))]
            if wR >= 2:
                out.append(("low behind a high right of %d" % peak, vec(peak, [(peak + wR - 1, 9.0), (peak + wR, 0.0)], -2)))
    # the stopping value in the last position of a tile and in the first of the next, peaks on both sides of it
    for stop in (T - 1, T, 2 * T - 1, 2 * T):
        v = np.full(n, 2.0)
        v[stop] = 9.0
        for peak in (stop - 5, stop + 5, stop - wL + 1, stop + wR - 1):
            if 0 < peak < n - 1 and peak != stop:
                v[peak] = 5.0
        v[max(0, stop - wL - 3)] = 0.0
        v[min(n - 1, stop + wR + 3)] = 0.0
        out.append(("stop at %d" % stop, v))
    # the deciding minimum in the halo of the tile that owns the peak
    if wL >= 4:
        v = np.full(n, 2.0)
        v[T + 1] = 5.0;  v[T - 3] = 0.5;  v[T + 3] = 0.25
        v[2 * T - 2] = 6.0;  v[2 * T + 2] = 1.5;  v[2 * T - 4] = 1.0
        out.append(("minimum in the halo", v))
    # plateaus: straddling a seam; longer than the window
    v = np.full(n, 2.0)
    v[T - 5:T + 6] = 5.0
    v[3] = 1.0
    out.append(("plateau over the seam", v))
    v = np.full(n, 1.0)
    v[T - W - 9:T + W + 9] = 4.0
    out.append(("plateau longer than W", v))
    # peaks at the two ends of the vector
    v = np.full(n, 2.0)
    v[0] = 8.0;  v[n - 1] = 8.0;  v[1] = 1.0;  v[n - 2] = 1.0;  v[5] = 3.0;  v[n - 6] = 3.0
    out.append(("peaks at the ends", v))
    # the first greater value in position 0, 63 and 64 of a summary block (tile 0 stages base b at wL rounded up to even + b)
    HL = (wL + 1) & ~1
    for k in (0, 63, 64):
        for far in (200, 70, 5):
            g = 64 * 4 + k - HL % 64
            if g - 1 >= 0 and g + far + 2 < n and far <= min(wL, wR):
                v = np.full(n, 2.0);  v[g] = 9.0;  v[g + far] = 5.0;  v[g + 1] = 1.5;  v[g - 1] = 0.0;  v[g + far + 2] = 1.0
                out.append(("greater at block position %d, left of a peak %d away" % (k, far), v))
                v = np.full(n, 2.0);  v[g + far] = 9.0;  v[g] = 5.0;  v[g + far - 1] = 1.5;  v[g + far + 1] = 0.0;  v[g - 2] = 1.0
                out.append(("greater %d right of a peak at block position %d" % (far, k), v))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("W", [4, 100, 101, 1000, 4095])
def test_crafted_vectors(W):
    gd = gd_mod()
    T = tile_of(W)
    cases = crafted(W, T)
    assert len(cases) >= 20
    for name, v in cases:
        check(gd, v, W, (W, name))


def ladder(W, T):
    """-> [(name, vector)] for the walks' ladder of block sizes (single values, 8, 64, 512 staged positions): the first
    greater value, or the deciding minimum, on either side of a multiple of 512, a peak far enough away that whole blocks
    of 512 lie between; and the deciding minimum in the last few positions of a window, where the walk has stepped down
    to blocks of 64, of 8 and to single values -- or one base beyond, where it decides nothing.  In tile 0 and in tile 1."""
    wL, wR = ref.reach(W)
    HL = (wL + 1) & ~1
    n = 2 * T + wR + 40
    out = []

    def vec(peak, marks, other):
        v = np.full(n, 2.0)
        v[peak] = 5.0
        v[other] = -1.0                                                 # the other side's minimum: below every mark
        for pos, val in marks:
            v[pos] = val
        return v

    for tile in (0, 1):
        for edge in range(512, HL + T + wR, 512):
            for d in (-1, 0, 1):
                at = edge + d - HL + tile * T                           # the base staged at a multiple of 512, and its neighbours
                for far in (600, 1100, 70):
                    if far > min(wL, wR):
                        continue
                    for side in (-1, 1):                                # the peak to the right of `at`, to the left of it
                        peak = at - side * far
                        if not (tile * T <= peak < min((tile + 1) * T, n - 3)) or not (2 <= at < n - 2) or peak < 3:
                            continue
                        out.append(("greater at staged %d%+d, peak %d to its %s (tile %d)" % (edge, d, far, "right" if side < 0 else "left", tile),
                                    vec(peak, [(at, 9.0), (at + side, 0.0), (at - side, 1.5)], peak - 2 * side)))
                        out.append(("minimum at staged %d%+d, peak %d to its %s (tile %d)" % (edge, d, far, "right" if side < 0 else "left", tile),
                                    vec(peak, [(at, 0.0)], peak - 2 * side)))
        peak = tile * T + T // 2
        for back in (-1, 0, 1, 3, 8, 9, 63, 64, 70, 511, 512, 600):       # (-1: one base outside the window)
            if peak - wL + back > 2 and back < wL:
                out.append(("minimum %d inside the left end (tile %d)" % (back, tile), vec(peak, [(peak - wL + back, 0.0)], peak + 2)))
            if peak + wR - back < n - 2 and back < wR:
                out.append(("minimum %d inside the right end (tile %d)" % (back, tile), vec(peak, [(peak + wR - back, 0.0)], peak - 2)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("W", [1000, 4094, 4095])
def test_the_ladder_of_block_sizes(W):
    gd = gd_mod()
    cases = ladder(W, tile_of(W))
    assert len(cases) >= 60, len(cases)
    for name, v in cases:
        check(gd, v, W, (W, name))


@pytest.mark.gpu
def test_crafted_vectors_decide_what_they_are_meant_to():
    """the library itself on the hand-worked figures: a low value at exactly wL counts, one base further it does not"""
    gd = gd_mod()
    W = 100
    wL, wR = ref.reach(W)                                               # 49 left, 50 right
    T = tile_of(W)
    for peak in (T, T - 1, T + 7):
        for side, w in ((-1, wL), (+1, wR)):
            for d, want in ((w, 4.0), (w + 1, 3.0)):
                v = np.full(2 * T, 2.0)
                v[peak] = 5.0
                v[peak - 2 * side] = 1.0                                # the other side's minimum
                v[peak + side * d] = 0.0
                got = gd.prominence(gd.DeviceVector.from_numpy(v), W).numpy()
                assert got[peak] == want, (peak, side, d, got[peak])


@pytest.mark.gpu
@pytest.mark.parametrize("W", [11, 1001, 4094])
def test_batch_equals_the_single_vector_calls(W):
    gd = gd_mod()
    T = tile_of(W)
    rng = np.random.default_rng(W)
    hosts = [np.round(rng.standard_normal(n) * 3, 1) for n in (0, 1, T - 1, T + 1, 3 * T + 5, 17)]
    vecs = [gd.DeviceVector.from_numpy(h) for h in hosts]
    for as_ in ("prominence", "base"):
        outs = gd.prominence_batch(vecs, W, as_=as_)
        assert len(outs) == len(vecs)
        for h, v, o in zip(hosts, vecs, outs):
            assert v.numpy().tobytes() == h.tobytes()                   # the inputs are unchanged
            if v.n:
                assert o.numpy().tobytes() == gd.prominence(v, W, as_=as_).numpy().tobytes(), (W, as_, v.n)
        want = ref.prominence(hosts[4], W)
        assert outs[4].numpy().tobytes() == want[0].tobytes() if as_ == "prominence" else np.array_equal(outs[4].numpy(), want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("W", [4, 101, 1000])
def test_nan_spoils_only_the_windows_that_hold_it(W):
    gd = gd_mod()
    T = tile_of(W)
    n = 2 * T + 300
    rng = np.random.default_rng(W)
    v = rng.integers(0, 9, n).astype(np.float64)
    v[[5, T - 1, T + 130]] = np.nan
    ok = ref.clean(v, W)
    assert 0 < np.count_nonzero(~ok) < n // 2
    check(gd, v, W, (W, "nan"), where=ok)


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    gd = gd_mod()
    L = gd.lib()
    d = gd.DeviceVector.from_numpy(np.arange(100.0))
    o = d.like()
    assert L.gdsp_prominence(d.ptr, d.ptr, d.n, 11, 0, None) == EINVAL
    assert L.gdsp_prominence(d.ptr, o.ptr, d.n, 0, 0, None) == EINVAL
    assert L.gdsp_prominence(d.ptr, o.ptr, d.n, MAXW + 1, 0, None) == EINVAL
    assert L.gdsp_prominence(d.ptr, o.ptr, d.n, 11, 2, None) == EINVAL
    assert L.gdsp_prominence(d.ptr, o.ptr, d.n, 11, -1, None) == EINVAL
    assert L.gdsp_prominence(d.ptr, o.ptr, 0, 11, 0, None) == 0
    items = gd.batch_items([d], [d])
    assert L.gdsp_prominence_batch(items, 1, 11, 0, None) == EINVAL
    items = gd.batch_items([d], [o])
    assert L.gdsp_prominence_batch(items, 1, 0, 0, None) == EINVAL
    assert L.gdsp_prominence_batch(items, 1, MAXW + 1, 0, None) == EINVAL
    assert L.gdsp_prominence_batch(items, 1, 11, 2, None) == EINVAL
    assert L.gdsp_prominence(d.ptr, o.ptr, d.n, MAXW, 1, None) == 0
    with pytest.raises(ValueError):
        gd.prominence(d, 11, as_="nonsense")
    assert gd.PROMINENCE_MAX_WINDOW == MAXW


def test_the_tile_query():
    """host code: 0 outside 1..4095; inside, a tile with both reaches fits what one workgroup stages -- which is the
    tile of W = 1, the window with no reach"""
    assert tile_of(0) == 0 and tile_of(MAXW + 1) == 0 and tile_of(2 ** 31) == 0
    staged = tile_of(1)
    for W in WINDOWS:
        T = tile_of(W)
        assert T > 0 and T % 2 == 0 and T + W - 1 <= staged, (W, T, staged)
        assert tile_of(W) <= tile_of(max(1, W - 1))                     # a longer window never leaves more outputs
