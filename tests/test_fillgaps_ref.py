"""tests/fillgaps_ref.py against itself: the vectorised checker held to the literal loop of the definition (gdsp_fillgaps,
include/genodsp_hip.h) on short vectors under every option combination, and to what the definition promises: the line of
np.interp, values between the two neighbours', the neighbours that `distance` finds, the longest gap, idempotence.
tests/test_fillgaps.py and tests/test_cli_fillgaps.py lean on it.  No GPU."""
import itertools

import numpy as np
import pytest

import distance_ref
import fillgaps_ref as ref

OPTIONS = list(itertools.product(ref.HOW, ref.ENDS, (None, 1, 3, 7)))
IDS = ["%s-%s-%s" % o for o in OPTIONS]

# test_linear_is_the_line_of_interp: the worst distance seen, in units of the spacing of doubles at max(|a|, |b|)
INTERP_WORST = 4.0


def contents(n, rng):
    """what a vector of n bases can hold that matters: nothing known, everything, one known base at either end, NaNs and
    infinities, negative values, and real values at several densities"""
    first = np.zeros(n)
    first[0] = 1.5
    last = np.zeros(n)
    last[n - 1] = -2.5
    odd = rng.choice([0.0, -0.0, 1.0, np.nan, np.inf, -np.inf, -3.0, 1e308, -1e308], n)
    out = [np.zeros(n), rng.random(n) + 1.0, first, last, odd]
    for density in (0.5, 0.2, 0.05):
        out.append(np.where(rng.random(n) < density, rng.standard_normal(n) * 100.0, 0.0))
        out.append(np.where(rng.random(n) < density, rng.random(n) + 0.5, -rng.random(n)))
    return out


@pytest.mark.parametrize("how,ends,maxgap", OPTIONS, ids=IDS)
def test_the_vectorised_checker_is_the_loop(how, ends, maxgap):
    rng = np.random.default_rng(20260202)
    count = 0
    for n in list(range(1, 25)) + [40]:
        for v in contents(n, rng):
            for known, T, ties in (("above", 0.0, False), ("nonzero", 0.0, False), ("above", 1.0, True), ("above", -1.0, False)):
                got = ref.fill_gaps(v, T, ties, known, how, ends, maxgap)
                want = ref.fill_gaps_loop(v, T, ties, known, how, ends, maxgap)
                assert got.tobytes() == want.tobytes(), (n, known, T, ties, v.tolist(), got.tolist(), want.tolist())
                count += 1
    assert count >= 300


def test_which_bases_are_known():
    v = np.array([0.0, 2.0, 3.0, np.nan, -0.0, -1.0, np.inf, -np.inf])
    assert ref.known_bases(v, 2.0).tolist() == [False, False, True, False, False, False, True, False]
    assert ref.known_bases(v, 2.0, True).tolist() == [False, True, True, False, False, False, True, False]
    assert ref.known_bases(v, known="nonzero").tolist() == [False, True, True, False, False, True, True, True]
    assert ref.known_bases(v, 99.0, True, "nonzero").tolist() == ref.known_bases(v, known="nonzero").tolist()   # T is not used


def test_small_cases_by_hand():
    v = np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 5.0, 0.0, 7.0, 0.0])
    assert ref.fill_gaps(v).tolist() == [1, 1, 1, 2, 3, 4, 5, 6, 7, 7]
    assert ref.fill_gaps(v, ends="keep").tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7, 0]
    assert ref.fill_gaps(v, how="nearest").tolist() == [1, 1, 1, 1, 1, 5, 5, 5, 7, 7]          # halfway: the lower coordinate
    assert ref.fill_gaps(v, how="left").tolist() == [1, 1, 1, 1, 1, 1, 5, 5, 7, 7]
    assert ref.fill_gaps(v, how="left", ends="keep").tolist() == [0, 0, 1, 1, 1, 1, 5, 5, 7, 7]
    assert ref.fill_gaps(v, how="right").tolist() == [1, 1, 1, 5, 5, 5, 5, 7, 7, 7]
    assert ref.fill_gaps(v, how="right", ends="keep").tolist() == [1, 1, 1, 5, 5, 5, 5, 7, 7, 0]
    assert ref.fill_gaps(v, maxgap=2).tolist() == [1, 1, 1, 0, 0, 0, 5, 6, 7, 7]
    assert ref.fill_gaps(v, maxgap=1).tolist() == [0, 0, 1, 0, 0, 0, 5, 6, 7, 7]
    assert ref.fill_gaps(v, 1.0).tolist() == [5, 5, 5, 5, 5, 5, 5, 6, 7, 7]                    # 1.0 is not above 1.0
    w = np.array([np.nan, np.inf, np.nan, -np.inf, 0.0, -np.inf, -0.0])
    got = ref.fill_gaps(w, known="nonzero")
    assert got[0] == np.inf and np.isnan(got[2]) and got[4] == -np.inf and got[6] == -np.inf   # inf - inf; a == b; the end
    none = np.array([0.0, -0.0, np.nan, -5.0])
    assert ref.fill_gaps(none).tobytes() == none.tobytes()                                     # nothing known: untouched


def interior(m):
    """the unknown bases that have a known base on both sides, with those two"""
    L, R = ref.neighbours(m)
    sel = ~m & (L >= 0) & (R < m.size)
    return sel, L, R


def test_linear_is_the_line_of_interp():
    """on interior gaps np.interp over the known bases computes a + ((b - a) / d) * k where the definition computes
    a + ((b - a) * k) / d: the two differ by roundings only.  Measured over these vectors the worst difference is
    4.0 spacings of doubles at max(|a|, |b|) (INTERP_WORST); the assertion is that figure doubled.  And every filled value
    lies in [min(a, b), max(a, b)], which np.interp's does not always."""
    rng = np.random.default_rng(31)
    worst = 0.0
    for n in (2, 17, 40, 300, 5000):
        for scale, density in itertools.product((1.0, 1e-3, 1e6), (0.5, 0.1, 0.01)):
            v = np.where(rng.random(n) < density, rng.standard_normal(n) * scale, 0.0)
            v[0] = v[n - 1] = scale
            m = ref.known_bases(v, known="nonzero")
            got = ref.fill_gaps(v, known="nonzero")
            sel, L, R = interior(m)
            if not sel.any():
                continue
            idx = np.arange(n)
            line = np.interp(idx[sel], idx[m], v[m])
            a, b = v[L[sel]], v[R[sel]]
            unit = np.spacing(np.maximum(np.abs(a), np.abs(b)))
            worst = max(worst, float(np.max(np.abs(got[sel] - line) / unit)))
            assert (got[sel] >= np.minimum(a, b)).all() and (got[sel] <= np.maximum(a, b)).all()
            assert (got[m].view(np.uint64) == v[m].view(np.uint64)).all()
    print("worst distance to np.interp: %.3f spacings" % worst)
    assert 0 < worst <= 2 * INTERP_WORST


@pytest.mark.parametrize("how", ["nearest", "left", "right"])
def test_the_neighbours_are_the_ones_distance_finds(how):
    """a filled base i holds v[i - dl] or v[i + dr] for the dl, dr that `distance --to=left|right` gives"""
    rng = np.random.default_rng(17)
    for n in (1, 2, 17, 40, 333):
        for v in contents(n, rng):
            m = ref.known_bases(v)
            if not m.any():
                continue
            got = ref.fill_gaps(v, how=how, ends="keep")
            dl = distance_ref.distance(v, to="left").astype(np.int64)          # n where there is none
            dr = distance_ref.distance(v, to="right").astype(np.int64)
            idx = np.arange(n)
            have_l, have_r = dl < n, dr < n
            from_l = v[np.where(have_l, idx - dl, 0)]
            from_r = v[np.where(have_r, idx + dr, 0)]
            if how == "left":
                want = np.where(have_l, from_l, v)
            elif how == "right":
                want = np.where(have_r, from_r, v)
            else:
                want = np.where(have_l & have_r, np.where(dl <= dr, from_l, from_r), v)
            assert got.tobytes() == want.tobytes(), (n, how, v.tolist())
            ext = ref.fill_gaps(v, how=how)                                     # extended: whichever side exists
            want = np.where(have_l & have_r, want, np.where(have_l, from_l, from_r))
            assert ext.tobytes() == want.tobytes(), (n, how, v.tolist())


@pytest.mark.parametrize("G", [1, 2, 9])
def test_gaps_of_exactly_the_longest_and_one_more(G):
    for how, ends in itertools.product(ref.HOW, ref.ENDS):
        # an end gap of G, an interior gap of G+1, one of G, an end gap of G+1 -- and the mirror image
        v = np.concatenate((np.zeros(G), [2.0], np.zeros(G + 1), [4.0], np.zeros(G), [8.0], np.zeros(G + 1)))
        for w in (v, v[::-1].copy()):
            got = ref.fill_gaps(w, how=how, ends=ends, maxgap=G)
            free = ref.fill_gaps(w, how=how, ends=ends)
            assert got.tobytes() == ref.fill_gaps_loop(w, how=how, ends=ends, maxgap=G).tobytes()
            L, R = ref.neighbours(w != 0)
            long_gap = (w == 0) & (R - L - 1 > G)
            assert np.count_nonzero(long_gap) == 2 * (G + 1)
            assert (got[long_gap] == 0).all()                                   # one base too long: as it was
            assert got[~long_gap].tobytes() == free[~long_gap].tobytes()        # exactly G: as without a limit
            assert (free[(w == 0) & (L >= 0) & (R < w.size)] != 0).all()


def test_twice_is_once():
    """whenever nothing unknown is left (the filled values here are all above the threshold) a second pass finds no gap"""
    rng = np.random.default_rng(23)
    for n in (1, 5, 40, 333):
        for density in (0.5, 0.05):
            v = np.where(rng.random(n) < density, rng.random(n) + 0.5, 0.0)
            for how in ref.HOW:
                once = ref.fill_gaps(v, how=how)
                assert ref.fill_gaps(once, how=how).tobytes() == once.tobytes()
                if (v != 0).any():
                    assert ref.known_bases(once).all()
                for ends, maxgap in (("keep", None), ("extend", 3)):            # what stays unknown stays as it is, and again
                    some = ref.fill_gaps(v, how=how, ends=ends, maxgap=maxgap)
                    left = ~ref.known_bases(some)
                    assert some[left].tobytes() == v[left].tobytes()
