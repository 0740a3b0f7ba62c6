"""CPU: the proof that the method of the 2^32 - 1 tests is sound (u32max_cases.py).  Those tests never run a checker over
the whole chromosome: they run it over a regenerated window plus a halo and compare the window's M bases.  Here the same
checkers, halos, signals and place rule run on a vector short enough to check whole (n = 50 000, its middle standing for
base 2^31), and for every case of group A

    checker(window + halo)[window]  ==  checker(whole vector)[window]      bit for bit, at every place,

the vector's two ends included, where windows are cut off.  With this a mismatch on the device means the kernel."""
import numpy as np
import pytest

from conftest import bits_equal
from oracle import cpu

import u32max_cases as U

FAKE_N = 50000


def fake_places():
    return U.places(FAKE_N, U.M, FAKE_N // 2)


def test_places_hold_what_they_must():
    """both ends, either side of the middle and, below the top, the last seam of every tiling -- the fixed ones and every
    one the library reports -- inside a window, with bases on both sides of it; at the real length too"""
    for n, mid in ((FAKE_N, FAKE_N // 2), (U.N, 2 ** 31)):
        p = U.places(n, U.M, mid)
        assert 0 in p and n - U.M in p and mid in p and mid - U.M // 2 in p
        assert all(0 <= s <= n - U.M for s in p)
        for tile in U.seam_tiles():
            seam = (n // tile) * tile
            if U.M <= seam <= n - U.M:
                assert any(s < seam - 1 and seam + 1 < s + U.M for s in p), tile
    assert set((2304, 2294, 3984, 4096, 8192, 16384, 32768, 1 << 18)) <= set(U.seam_tiles())
    assert len(set(U.seam_tiles())) > 8                                 # the library's own queries answered
    assert len(U.places()) == len(set(U.places()))


@pytest.fixture(scope="module")
def whole():
    """the whole short vector of each (chromosome index, mode), generated once"""
    return {(c, m): cpu.synth_coverage(U.SEED, c, 0, FAKE_N, m) for c in (U.CHROM, U.TRACK_CHROM) for m in (0, 1)}


def test_regenerated_windows_are_the_signal(whole):
    for mode in (0, 1):
        for s in fake_places():
            x, left = U.regenerate(s, U.M, 777, mode, FAKE_N)
            assert bits_equal(x[left:left + U.M], whole[(U.CHROM, mode)][s:s + U.M])


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_window_and_halo_give_what_the_whole_vector_gives(name, whole):
    case = U.CASES[name]
    tracks = [whole[(c, case.mode)] for c in (U.CHROM, U.TRACK_CHROM)[:case.tracks]]
    full = case.check(tracks)
    assert full.shape == (FAKE_N,)
    seen_end = False
    for p in fake_places():
        s, count = case.window(p, FAKE_N)
        assert s <= p and s + count >= p + U.M
        seen_end |= (s + count == FAKE_N)
        got = case.expected(s, count, FAKE_N)
        assert bits_equal(got, full[s:s + count]), (name, p, int(np.flatnonzero(got != full[s:s + count])[0]))
    assert seen_end
    # the case is worth running: the result is neither constant nor the input
    assert np.unique(full).size >= 2 and not bits_equal(full, tracks[0])


def test_the_sparse_set_has_gaps_on_both_sides_of_the_limit(whole):
    """distance cap=1000 and fillgaps maxgap=1000 see bases nearer and farther than 1000 from a member, and gaps shorter
    and longer than 1000, in the windows compared"""
    import fillgaps_ref
    x = whole[(U.CHROM, 1)]
    L, R = fillgaps_ref.neighbours(fillgaps_ref.known_bases(x, U.T_SPARSE))
    gap = (R - L - 1)[(L >= 0) & (R < FAKE_N) & (R > L)]
    assert (gap > 1000).any() and ((gap > 0) & (gap <= 1000)).any()
