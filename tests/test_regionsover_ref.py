"""CPU: the exact checker of regionsover (tests/regionsover_ref.py) against fractions.Fraction on random cells and against
the properties of the definition, and the library's host entry gdsp_region_cell_bounds (no GPU) against Python integers.

The minus strand.  The definition is the mirror image about the region: body column k of a minus region is
[e - floor((k+1) L / B), e - floor(k L / B)).  Read backwards, that row is the plus row of the same region with U and D
swapped exactly when B divides L (and always on the flanks): when it does not, floor rounds towards the region's first
base, which for a minus region is its high end, so the wide and narrow body cells change places -- with L = 5 and B = 2
the plus cells are 2 and 3 bases, and so are the minus cells from e downwards.  What holds for every L is the mirror
itself: a minus row over v is the plus row over v reversed of the region mirrored, [n - e, n - s), with the same U and D.
Both are tested: the mirror for every L, the reversed row where B divides L and on every flank."""
import math
from fractions import Fraction

import numpy as np

import matrixover_ref as mref
import regionsover_ref as rref
import xsum_ref as ref


def fraction_figures(xs, lo, hi):
    xs = [float(x) for x in xs if math.isfinite(x) and not x < lo and not x > hi]
    if not xs:
        return (math.nan, 0.0, 0.0, math.nan, math.nan)
    total = sum((Fraction(x) for x in xs), Fraction(0))
    rounded = lambda q: 0.0 if q == 0 else q.numerator / q.denominator         # int / int is correctly rounded
    return (rounded(total / len(xs)), rounded(total), float(len(xs)), min(xs) + 0.0, max(xs) + 0.0)


def definition_cell(n, s, e, strand, U, B, D, b, j):
    """the issue's formulas written out per strand and per part of the row, not the checker's single mirror"""
    L, n_up = e - s, U // b
    if j < n_up:
        lo, hi = (s - U + j * b, s - U + (j + 1) * b) if strand > 0 else (e + U - (j + 1) * b, e + U - j * b)
    elif j < n_up + B:
        k = j - n_up
        lo, hi = (s + k * L // B, s + (k + 1) * L // B) if strand > 0 else (e - (k + 1) * L // B, e - k * L // B)
    else:
        k = j - n_up - B
        lo, hi = (e + k * b, e + (k + 1) * b) if strand > 0 else (s - (k + 1) * b, s - k * b)
    return max(lo, 0), min(hi, n)


SHAPES = ((4, 7, 8, 4), (0, 1, 0, 1), (6, 64, 0, 3), (0, 5, 10, 10), (3, 3, 3, 1))           # U, B, D, bin


def random_regions(rng, sizes, count):
    out = []
    for _ in range(count):
        c = int(rng.integers(0, len(sizes)))
        s = int(rng.integers(0, sizes[c]))
        out.append((c, s, int(rng.integers(s + 1, sizes[c] + 1)), int(rng.choice([1, -1]))))
    return out


def test_random_cells_against_fractions():
    rng = np.random.default_rng(1)
    v = [np.ldexp(rng.standard_normal(300), rng.integers(-40, 40, 300).astype(np.int32)), rng.integers(0, 9, 57).astype(np.float64),
         rng.standard_normal(7)]
    v[0][rng.integers(0, 300, 12)] = rng.choice([np.nan, np.inf, -np.inf, -0.0], 12)
    v[1][:6] = -0.0
    regions = random_regions(rng, [x.size for x in v], 40) + [(1, 0, 57, 1), (1, 0, 57, -1), (2, 0, 1, -1), (2, 6, 7, 1), (1, 0, 3, 1)]
    for (U, B, D, b), (lo, hi) in zip(SHAPES, ((-ref.DBL_MAX, ref.DBL_MAX), (-0.5, 2.0), (-ref.DBL_MAX, 1.0),
                                               (-ref.DBL_MAX, ref.DBL_MAX), (0.0, 0.0))):
        got = rref.figures(v, regions, B, U, D, b, lo, hi)
        for i, (c, s, e, t) in enumerate(regions):
            for j in range(rref.columns(U, B, D, b)):
                a, z = definition_cell(v[c].size, s, e, t, U, B, D, b, j)
                assert (a, z) == rref.cell_interval(v[c].size, s, e, t, U, B, D, b, j)
                want = fraction_figures(v[c][a:z] if a < z else [], lo, hi)
                for k, name in enumerate(rref.FIGURES):
                    assert ref.same(got[name][i, j], want[k]), (U, B, D, b, i, j, name, got[name][i, j], want[k])
        for name in rref.FIGURES:
            assert rref.same_bits(rref.matrix(v, regions, B, U, D, b, name, lo, hi), got[name])
    assert math.copysign(1.0, rref.matrix(v, [(1, 0, 3, 1)], 1, what="sum")[0, 0]) == 1.0          # three -0.0: +0.0
    assert math.copysign(1.0, rref.matrix(v, [(1, 0, 3, 1)], 1, what="max")[0, 0]) == 1.0


def test_the_body_cells_partition_the_region():
    n = 5000
    for L in (1, 2, 5, 7, 8, 9, 63, 64, 65, 1000, 4999, 5000):
        for B in (1, 2, 7, 8, 9, 64, 100, 16384):
            for strand in (1, -1):
                s = (n - L) // 2
                cells = [rref.cell_interval(n, s, s + L, strand, 0, B, 0, 1, k) for k in range(B)]
                if strand < 0:
                    cells = cells[::-1]
                assert cells[0][0] == s and cells[-1][1] == s + L
                assert all(cells[k][1] == cells[k + 1][0] for k in range(B - 1))
                widths = {z - a for a, z in cells}
                assert widths <= {L // B, -(-L // B)}, (L, B, widths)
                assert (0 in widths) == (L < B)


def test_a_minus_row_is_the_mirror_image():
    rng = np.random.default_rng(4)
    n = 200
    v = rng.standard_normal(n) * 7
    spans = [(0, 1), (0, 200), (17, 30), (100, 101), (150, 200), (3, 67), (60, 124), (80, 180)]
    for U, B, D, b in SHAPES + ((12, 10, 20, 4),):
        minus = rref.figures([v], [(0, s, e, -1) for s, e in spans], B, U, D, b)
        mirrored = rref.figures([v[::-1]], [(0, n - e, n - s, 1) for s, e in spans], B, U, D, b)
        swapped = rref.figures([v], [(0, s, e, 1) for s, e in spans], B, D, U, b)
        n_up = U // b
        for name in rref.FIGURES:
            assert rref.same_bits(minus[name], mirrored[name]), (U, B, D, b, name)
            back = swapped[name][:, ::-1]
            assert rref.same_bits(minus[name][:, :n_up], back[:, :n_up]) and rref.same_bits(minus[name][:, n_up + B:], back[:, n_up + B:])
            whole = [i for i, (s, e) in enumerate(spans) if (e - s) % B == 0]
            assert rref.same_bits(minus[name][whole], back[whole]), (U, B, D, b, name)
    assert not rref.same_bits(rref.matrix([v], [(0, 17, 30, -1)], 5), rref.matrix([v], [(0, 17, 30, 1)], 5))
    # L = 5, B = 2: the wide cell is the second one in the region's own direction on either strand
    assert [rref.cell_interval(n, 10, 15, 1, 0, 2, 0, 1, k) for k in (0, 1)] == [(10, 12), (12, 15)]
    assert [rref.cell_interval(n, 10, 15, -1, 0, 2, 0, 1, k) for k in (0, 1)] == [(13, 15), (10, 13)]


def test_unscaled_rows_are_matrixovers():
    """B == L with bin 1 is matrixover around the start over offsets -U .. L - 1 + D; L == B w with bin w is matrixover at
    bin w"""
    rng = np.random.default_rng(5)
    v = [rng.standard_normal(400) * 3, rng.integers(0, 60, 90).astype(np.float64)]
    for c, s, L, U, D in ((0, 100, 37, 20, 9), (0, 0, 50, 30, 0), (0, 350, 50, 0, 80), (1, 5, 80, 7, 7), (1, 0, 90, 3, 4)):
        got = rref.figures(v, [(c, s, s + L, 1)], L, U, D, 1)
        want = mref.figures(v, [(c, s, 1)], -U, U + L + D, 1)
        for name in rref.FIGURES:
            assert rref.same_bits(got[name], want[name]), (c, s, L, name)
    for c, s, B, w, U, D in ((0, 100, 10, 4, 20, 8), (0, 0, 7, 9, 18, 0), (0, 337, 9, 7, 0, 70), (1, 6, 8, 10, 10, 10)):
        got = rref.figures(v, [(c, s, s + B * w, 1)], B, U, D, w)
        want = mref.figures(v, [(c, s, 1)], -U, U + B * w + D, w)
        for name in rref.FIGURES:
            assert rref.same_bits(got[name], want[name]), (c, s, B, w, name)


# ------------------------------------------------------------------------- the library's host entry, no GPU ----

BIG = 2 ** 32 - 1


def bounds_cases():
    """(n, s, e, U, B, D, bin): L = 2^32 - 1 and L = 1 at the most columns, L = B +- 1, flanks that leave the chromosome"""
    return [(BIG, 0, BIG, 0, 16384, 0, 1), (BIG, BIG - 1, BIG, 0, 16384, 0, 1), (BIG, 2 ** 31 - 5, 2 ** 31 - 4, 0, 16384, 0, 1),
            (BIG, 1000, 1000 + 16385, 0, 16384, 0, 1), (BIG, 2 ** 31 - 8000, 2 ** 31 + 8383, 0, 16384, 0, 1),
            (BIG, 100, 2 ** 32 - 200, 1000, 8192, 2000, 50), (BIG, 2 ** 31 - 77, BIG, 512, 1001, 1024, 256),
            (1000, 10, 19, 16, 8, 32, 4), (1000, 10, 17, 16, 8, 32, 4), (1000, 990, 997, 16, 8, 32, 4), (5, 0, 5, 3, 2, 3, 1),
            (1, 0, 1, 2, 3, 2, 2)]


def test_region_cell_bounds_against_python_integers():
    import genodsp_amd as g
    for n, s, e, U, B, D, b in bounds_cases():
        ncols = rref.columns(U, B, D, b)
        n_up = U // b
        cols = sorted({0, ncols - 1, n_up, n_up + B - 1, max(0, n_up - 1), min(ncols - 1, n_up + B), n_up + B // 2, n_up + B // 3,
                       n_up + (2 * B) // 3, n_up + min(B - 1, 16383)})
        for strand in (1, -1):
            for j in cols:
                got = g.region_cell_bounds(n, s, e, strand, B, U, D, b, j)
                assert got == rref.cell_interval(n, s, e, strand, U, B, D, b, j), (n, s, e, strand, U, B, D, b, j, got)
    # every column of a few rows, the products k L past 2^32 and past 2^45
    for n, s, e, U, B, D, b in ((BIG, 0, BIG, 0, 16384, 0, 1), (BIG, 3, BIG - 7, 8, 1000, 12, 4), (300, 100, 163, 8, 64, 12, 4)):
        for strand in (1, -1):
            for j in range(0, rref.columns(U, B, D, b), 1 if B <= 1000 else 97):
                assert g.region_cell_bounds(n, s, e, strand, B, U, D, b, j) == rref.cell_interval(n, s, e, strand, U, B, D, b, j)
    assert g.region_cell_bounds(BIG, 0, BIG, 1, 16384, column=16383) == (16383 * BIG // 16384, BIG)
    assert g.region_cell_bounds(BIG, 0, BIG, -1, 16384, column=0) == (BIG - BIG // 16384, BIG)


def test_region_cell_bounds_refuses_what_is_not_a_row():
    import genodsp_amd as g
    for args in ((100, 10, 10, 1, 8), (100, 10, 101, 1, 8), (100, 20, 10, 1, 8), (100, 10, 20, 1, 0), (100, 10, 20, 1, 16385),
                 (100, 10, 20, 1, 8, 16385), (100, 10, 20, 1, 8, 6, 6, 4), (100, 10, 20, 1, 8, 0, 0, 0), (100, 10, 20, 1, 8, 8, 8, 1, 24),
                 (100, 10, 20, 1, 16000, 200, 200, 1)):
        try:
            g.region_cell_bounds(*args)
        except g.GdspError:
            continue
        raise AssertionError(args)
