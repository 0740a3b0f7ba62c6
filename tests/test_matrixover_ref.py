"""CPU: the exact checker of matrixover (tests/matrixover_ref.py) against fractions.Fraction on random cells, against
profileover's checker column by column on integer data, and against its own mirror image."""
import math
from fractions import Fraction

import numpy as np

import matrixover_ref as mref
import profileover_ref as pref
import xsum_ref as ref


def fraction_cell(v, p, s, off_lo, bin, j, lo, hi):
    """the cell's figures from the definition: a loop over its offsets, sums in Fraction"""
    xs = []
    for k in range(off_lo + j * bin, off_lo + (j + 1) * bin):
        g = p + s * k
        if 0 <= g < len(v) and math.isfinite(v[g]) and not v[g] < lo and not v[g] > hi:
            xs.append(float(v[g]))
    if not xs:
        return (math.nan, 0.0, 0.0, math.nan, math.nan)
    total = sum((Fraction(x) for x in xs), Fraction(0))
    rounded = lambda q: 0.0 if q == 0 else q.numerator / q.denominator         # int / int is correctly rounded
    return (rounded(total / len(xs)), rounded(total), float(len(xs)), min(xs) + 0.0, max(xs) + 0.0)


def test_random_cells_against_fractions():
    rng = np.random.default_rng(1)
    v = [np.ldexp(rng.standard_normal(400), rng.integers(-40, 40, 400).astype(np.int32)), rng.integers(0, 9, 57).astype(np.float64),
         rng.standard_normal(7)]
    v[0][rng.integers(0, 400, 12)] = rng.choice([np.nan, np.inf, -np.inf, -0.0], 12)
    v[1][:6] = -0.0
    anchors = [(c, int(rng.integers(0, v[c].size)), int(rng.choice([1, -1]))) for c in rng.integers(0, 3, 60)]
    anchors += [(1, 0, 1), (1, 0, -1), (1, 56, 1), (1, 56, -1), (1, 2, 1)]
    for off_lo, noffsets, bin, lo, hi in ((-9, 24, 3, -ref.DBL_MAX, ref.DBL_MAX), (-30, 60, 1, -0.5, 2.0), (3, 40, 40, -ref.DBL_MAX, 1.0),
                                          (-500, 600, 100, -ref.DBL_MAX, ref.DBL_MAX)):
        got = mref.figures(v, anchors, off_lo, noffsets, bin, lo, hi)
        for i, (c, p, s) in enumerate(anchors):
            for j in range(noffsets // bin):
                want = fraction_cell(v[c], p, s, off_lo, bin, j, lo, hi)
                for k, name in enumerate(mref.FIGURES):
                    assert ref.same(got[name][i, j], want[k]), (off_lo, bin, i, j, name, got[name][i, j], want[k])
        for name in mref.FIGURES:
            assert mref.same_bits(mref.matrix(v, anchors, off_lo, noffsets, bin, name, lo, hi), got[name])
    assert math.copysign(1.0, mref.matrix(v, [(1, 2, 1)], 0, 3, 3, "sum")[0, 0]) == 1.0          # three -0.0: +0.0
    assert math.copysign(1.0, mref.matrix(v, [(1, 2, 1)], 0, 3, 3, "max")[0, 0]) == 1.0


def test_one_base_cells_take_the_short_way_to_the_same_bits():
    rng = np.random.default_rng(2)
    v = [rng.standard_normal(90)]
    v[0][[3, 9, 40]] = [-0.0, np.nan, np.inf]
    anchors = [(0, int(p), s) for p in (0, 5, 44, 89) for s in (1, -1)]
    for lo, hi in ((-ref.DBL_MAX, ref.DBL_MAX), (-0.3, 0.8)):
        short = mref.figures(v, anchors, -50, 100, 1, lo, hi)
        literal = mref.figures(v, anchors, -50, 100, 1, lo, hi, literal=True)
        for name in mref.FIGURES:
            assert mref.same_bits(short[name], literal[name]), name


def test_columns_summed_over_rows_are_profileovers_on_integer_data():
    """integer data: a column's count and sum are the plain sums of its cells' (every partial sum is an exact integer)"""
    rng = np.random.default_rng(3)
    v = [rng.integers(0, 60, 300).astype(np.float64), rng.integers(0, 9, 41).astype(np.float64)]
    anchors = [(c, int(rng.integers(0, v[c].size)), int(rng.choice([1, -1]))) for c in rng.integers(0, 2, 120)]
    for off_lo, noffsets, bin in ((-20, 48, 1), (-20, 48, 4), (-70, 140, 35)):
        m = mref.figures(v, anchors, off_lo, noffsets, bin)
        prof = pref.profile(v, anchors, off_lo, noffsets, bin=bin)
        count, total = m["count"].sum(axis=0), m["sum"].sum(axis=0)
        assert count.tobytes() == np.array([f[0] for f in prof], np.float64).tobytes()
        assert total.tobytes() == np.array([f[1] for f in prof], np.float64).tobytes()


def test_a_minus_row_is_the_plus_row_over_the_mirrored_window_reversed():
    rng = np.random.default_rng(4)
    v = [rng.standard_normal(200) * 7]
    pos = [0, 1, 17, 100, 198, 199]
    for off_lo, noffsets, bin in ((-12, 30, 1), (-12, 30, 5), (40, 60, 20), (-150, 64, 64)):
        minus = mref.figures(v, [(0, p, -1) for p in pos], off_lo, noffsets, bin)
        plus = mref.figures(v, [(0, p, 1) for p in pos], -(off_lo + noffsets - 1), noffsets, bin)
        for name in mref.FIGURES:
            assert mref.same_bits(minus[name], plus[name][:, ::-1]), (off_lo, bin, name)
    assert not mref.same_bits(mref.matrix(v, [(0, 100, -1)], -12, 30, 5), mref.matrix(v, [(0, 100, 1)], -12, 30, 5))
