"""matrixover (not in the reference) through the library: gdsp_matrix_rows_batch and gdsp_genome_matrix of
include/genodsp_hip.h.  Every value is exact and rounded once, so everything here is bit for bit (NaN equal to NaN) against
the literal checker tests/matrixover_ref.py -- itself held to fractions.Fraction in test_matrixover_ref.py -- for all five
figures, at the shapes where the kernel changes its route: bins of one base (the copy), below 16, below 64 and below 256
bases (the staged route, one lane, four or sixteen to a cell) and from 256 up (the wave strides over the cell); windows that leave either
end; chromosomes shorter than a cell; more rows than a launch takes; cells the device has to leave to the host.

The flagged cell.  A cell of 1e300, 1.0, -1e300 is NOT flagged by a two-term expansion: TwoSum keeps 1e300 and 1.0 in the
two terms and the third value cancels the first exactly, so the device finishes that cell itself (sum 1.0, mean 1/3, no
host cell).  The row is checked all the same, and the host path is pinned on 1e300, 1.0, 1e-300, three magnitudes two
terms cannot hold, where host cells >= 1 is required."""
import math

import numpy as np
import pytest

import anchor_cases as cases
import matrixover_ref as mref
import xsum_ref as ref
from anchor_cases import depth, dev, every_base, random_anchors, real, up

DBL_MAX = ref.DBL_MAX
FIGURES = mref.FIGURES


def check(g, d, v, anchors, off_lo, noffsets, bin, lo=-DBL_MAX, hi=DBL_MAX, what="", host=None, figures=FIGURES):
    """all figures of one shape against one pass of the checker; -> the checker's figures.  host: what the host may have
    finished (0: nothing; "some": at least a cell of the mean and of the sum; "few": no sum and at most a quarter of the
    means.  A mean goes to the host only on a tie or within 2^-40 of one, when the quotient is a power of two or at extreme
    exponents.  Exact ties are not rare at small counts -- a sum of 54 significant bits leaves e = ulp(s)/2, and a count n
    that divides s then makes (s + e) / n a midpoint: of the order of one cell in 2 n -- so the bound is a quarter, which
    holds for every n >= 3 (powers of two are decided outright) and which finishing only one-double sums on the device
    misses by far: three or more real values almost never add up to one double)"""
    want = mref.figures(v, anchors, off_lo, noffsets, bin, lo, hi)
    left = {}
    for name in figures:
        got = g.genome_matrix(d, anchors, off_lo, noffsets, bin=bin, what=name, lo=lo, hi=hi)
        last = g.genome_matrix_last()
        bad = [] if mref.same_bits(got, want[name]) else np.argwhere(~((got == want[name]) | (np.isnan(got) & np.isnan(want[name]))))[:3].tolist()
        print(what, name, "shape", got.shape, "host cells", last["host cells"], "launches", last["launches"])
        assert mref.same_bits(got, want[name]), (what, name, bad, [(got[i, j], want[name][i, j]) for i, j in bad])
        assert last["rows"] == len(anchors) and last["cells"] == len(anchors) * (noffsets // bin)
        left[name] = last["host cells"]
        if name in ("count", "min", "max") or host == 0:
            assert last["host cells"] == 0, (what, name, last)
    if host == "some":
        assert left["mean"] >= 1 and left["sum"] >= 1, (what, left)
    if host == "few":
        assert left["sum"] == 0 and left["mean"] * 4 <= len(anchors) * (noffsets // bin), (what, left)
    return want


# ------------------------------------------------------------------------------------------ shapes ----

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 5, 64, 3 * 512 + 7])
def test_vector_lengths(n):
    """an anchor at every base on both strands: windows that leave either end, chromosomes shorter than a cell"""
    g = dev()
    rng = np.random.default_rng(n)
    for k, (off_lo, noffsets, bin) in enumerate(((-8, 16, 1), (-8, 16, 4), (-8, 16, 16), (-512, 1024, 64))):
        make = depth if k % 2 == 0 else real
        v = [make(n, rng)]
        want = check(g, up(g, v), v, every_base(n), off_lo, noffsets, bin, what=(n, off_lo, bin), host=0 if make is depth else "few")
        assert want["count"].max() == min(n, bin) and want["count"].shape == (2 * n, noffsets // bin)


N = 75000


def ends_and_middle(rng, n=N):
    pos = np.concatenate([rng.integers(0, 4000, 20), rng.integers(n - 4000, n, 20), rng.integers(30000, 40000, 6), [0, n - 1, 1, n - 2]])
    return [(0, int(p), 1 if i % 2 else -1) for i, p in enumerate(pos)]


@pytest.mark.gpu
@pytest.mark.parametrize("bin", [1, 2, 3, 7, 10, 15, 16, 63, 64, 65, 100, 128, 255, 256, 257, 1000])
def test_bin_widths(bin):
    """two and five columns of each width, on depth (which the device finishes alone) and on reals"""
    g = dev()
    rng = np.random.default_rng(bin)
    anchors = ends_and_middle(rng)
    assert len(anchors) == 50
    for make in (depth, real):
        v = [make(N, rng)]
        d = up(g, v)
        for cols in (2, 5):
            noffsets = bin * cols
            check(g, d, v, anchors, -(noffsets // 2), noffsets, bin, what=(bin, cols, make.__name__), host=0 if make is depth else "few")


@pytest.mark.gpu
@pytest.mark.parametrize("bin", [16384, 8192, 1])
def test_the_most_offsets(bin):
    g = dev()
    rng = np.random.default_rng(bin)
    anchors = ends_and_middle(rng)
    for make in (depth, real):
        v = [make(N, rng)]
        check(g, up(g, v), v, anchors, -8000, 16384, bin, what=(bin, make.__name__), host=0 if make is depth else "few")


@pytest.mark.gpu
@pytest.mark.parametrize("off_lo", [-70000, 70000])
def test_far_offsets(off_lo):
    """cells no anchor reaches are empty: count 0, sum +0.0, the rest NaN"""
    g = dev()
    rng = np.random.default_rng(7)
    v = [real(N, rng)]
    d = up(g, v)
    anchors = ends_and_middle(rng)
    for noffsets, bin in ((16384, 128), (6000, 10), (6016, 32), (4000, 1)):
        want = check(g, d, v, anchors, off_lo, noffsets, bin, what=(off_lo, noffsets, bin))
        empty = want["count"] == 0
        assert empty.any() and not empty.all()
        assert np.isnan(want["mean"][empty]).all() and (want["sum"][empty].view(np.uint64) == 0).all()


@pytest.mark.gpu
def test_thirty_three_vectors():
    """one more than a launch sequence holds"""
    g = dev()
    rng = np.random.default_rng(33)
    sizes = [1, 2, 700] + [int(s) for s in rng.integers(1, 701, 30)]
    v = [real(n, rng) if i % 2 else depth(n, rng) for i, n in enumerate(sizes)]
    anchors = random_anchors(v, 400, rng) + [(c, 0, 1) for c in range(33)] + [(c, v[c].size - 1, -1) for c in range(33)]
    d = up(g, v)
    for off_lo, noffsets, bin in ((-30, 60, 1), (-30, 60, 6), (-30, 60, 20), (-100, 256, 128), (-300, 600, 300)):
        check(g, d, v, anchors, off_lo, noffsets, bin, what=("33", bin))
    assert g.genome_matrix_last()["launches"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 5000])
def test_numbers_of_anchors_seven_rows_a_launch(count):
    g = dev()
    rng = np.random.default_rng(count)
    v = [depth(2000, rng), real(301, rng)]
    anchors = random_anchors(v, count, rng)
    d = up(g, v)
    whole = {name: g.genome_matrix(d, anchors, -20, 40, bin=10, what=name) for name in FIGURES}
    g.matrix_set_launch_rows(7)
    try:
        check(g, d, v, anchors, -20, 40, 10, what=count)
        assert g.genome_matrix_last()["launches"] == (count + 6) // 7
        for name in FIGURES:
            got = g.genome_matrix(d, anchors, -20, 40, bin=10, what=name)
            assert got.shape == (count, 4) and mref.same_bits(got, whole[name]), name
    finally:
        g.matrix_set_launch_rows(0)
    assert g.genome_matrix_last()["rows"] == count


@pytest.mark.gpu
def test_order_duplicates_and_an_odd_alignment():
    g = dev()
    rng = np.random.default_rng(5)
    n = 3 * 512 + 7
    whole = real(n + 1, rng)
    buf = g.DeviceVector.from_numpy(whole)
    assert buf.ptr.value % 16 == 0
    v = [whole[1:], depth(900, rng)]
    d = [(buf, 1, n), g.DeviceVector.from_numpy(v[1])]
    anchors = random_anchors(v, 300, rng)
    anchors += anchors[:20]                                                   # duplicates: equal rows
    for off_lo, noffsets, bin in ((-100, 200, 1), (-100, 200, 8), (-100, 200, 25), (-300, 640, 64), (-600, 1280, 320)):
        want = check(g, d, v, anchors, off_lo, noffsets, bin, what=("odd", bin))
        perm = rng.permutation(len(anchors))
        for name in ("mean", "max"):
            got = g.genome_matrix(d, [anchors[i] for i in perm], off_lo, noffsets, bin=bin, what=name)
            assert mref.same_bits(got, want[name][perm]), (bin, name)
            swapped = g.genome_matrix(d[::-1], [(1 - c, p, s) for c, p, s in anchors], off_lo, noffsets, bin=bin, what=name)
            assert mref.same_bits(swapped, want[name]), (bin, name)
        assert mref.same_bits(want["mean"][:20], want["mean"][300:])


# ------------------------------------------------------------------------------------------ values ----

@pytest.mark.gpu
def test_limits_nan_inf_and_negative_zeros():
    g = dev()
    rng = np.random.default_rng(23)
    v = [depth(1500, rng), real(700, rng), np.full(300, -0.0)]
    for x in v[:2]:
        hit = rng.random(x.size) < 0.05
        x[hit] = rng.choice([np.nan, np.inf, -np.inf, -0.0], int(hit.sum()))
    v[2][100:110] = [np.nan, -0.0, np.inf, 0.0, -0.0, -np.inf, -0.0, 5e-324, -5e-324, -0.0]
    d = up(g, v)
    anchors = random_anchors(v, 200, rng) + [(2, p, s) for p in (0, 50, 104, 299) for s in (1, -1)]
    for lo, hi in ((-DBL_MAX, DBL_MAX), (1.0, 20.0), (5.0, 5.0), (100.0, 200.0), (-math.inf, math.inf), (-0.0, 0.0)):
        for off_lo, noffsets, bin in ((-12, 24, 1), (-12, 24, 4), (-32, 64, 32), (-96, 192, 64), (-300, 600, 300)):
            want = check(g, d, v, anchors, off_lo, noffsets, bin, lo, hi, what=(lo, hi, bin))
    zeros = mref.figures(v, [(2, 50, 1)], -12, 24, 4)                        # cells of nothing but -0.0
    for name in ("mean", "sum", "min", "max"):
        assert (zeros[name].view(np.uint64) == 0).all(), name
    assert (want["count"] >= 0).all()


@pytest.mark.gpu
def test_a_cell_two_terms_cannot_hold_goes_to_the_host():
    g = dev()
    v = [np.zeros(600)]
    v[0][10:13] = [1e300, 1.0, -1e300]                                       # (two terms hold this one: see the docstring)
    v[0][20:23] = [1e300, 1.0, 1e-300]
    v[0][200:203] = [1e300, 1.0, 1e-300]
    v[0][300:303] = [DBL_MAX, DBL_MAX, 1.0]                                  # the sum overflows, the mean does not
    d = up(g, v)
    for anchors, off_lo, noffsets, bin in (([(0, 10, 1), (0, 12, -1), (0, 20, 1), (0, 22, -1), (0, 300, 1)], 0, 3, 3),
                                           ([(0, 8, 1), (0, 25, -1)], 0, 18, 3), ([(0, 200, 1), (0, 263, -1), (0, 290, 1)], -64, 192, 64), ([(0, 200, 1), (0, 455, -1)], -256, 768, 256),
                                           ([(0, 16, 1), (0, 300, 1)], 0, 32, 16)):
        want = check(g, d, v, anchors, off_lo, noffsets, bin, what=("flagged", bin), host="some")
    assert want["sum"][1, 0] == math.inf and want["mean"][1, 0] < math.inf
    first = mref.figures(v, [(0, 10, 1)], 0, 3, 3)
    assert first["sum"][0, 0] == 1.0 and first["mean"][0, 0] == 1.0 / 3.0
    # the raw rows and the list: what the list names is what the host then computes, and nothing else is wrong
    anchors = [(0, 8, 1), (0, 25, -1)]
    rows, todo = g.matrix_rows(d, anchors, 0, 18, bin=3, what="sum")
    want = mref.matrix(v, anchors, 0, 18, 3, "sum")
    assert todo.size >= 2 and np.unique(todo).size == todo.size and todo.max() < 12
    keep = np.ones(12, bool)
    keep[todo] = False
    assert mref.same_bits(rows.ravel()[keep], want.ravel()[keep])
    rows, todo = g.matrix_rows(d, anchors, 0, 18, bin=3, what="max")
    assert todo.size == 0 and mref.same_bits(rows, mref.matrix(v, anchors, 0, 18, 3, "max"))


@pytest.mark.gpu
def test_host_cells_of_later_vectors_and_later_launches():
    """the cells the host finishes lie on the second and the third of three vectors and, two rows a launch, in the third
    launch and after it: each has to find its own vector, its own row there and its own interval"""
    g = dev()
    v = [depth(50, np.random.default_rng(3)), np.zeros(600), np.zeros(600)]
    for x in v[1:]:
        x[20:23] = [1e300, 1.0, 1e-300]
        x[200:203] = [1e300, 1.0, 1e-300]
    d = up(g, v)
    for anchors, off_lo, noffsets, bin in (([(0, 3, 1), (1, 8, 1), (0, 40, -1), (2, 25, -1), (0, 0, 1), (1, 25, -1), (0, 49, -1), (2, 8, 1), (0, 20, 1), (1, 300, 1)], 0, 18, 3),
                                           ([(0, 10, 1), (0, 30, -1), (2, 200, 1), (0, 45, 1), (1, 263, -1), (0, 5, -1), (1, 290, 1), (2, 263, -1), (0, 25, 1)], -64, 192, 64)):
        whole = {name: g.genome_matrix(d, anchors, off_lo, noffsets, bin=bin, what=name) for name in ("sum", "mean")}
        g.matrix_set_launch_rows(2)
        try:
            want = check(g, d, v, anchors, off_lo, noffsets, bin, what=("later", bin), host="some", figures=("sum", "mean"))
            assert g.genome_matrix_last()["launches"] == (len(anchors) + 1) // 2
            for name in ("sum", "mean"):
                got = g.genome_matrix(d, anchors, off_lo, noffsets, bin=bin, what=name)
                assert mref.same_bits(got, whole[name]), (bin, name)
        finally:
            g.matrix_set_launch_rows(0)
        # the cells the host finished are on the vectors behind the first, whose five rows fill the first two launches
        on = sorted({anchors[i][0] for i in np.argwhere(want["sum"] == 1e300)[:, 0]})
        assert on == [1, 2], on


@pytest.mark.gpu
def test_depth_needs_no_host():
    """an integer sum below 2^53 is one double: nothing may be left to the host, whatever the figure and the route"""
    g = dev()
    rng = np.random.default_rng(53)
    v = [rng.integers(0, 2 ** 31, 9000).astype(np.float64), depth(4000, rng)]
    d = up(g, v)
    anchors = random_anchors(v, 150, rng)
    for off_lo, noffsets, bin in ((-50, 100, 1), (-50, 100, 5), (-64, 128, 16), (-126, 252, 63), (-500, 1000, 250), (-512, 1024, 256), (-4096, 8192, 8192)):
        check(g, d, v, anchors, off_lo, noffsets, bin, what=("depth", bin), host=0)


@pytest.mark.gpu
def test_ties_of_the_mean():
    """three-base cells whose exact sums take two terms and whose means sit on, just above and just below a rounding
    boundary, both signs, at three scales: the exact checker decides the expected bits"""
    g = dev()
    u, t = 3 * 2.0 ** -53, 2.0 ** -104
    cells = []
    for scale in (1.0, 2.0 ** 600, 2.0 ** -600):
        for sign in (1.0, -1.0):
            for third in (u, u + t, u - t):
                cells.append([sign * scale * 1.0, sign * scale * 2.0, sign * scale * third])
    assert len(cells) == 18 and u + t != u and u - t != u
    v = [np.array(cells, np.float64).ravel()]
    anchors = [(0, 3 * i, 1) for i in range(18)] + [(0, 3 * i + 2, -1) for i in range(18)]
    want = check(g, up(g, v), v, anchors, 0, 3, 3, what="ties")
    # (1 + 2 + 3 2^-53) / 3 = 1 + 2^-53 exactly: half an ulp above 1, a tie that goes to even; tipped, it must not
    assert want["mean"][0, 0] == 1.0 and want["mean"][1, 0] == 1.0 + 2.0 ** -52 and want["mean"][2, 0] == 1.0
    assert want["mean"][3, 0] == -1.0 and want["mean"][4, 0] == -(1.0 + 2.0 ** -52)
    # the same cells inside wider windows, through the other routes
    wide = [np.concatenate([np.zeros(70), v[0], np.zeros(70)])]
    d = up(g, wide)
    for bin in (3, 18, 54):
        check(g, d, wide, [(0, 70, 1), (0, 70 + 53, -1)], 0, 54, bin, what=("ties", bin))
    check(g, d, wide, [(0, 0, 1), (0, 193, -1), (0, 70, 1)], 0, 512, 256, what=("ties", 256))


@pytest.mark.gpu
def test_against_interval_stats():
    """one shape, also against statsover's library call over the cells' intervals"""
    g = dev()
    rng = np.random.default_rng(200)
    v = [real(N, rng)]
    d = up(g, v)
    anchors = random_anchors(v, 200, rng)
    for bin in (10, 80):
        ncols = 2000 // bin
        got = {name: g.genome_matrix(d, anchors, -1000, 2000, bin=bin, what=name) for name in FIGURES}
        iv = [(i, j) + mref.cell_interval(N, p, s, -1000, bin, j) for i, (_, p, s) in enumerate(anchors) for j in range(ncols)]
        full = [(i, j, a, b) for i, j, a, b in iv if a < b]
        st = g.interval_stats(d[0], [a for _, _, a, _ in full], [b for _, _, _, b in full])
        want = {name: np.full((200, ncols), 0.0 if name in ("sum", "count") else np.nan) for name in FIGURES}
        rows, cols = np.array([i for i, _, _, _ in full]), np.array([j for _, j, _, _ in full])
        for name in FIGURES:
            want[name][rows, cols] = st[name].astype(np.float64)
            assert mref.same_bits(got[name], want[name]), (bin, name)
        assert len(full) < len(iv)                                            # (some windows leave the chromosome)
        lit = mref.figures(v, anchors[:25], -1000, 2000, bin)
        for name in FIGURES:
            assert mref.same_bits(got[name][:25], lit[name]), (bin, name)


@pytest.mark.gpu
def test_what_is_refused():
    g = dev()
    v = up(g, [np.arange(100, dtype=np.float64)])
    ok = [(0, 50, 1)]
    for args in ((ok, 0, 10, 3), (ok, 0, 10, 0), (ok, 0, 0, 1), (ok, 0, 16385, 1), (ok, 2 ** 31 - 5, 10, 1),
                 ([(0, 100, 1)], 0, 10, 1), (ok + [(0, 2 ** 32 - 1, -1)], 0, 10, 1)):
        with pytest.raises(g.GdspError):
            g.genome_matrix(v, *args)
        with pytest.raises(g.GdspError):
            g.matrix_rows(v, *args)
    with pytest.raises(g.GdspError):
        g.genome_matrix(v, ok, 0, 10, 1, what=5)
    with pytest.raises(g.GdspError):
        g.matrix_rows(v, ok * 70 + [(0, 100, -1)], 0, 10, 1)
    assert g.genome_matrix(v, ok, 2 ** 31 - 10, 10, what="count").tolist() == [[0.0] * 10]   # (the last offset is INT32_MAX)
    assert g.genome_matrix(v, ok, -3, 6, 2, what="sum").tolist() == [[47.0 + 48.0, 49.0 + 50.0, 51.0 + 52.0]]
    assert g.genome_matrix(v, [(0, 50, -1)], -3, 6, 2, what="sum").tolist() == [[53.0 + 52.0, 51.0 + 50.0, 49.0 + 48.0]]


@pytest.mark.gpu
def test_the_anchor_check_sees_every_anchor():
    """the device's check of matrix_rows (genome_matrix refuses on the host before it): a bad last anchor among one
    thread's, one workgroup's, the next workgroup's, and where only the check's stride loop reaches it"""
    g = dev()
    v = up(g, [np.arange(cases.CHECK_N, dtype=np.float64)])
    most = cases.CHECK_COUNTS[-1]
    rows, todo = g.matrix_rows(v, cases.check_anchors(most), 0, 1, 1)
    assert most == 262145 and rows.shape == (most, 1) and np.all(rows == 50.0) and todo.size == 0
    for count in cases.CHECK_COUNTS:
        with pytest.raises(g.GdspError):
            g.matrix_rows(v, cases.check_anchors(count, bad_last=True), 0, 1, 1)
