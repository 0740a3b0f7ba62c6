"""regionsover (not in the reference) through the library: gdsp_region_rows_batch and gdsp_genome_regions of
include/genodsp_hip.h.  Every value is exact and rounded once, so everything here is bit for bit (NaN equal to NaN) against
the literal checker tests/regionsover_ref.py -- itself held to fractions.Fraction in test_regionsover_ref.py -- for all
five figures, at the smallest shapes that reach each way the kernel can go wrong: the widest body cell ceil(L / B) on
either side of every route seam (1: the copy; below 16, 64 and 256: the staged route with one, four and sixteen lanes to
a cell; from 256: the wave strides), with both widths of a row on either side of a seam; regions shorter than their
columns; a last stretch that is partial, full and one cell over; flanks of every route that leave the chromosome at both
ends; more vectors than a table and more rows than a launch; the cells the device leaves to the host; the device's check
of the regions; and a chromosome of 2^32 - 1 bases.

The host cells.  The finish of a cell is matrixover's (gdsp_matrix_cell.h), so the conditions of test_matrixover.py carry
over unchanged: none on depth, none ever for count, min and max, and on reals no sum cell and at most a quarter of the
mean cells (its docstring has the argument).  The host path is pinned on a cell of 1e300, 1.0, 1e-300 as it is there."""
import numpy as np
import pytest

import anchor_cases as cases
import regionsover_ref as rref
import xsum_ref as ref
from anchor_cases import depth, dev, real, up

DBL_MAX = ref.DBL_MAX
FIGURES = rref.FIGURES


def check(g, d, v, regions, B, U=0, D=0, bin=1, lo=-DBL_MAX, hi=DBL_MAX, what="", host=None, figures=FIGURES):
    """all figures of one shape against one pass of the checker; -> the checker's figures.  host: what the host may have
    finished (0: nothing; "some": at least a cell of the mean and of the sum; "few": no sum and at most a quarter of the
    means -- test_matrixover.check has the argument)"""
    want = rref.figures(v, regions, B, U, D, bin, lo, hi)
    ncols = rref.columns(U, B, D, bin)
    left = {}
    for name in figures:
        got = g.genome_regions(d, regions, B, U, D, bin, what=name, lo=lo, hi=hi)
        last = g.genome_regions_last()
        bad = [] if rref.same_bits(got, want[name]) else np.argwhere(~((got == want[name]) | (np.isnan(got) & np.isnan(want[name]))))[:3].tolist()
        print(what, name, "shape", got.shape, "host cells", last["host cells"], "launches", last["launches"])
        assert rref.same_bits(got, want[name]), (what, name, bad, [(got[i, j], want[name][i, j]) for i, j in bad])
        assert last["rows"] == len(regions) and last["cells"] == len(regions) * ncols
        left[name] = last["host cells"]
        if name in ("count", "min", "max") or host == 0:
            assert last["host cells"] == 0, (what, name, last)
    if host == "some":
        assert left["mean"] >= 1 and left["sum"] >= 1, (what, left)
    if host == "few":
        assert left["sum"] == 0 and left["mean"] * 4 <= len(regions) * ncols, (what, left)
    return want


N = 40000


def spread(rng, L, count, n=N, c=0):
    """count regions of L bases on both strands: at base 0, up to base n, and in between"""
    starts = [0, n - L] + [int(s) for s in rng.integers(0, n - L + 1, max(0, count - 2))]
    return [(c, s, s + L, 1 if i % 2 else -1) for i, s in enumerate(starts[:count])]


# ------------------------------------------------------------------------------------------ shapes ----

@pytest.mark.gpu
@pytest.mark.parametrize("w", [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000])
def test_route_seams_of_the_body(w):
    """B = 8 and the widest cell w: L = 8 w has every cell w wide; L = 8 (w - 1) + 1 and 8 (w - 1) + 7 have cells of
    w - 1 and w bases in one row, and L = 8 w + 1 and 8 w + 7 cells of w and w + 1 -- both sides of 16, 64 and 256"""
    g = dev()
    rng = np.random.default_rng(w)
    B = 8
    lengths = [B * w, B * w + 1, B * w + B - 1] + ([B * (w - 1) + 1, B * (w - 1) + B - 1] if w > 1 else [])
    regions = [r for L in lengths for r in spread(rng, L, 6)]
    for make in (depth, real):
        v = [make(N, rng)]
        d = up(g, v)
        want = check(g, d, v, regions, B, what=(w, make.__name__), host=0 if make is depth else "few")
        widths = set(want["count"].ravel().tolist())                          # (every base is sampled: a count is a width)
        assert float(w) in widths and widths <= {float(w - 1), float(w), float(w + 1)}, widths
        check(g, d, v, regions[::5], B, 6, 9, 3, what=(w, "flanked", make.__name__), host=0 if make is depth else "few")


@pytest.mark.gpu
def test_regions_shorter_than_their_columns():
    g = dev()
    rng = np.random.default_rng(8)
    v = [depth(3000, rng), real(3000, rng)]
    d = up(g, v)
    regions = [(c, s, s + L, t) for c in (0, 1) for L in (1, 2, 5) for s in (0, 1500, 3000 - L) for t in (1, -1)]
    want = check(g, d, v, regions, 8, what="L < B")
    assert (want["count"].sum(axis=1) == [e - s for _, s, e, _ in regions]).all() and set(want["count"].ravel().tolist()) == {0.0, 1.0}
    assert np.isnan(want["mean"][want["count"] == 0]).all() and (want["sum"][want["count"] == 0].view(np.uint64) == 0).all()
    check(g, d, v, regions, 8, 4, 4, 2, what="L < B, flanked")
    # one cell full, the rest empty
    ones = [(0, 7, 8, 1), (1, 2999, 3000, -1)]
    want = check(g, d, v, ones, 16384, what="L = 1")
    assert (want["count"].sum(axis=1) == 1).all() and want["count"][0, 16383] == 1 and want["count"][1, 16383] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("w,columns", [(3, (63, 64, 65, 130)), (20, (15, 16, 17)), (100, (3, 4, 5))])
def test_stretch_seams(w, columns):
    """a stretch is 64, 16 or 4 cells: a last stretch that is partial, full, and one cell over"""
    g = dev()
    rng = np.random.default_rng(w)
    for make in (depth, real):
        v = [make(N, rng)]
        d = up(g, v)
        for B in columns:
            regions = spread(rng, B * w, 4) + spread(rng, B * w - 1, 2) + spread(rng, B * (w - 1) + 1, 2)
            check(g, d, v, regions, B, what=(w, B, make.__name__), host=0 if make is depth else "few")


@pytest.mark.gpu
@pytest.mark.parametrize("bin", [1, 4, 16, 256])
def test_flanks(bin):
    """U != D, every route of a flank; regions at base 0 and up to base n, so that both flanks leave the chromosome; the
    whole chromosome as one region"""
    g = dev()
    rng = np.random.default_rng(bin)
    n = 9000
    for make in (depth, real):
        v = [make(n, rng)]
        d = up(g, v)
        regions = [(0, 0, 700, 1), (0, 0, 700, -1), (0, n - 333, n, 1), (0, n - 333, n, -1), (0, 0, n, 1), (0, 0, n, -1),
                   (0, 100, 300, 1), (0, n - 600, n - 500, -1), (0, 4000, 4777, 1), (0, 4000, 4777, -1)]
        want = check(g, d, v, regions, 10, 512, 1024, bin, what=(bin, make.__name__), host=0 if make is depth else "few")
        nu, nd = 512 // bin, 1024 // bin
        assert (want["count"][0, :nu] == 0).all() and (want["count"][1, -nd:] == 0).all()          # below base 0: upstream, or a minus region's downstream
        assert (want["count"][2, -nd:] == 0).all() and (want["count"][3, :nu] == 0).all()          # beyond base n
        assert (want["count"][4, nu:nu + 10] == n // 10).all() and want["count"][4].sum() == n
        assert np.isnan(want["max"][0, 0]) and not np.isnan(want["max"][8]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_short_chromosomes(n):
    g = dev()
    rng = np.random.default_rng(n)
    for k, (B, U, D, bin) in enumerate(((1, 0, 0, 1), (3, 4, 8, 1), (8, 8, 16, 4), (2, 32, 16, 16), (5, 512, 256, 256))):
        make = depth if k % 2 == 0 else real
        v = [make(n, rng)]
        regions = [(0, s, e, t) for s in range(n) for e in range(s + 1, n + 1) for t in (1, -1)][:160]
        want = check(g, up(g, v), v, regions, B, U, D, bin, what=(n, B, bin), host=0 if make is depth else "few")
        assert want["count"].sum(axis=1).max() == n


@pytest.mark.gpu
def test_thirty_three_vectors():
    """one more than a launch sequence holds, with regions in the first, the 32nd and the 33rd"""
    g = dev()
    rng = np.random.default_rng(33)
    sizes = [700, 1, 2] + [int(s) for s in rng.integers(1, 701, 28)] + [650, 700]
    v = [real(n, rng) if i % 2 else depth(n, rng) for i, n in enumerate(sizes)]
    assert len(v) == 33
    regions = []
    for c in [0, 31, 32] + [int(c) for c in rng.integers(0, 33, 150)]:
        s = int(rng.integers(0, v[c].size))
        regions.append((c, s, int(rng.integers(s + 1, v[c].size + 1)), int(rng.choice([1, -1]))))
    regions += [(c, 0, v[c].size, t) for c in (0, 31, 32) for t in (1, -1)]
    d = up(g, v)
    for B, U, D, bin in ((6, 0, 0, 1), (20, 30, 12, 6), (3, 40, 20, 20), (2, 256, 0, 256)):
        check(g, d, v, regions, B, U, D, bin, what=("33", B, bin))
    assert g.genome_regions_last()["launches"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1000])
def test_numbers_of_regions_seven_rows_a_launch(count):
    """several launches; the rows come back in the caller's order whatever vector each is on"""
    g = dev()
    rng = np.random.default_rng(count)
    v = [depth(2000, rng), real(301, rng)]
    regions = []
    for c in rng.integers(0, 2, count).tolist():
        s = int(rng.integers(0, v[c].size))
        regions.append((c, s, int(rng.integers(s + 1, min(v[c].size, s + 400) + 1)), int(rng.choice([1, -1]))))
    d = up(g, v)
    whole = {name: g.genome_regions(d, regions, 5, 20, 10, 10, what=name) for name in FIGURES}
    g.regions_set_launch_rows(7)
    try:
        check(g, d, v, regions, 5, 20, 10, 10, what=count)
        assert g.genome_regions_last()["launches"] == (count + 6) // 7
        for name in FIGURES:
            got = g.genome_regions(d, regions, 5, 20, 10, 10, what=name)
            assert got.shape == (count, 8) and rref.same_bits(got, whole[name]), name
        if count > 1:
            perm = rng.permutation(count)
            got = g.genome_regions(d, [regions[i] for i in perm], 5, 20, 10, 10, what="mean")
            assert rref.same_bits(got, whole["mean"][perm])
            swapped = g.genome_regions(d[::-1], [(1 - c, s, e, t) for c, s, e, t in regions], 5, 20, 10, 10, what="mean")
            assert rref.same_bits(swapped, whole["mean"])
    finally:
        g.regions_set_launch_rows(0)
    assert g.genome_regions_last()["rows"] == count


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
    regions = []
    for c in rng.integers(0, 3, 60).tolist():
        s = int(rng.integers(0, v[c].size))
        regions.append((c, s, int(rng.integers(s + 1, v[c].size + 1)), int(rng.choice([1, -1]))))
    regions += [(2, 98, 112, 1), (2, 98, 112, -1), (2, 0, 300, 1)]
    for lo, hi in ((-DBL_MAX, DBL_MAX), (1.0, 20.0), (5.0, 5.0), (100.0, 200.0), (-np.inf, np.inf), (-0.0, 0.0)):
        for B, U, D, bin in ((7, 0, 0, 1), (14, 6, 6, 2), (3, 64, 32, 32)):
            check(g, d, v, regions, B, U, D, bin, lo, hi, what=(lo, hi, B))
    zeros = rref.figures(v, [(2, 0, 90, 1)], 9, 8, 8, 4)                      # cells of nothing but -0.0
    for name in ("mean", "sum", "min", "max"):
        assert (zeros[name][:, 2:].view(np.uint64) == 0).all(), name


@pytest.mark.gpu
def test_a_cell_two_terms_cannot_hold_goes_to_the_host():
    g = dev()
    v = [np.zeros(3000)]
    for at in (20, 200, 1000, 2000):
        v[0][at:at + 3] = [1e300, 1.0, 1e-300]                               # three magnitudes two terms cannot hold
    v[0][300:303] = [DBL_MAX, DBL_MAX, 1.0]                                   # the sum overflows, the mean does not
    d = up(g, v)
    for regions, B, U, D, bin in (([(0, 20, 23, 1), (0, 20, 23, -1), (0, 300, 303, 1)], 1, 0, 0, 1),          # one cell of three bases
                                  ([(0, 14, 32, 1), (0, 11, 29, -1)], 6, 6, 6, 3),                            # G = 1
                                  ([(0, 180, 280, 1), (0, 150, 250, -1), (0, 290, 340, 1)], 2, 40, 40, 20),   # G = 4
                                  ([(0, 900, 1300, 1), (0, 1900, 2300, -1)], 4, 0, 0, 1),                     # G = 16
                                  ([(0, 500, 1500, 1), (0, 1600, 2600, -1)], 2, 512, 512, 256)):             # the wave strides
        want = check(g, d, v, regions, B, U, D, bin, what=("flagged", B, bin), host="some")
    assert np.isinf(rref.matrix(v, [(0, 300, 303, 1)], 1, what="sum")[0, 0]) and rref.matrix(v, [(0, 300, 303, 1)], 1)[0, 0] < np.inf
    # the raw rows and the list: what the list names is what the host then computes, and nothing else is wrong
    regions = [(0, 14, 32, 1), (0, 11, 29, -1), (0, 400, 418, 1)]
    rows, todo = g.regions_rows(d, regions, 6, 6, 6, 3, what="sum")
    want = rref.matrix(v, regions, 6, 6, 6, 3, "sum")
    ncols = 10
    flagged = sorted(i * ncols + j for i in (0, 1) for j in range(ncols) if want[i, j] == 1e300)
    assert len(flagged) == 2 and sorted(todo.tolist()) == flagged             # row * ncols + column, each once
    keep = np.ones(3 * ncols, bool)
    keep[todo] = False
    assert rref.same_bits(rows.ravel()[keep], want.ravel()[keep])
    rows, todo = g.regions_rows(d, regions, 6, 6, 6, 3, what="max")
    assert todo.size == 0 and rref.same_bits(rows, rref.matrix(v, regions, 6, 6, 6, 3, "max"))


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
    for regions, B, U, D, bin in (([(0, 3, 9, 1), (1, 14, 32, 1), (0, 30, 50, -1), (2, 11, 29, -1), (0, 0, 1, 1), (1, 11, 29, -1), (0, 40, 47, -1), (2, 14, 32, 1), (0, 20, 21, 1), (1, 300, 330, 1)], 6, 6, 6, 3),
                                  ([(0, 10, 40, 1), (0, 0, 50, -1), (2, 180, 280, 1), (0, 45, 50, 1), (1, 150, 250, -1), (0, 5, 9, -1), (1, 290, 340, 1), (2, 150, 250, -1), (0, 25, 26, 1)], 2, 40, 40, 20)):
        whole = {name: g.genome_regions(d, regions, B, U, D, bin, what=name) for name in ("sum", "mean")}
        g.regions_set_launch_rows(2)
        try:
            want = check(g, d, v, regions, B, U, D, bin, what=("later", B, bin), host="some", figures=("sum", "mean"))
            assert g.genome_regions_last()["launches"] == (len(regions) + 1) // 2
            for name in ("sum", "mean"):
                got = g.genome_regions(d, regions, B, U, D, bin, what=name)
                assert rref.same_bits(got, whole[name]), (B, name)
        finally:
            g.regions_set_launch_rows(0)
        # the cells the host finished are on the vectors behind the first, whose five rows fill the first two launches
        on = sorted({regions[i][0] for i in np.argwhere(want["sum"] == 1e300)[:, 0]})
        assert on == [1, 2], on


@pytest.mark.gpu
def test_depth_needs_no_host():
    """an integer sum below 2^53 is one double: nothing may be left to the host, whatever the figure and the route"""
    g = dev()
    rng = np.random.default_rng(53)
    v = [rng.integers(0, 2 ** 31, 9000).astype(np.float64), depth(4000, rng)]
    d = up(g, v)
    regions = []
    for c in rng.integers(0, 2, 80).tolist():
        s = int(rng.integers(0, v[c].size))
        regions.append((c, s, int(rng.integers(s + 1, v[c].size + 1)), int(rng.choice([1, -1]))))
    for B, U, D, bin in ((1, 0, 0, 1), (5, 50, 50, 5), (40, 64, 128, 16), (100, 126, 63, 63), (7, 512, 256, 256), (1000, 0, 0, 1)):
        check(g, d, v, regions, B, U, D, bin, what=("depth", B, bin), host=0)


@pytest.mark.gpu
def test_against_interval_stats():
    """one shape, also against statsover's library call over the cells' intervals"""
    g = dev()
    rng = np.random.default_rng(200)
    n = 30000
    v = [real(n, rng)]
    d = up(g, v)
    regions = [(0, 0, 900, 1), (0, n - 450, n, -1)]
    for _ in range(100):
        s = int(rng.integers(0, n - 1))
        regions.append((0, s, int(rng.integers(s + 1, min(n, s + 3000) + 1)), int(rng.choice([1, -1]))))
    B, U, D, bin = 25, 200, 100, 20
    ncols = rref.columns(U, B, D, bin)
    got = {name: g.genome_regions(d, regions, B, U, D, bin, what=name) for name in FIGURES}
    iv = [(i, j) + rref.cell_interval(n, s, e, t, U, B, D, bin, j) for i, (_, s, e, t) in enumerate(regions) for j in range(ncols)]
    full = [(i, j, a, z) for i, j, a, z in iv if a < z]
    st = g.interval_stats(d[0], [a for _, _, a, _ in full], [z for _, _, _, z in full])
    rows, cols = np.array([i for i, _, _, _ in full]), np.array([j for _, j, _, _ in full])
    for name in FIGURES:
        want = np.full((len(regions), ncols), 0.0 if name in ("sum", "count") else np.nan)
        want[rows, cols] = st[name].astype(np.float64)
        assert rref.same_bits(got[name], want), name
    assert len(full) < len(iv)                                                # (flanks leave the chromosome, short regions leave cells empty)


# ------------------------------------------------------------------------------------- what is refused ----

@pytest.mark.gpu
def test_what_is_refused():
    g = dev()
    v = up(g, [np.arange(100, dtype=np.float64)])
    ok = [(0, 40, 60, 1)]
    for args in ((ok, 0), (ok, 16385), (ok, 8, 16385, 0), (ok, 8, 0, 16385), (ok, 8, 6, 6, 4), (ok, 8, 6, 8, 0), (ok, 16000, 200, 200, 1),
                 ([(0, 40, 101, 1)], 8), ([(0, 60, 40, 1)], 8), ([(0, 50, 50, -1)], 8), (ok + [(0, 2 ** 32 - 2, 2 ** 32 - 1, -1)], 8)):
        with pytest.raises(g.GdspError):
            g.genome_regions(v, *args)
        with pytest.raises(g.GdspError):
            g.regions_rows(v, *args)
    with pytest.raises(g.GdspError):
        g.genome_regions(v, ok, 8, what=5)
    with pytest.raises(g.GdspError):
        g.regions_rows(v, ok * 70 + [(1, 40, 60, 1)], 8)                      # a vector the call does not have
    assert g.genome_regions(v, ok, 4, 2, 2, 2, what="sum").tolist() == [[38.0 + 39.0, 210.0, 235.0, 260.0, 285.0, 60.0 + 61.0]]
    assert g.genome_regions(v, [(0, 40, 60, -1)], 4, 2, 2, 2, what="sum").tolist() == [[61.0 + 60.0, 285.0, 260.0, 235.0, 210.0, 39.0 + 38.0]]
    assert g.genome_regions(v, [(0, 0, 100, 1)], 16384, what="count").sum() == 100.0


def check_regions(count, bad=None):
    a = np.tile(np.array((0, 40, 60, 1), dtype=np.int64), (count, 1))
    if bad is not None:
        a[-1] = bad
    return a


@pytest.mark.gpu
def test_the_region_check_sees_every_region():
    """the device's check of regions_rows (genome_regions refuses on the host before it): a bad last region among one
    thread's, one workgroup's, the next workgroup's, and where only the check's stride loop reaches it -- an end beyond the
    vector, an empty region, a vector the call does not have"""
    g = dev()
    v = up(g, [np.arange(cases.CHECK_N, dtype=np.float64)])
    most = cases.CHECK_COUNTS[-1]
    rows, todo = g.regions_rows(v, check_regions(most), 1, what="sum")
    assert most == 262145 and rows.shape == (most, 1) and np.all(rows == 990.0) and todo.size == 0
    for count in cases.CHECK_COUNTS:
        for bad in ((0, 40, cases.CHECK_N + 1, 1), (0, 60, 60, -1), (0, 61, 60, 1), (1, 40, 60, 1)):
            with pytest.raises(g.GdspError):
                g.regions_rows(v, check_regions(count, bad), 1, what="sum")


# --------------------------------------------------------------------------- a chromosome of 2^32 - 1 bases ----

@pytest.mark.gpu
def test_regions_across_base_2_to_the_31_and_up_to_the_last_base():
    """regions on both strands that straddle base 2^31 and end at the last base of a chromosome of 2^32 - 1 bases, with B
    not dividing L: a signed position, or a product k L kept in 32 bits (16384 columns over 300007 bases: up to 4.9e9),
    would show.  The signal is u32max_cases' synthetic depth, regenerated on the host in windows that hold each region
    and its flanks, or end where the chromosome ends"""
    import genodsp_amd as gd
    from oracle import cpu
    import u32max_cases as U32
    n, mid = U32.N, 2 ** 31
    x = gd.DeviceVector(n)
    gd.synth_coverage(U32.SEED, U32.CHROM, 0, n, 0, out=x)
    gd.sync()
    L = 300007
    windows = [(mid - 160000, 320000), (n - 310000, 310000)]                 # (first base, length)
    host = [cpu.synth_coverage(U32.SEED, U32.CHROM, first, count, 0) for first, count in windows]
    spans = [(0, mid - 150003, mid - 150003 + L), (1, n - L, n), (0, mid - 700, mid + 652), (1, n - 2001, n), (0, mid - 1, mid + 1)]
    for B, U, D, bin, which, strands in ((16384, 0, 0, 1, (0, 1), (1, -1)), (7, 300, 200, 4, (2, 3, 4), (1, -1, 1)),
                                         (1000, 512, 256, 256, (0, 1, 2, 3), (-1, 1, -1, 1))):
        whole = [(0, spans[k][1], spans[k][2], t) for k, t in zip(which, strands)]
        inside = [(spans[k][0], spans[k][1] - windows[spans[k][0]][0], spans[k][2] - windows[spans[k][0]][0], t) for k, t in zip(which, strands)]
        want = rref.figures(host, inside, B, U, D, bin)
        for name in FIGURES:
            got = gd.genome_regions([x], whole, B, U, D, bin, what=name)
            assert rref.same_bits(got, want[name]), (B, name)
            assert gd.genome_regions_last()["host cells"] == 0
        if B == 7:
            assert (want["count"][1, :U // bin] == 0).all() and (want["count"][0] > 0).all()      # upstream of a minus region that ends at the last base
