"""Group B of the 2^32 - 1 tests (test_hip_u32max_ops.py): operators whose reach is unbounded -- distance and fillgaps
without a limit, clump, segments, keepsegments, statsover -- on vectors that are one level with a handful of planted
features, so that the expected output is a formula in numpy, evaluated only where the test looks.  Every construction
takes the vector's length n and its "middle" (2^31 for the real thing) as parameters: test_planted_cases.py runs the same
constructions at n = 50 000 on the CPU and holds every formula to the operator's checker over the whole vector.

A vector is given as (level, intervals): `level` everywhere, then val added over each [start, end) (apply_intervals)."""
import numpy as np

f64 = np.float64


def build(n, level, intervals):
    """the vector as an array (short n only)"""
    v = np.full(n, level, np.float64)
    for a, z, x in intervals:
        v[a:z] += x
    return v


def window_of(n, level, intervals, a, z):
    """bases [a, z) of the vector"""
    v = np.full(z - a, level, np.float64)
    for s, e, x in intervals:
        lo, hi = max(s, a), min(e, z)
        if lo < hi:
            v[lo - a:hi - a] += x
    return v


# ------------------------------------------------------------------------------------------------ distance ----

def distance_cases(n, mid):
    """name -> (intervals of the zero vector, keyword arguments, formula(i: int64 array) -> float64 array, extra places)"""
    long_run = (mid // 2, n - 5)                                        # longer than mid: half-widths above mid / 2
    centre = (long_run[0] + long_run[1] - 1) // 2

    def both_ends(i):
        return np.minimum(i, n - 1 - i).astype(f64)

    def signed_run(i):
        a, z = long_run
        inside = -np.minimum(i - (a - 1), z - i)
        outside = np.where(i < a, a - i, i - (z - 1))
        return np.where((i >= a) & (i < z), inside, outside).astype(f64)

    return {
        "first-base-nearest": ([(0, 1, 1.0)], {}, lambda i: i.astype(f64), [n - 1]),
        "first-base-left": ([(0, 1, 1.0)], {"to": "left"}, lambda i: i.astype(f64), [n - 1]),
        "first-base-right": ([(0, 1, 1.0)], {"to": "right"}, lambda i: np.where(i == 0, 0.0, f64(n)), [n - 1]),
        "both-ends": ([(0, 1, 1.0), (n - 1, n, 1.0)], {}, both_ends, [(n - 1) // 2]),          # the tie at the midpoint
        "signed-long-run": ([long_run + (1.0,)], {"signed": True}, signed_run, [centre, long_run[0], long_run[1]]),
    }


# ------------------------------------------------------------------------------------------------ fillgaps ----

FILL_A, FILL_B = 0.1, 7.3                        # the values of the two known bases


def fill_l(n):
    """the lower known base, 2 or 3: r - l even with r = n - 1, so that one base ties between them"""
    return 2 + (n - 1) % 2


def fill_intervals(n):
    return [(fill_l(n), fill_l(n) + 1, FILL_A), (n - 1, n, FILL_B)]


def fill_cases(n):
    """name -> (keyword arguments, formula(i) -> float64 array); the vector is fill_intervals(n) on zeros, T = 0"""
    l, r, a, b = fill_l(n), n - 1, f64(FILL_A), f64(FILL_B)

    def linear(i):
        k = (i - l).astype(f64)
        d = f64(r - l)
        x = a + ((b - a) * k) / d                                       # four operations, each rounded once
        x = np.where(x < a, a, np.where(x > b, b, x))
        return np.where(i < l, a, x)                                    # (ends extend: in front of l only l exists)

    def nearest(i):
        return np.where(i < l, a, np.where(i - l <= r - i, a, b))       # the lower coordinate wins the tie

    return {
        "linear": ({"how": "linear"}, linear),
        "nearest": ({"how": "nearest"}, nearest),
        "left-extend": ({"how": "left", "ends": "extend"}, lambda i: np.where(i == r, b, a)),
        "left-keep": ({"how": "left", "ends": "keep"}, lambda i: np.where(i == r, b, np.where(i < l, 0.0, a))),
        "right-extend": ({"how": "right", "ends": "extend"}, lambda i: np.where(i <= l, a, b)),
        "right-keep": ({"how": "right", "ends": "keep"}, lambda i: np.where(i <= l, a, b)),
    }


# --------------------------------------------------------------------------------------------------- clump ----
# The running excess P[i] = sum of (v[k] - average) over k <= i.  On the level between two bumps every term is -1/2
# (clump: level 0, average 1/2; anticlump: level 1 with dips to 0, average 1/2, the sign turned), so P only falls there:
# a stretch with a non-negative sum that reaches into the level has to hold a bump, and it can hold at most 2 E bases of
# level for a bump whose own excess is E.  With the bumps further apart than that, what is marked around a bump depends on
# nothing but the bump and 2 E bases of level on either side: the result is local to a bump, and a window that starts and
# ends in the level at least CLUMP_MARGIN from it sees what the whole vector sees.

CLUMP_AVERAGE, CLUMP_MIN_LENGTH = 0.5, 40
CLUMP_MARGIN = 2000                              # above 2 E + min_length for the largest bump (E = 300 x 2.5 = 750)


def clump_bumps(n, mid):
    """(start, end, height) of the bumps: near base 0, across mid, in the last tile, up to the very last base, and one too
    short to count"""
    return [(30, 130, 3.0), (mid - 150, mid + 150, 3.0), (mid + 5000, mid + 5010, 1.0), (n - 3500, n - 3400, 2.0), (n - 60, n, 4.0)]


def clump_vector(n, mid, above):
    """(level, intervals): bumps on zeros for clump, dips of a level of ones for anticlump"""
    if above:
        return 0.0, clump_bumps(n, mid)
    return 1.0, [(a, z, -1.0) for a, z, _ in clump_bumps(n, mid)]


def clump_windows(n, mid):
    """[a, z) around every bump, starting and ending in the level (or at an end of the vector)"""
    return [(max(0, a - CLUMP_MARGIN), min(n, z + CLUMP_MARGIN)) for a, z, _ in clump_bumps(n, mid)]


# ------------------------------------------------------------------- segments, keepsegments, statsover ----

def region_intervals(n, mid):
    """planted regions of a zero vector: near base 0 with a summit, two either side of mid 10 bases apart (the second across
    mid, with a summit past it), one in the last tile, and the very last base"""
    return [(5, 9, 2.0), (7, 8, 1.0),
            (mid - 100, mid - 20, 1.5), (mid - 10, mid + 10, 3.0), (mid + 3, mid + 4, 0.5),
            (n - 3000, n - 2000, 4.0), (n - 2500, n - 2499, 0.25),
            (n - 1, n, 8.0)]


def region_rows(n, mid, merge_gap=0):
    """the segments of region_intervals above T = 0: (start, end, count, sum, mean, min, max, maxpos), written out by hand"""
    rows = [(5, 9, 4, 9.0, 2.25, 2.0, 3.0, 7)]
    left = (mid - 100, mid - 20, 80, 120.0, 1.5, 1.5, 1.5, mid - 100)
    right = (mid - 10, mid + 10, 20, 60.5, 3.025, 3.0, 3.5, mid + 3)
    if merge_gap >= 10:
        rows.append((mid - 100, mid + 10, 100, 180.5, 1.805, 1.5, 3.5, mid + 3))
    else:
        rows += [left, right]
    rows.append((n - 3000, n - 2000, 1000, 4000.25, 4.00025, 4.0, 4.25, n - 2500))
    rows.append((n - 1, n, 1, 8.0, 8.0, 8.0, 8.0, n - 1))
    return rows


def long_run(n, mid):
    """one run of ones longer than mid, and its row"""
    a, z = mid // 2, n - 5
    return [(a, z, 1.0)], (a, z, z - a, float(z - a), 1.0, 1.0, 1.0, a)


def interval_queries(n, mid):
    """[start, end) to ask statsover for: everything, across mid, up to the end, inside the level"""
    return [(0, n), (mid - 50, mid + 7), (n - 2600, n), (100, 200)]


# ---------------------------------------------------------------------------- profileover, matrixover ----

FLANK = 300


def anchor_groups(n, mid):
    """[(first base of a window, its length, [(position, strand), ...])]: anchors on both strands near base 0, either side
    of mid, and within FLANK of the last base (their windows are cut at both ends of the vector).  Every window holds its
    anchors' whole reach, or ends where the vector ends: the checkers, fed one window per group with the anchors moved
    into it, cut exactly where the vector does"""
    return [(0, 1000, [(100, 1), (50, -1), (0, 1), (299, -1), (0, -1)]),
            (mid - 1000, 2000, [(mid - 1, 1), (mid - 1, -1), (mid, 1), (mid, -1), (mid - 150, 1), (mid + 150, -1)]),
            (n - 1000, 1000, [(n - 1, 1), (n - 1, -1), (n - 100, 1), (n - 200, -1), (n - FLANK, 1)])]


def anchors_whole(n, mid):
    """rows (vector 0, position, strand) for the library"""
    return [(0, p, s) for _, _, group in anchor_groups(n, mid) for p, s in group]


def anchors_windowed(n, mid):
    """rows (window index, position inside the window, strand) for a checker fed the windows as vectors"""
    return [(k, p - first, s) for k, (first, _, group) in enumerate(anchor_groups(n, mid)) for p, s in group]
