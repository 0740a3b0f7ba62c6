"""GPU: the operators test_hip_u32max.py does not reach, on one chromosome of 2^32 - 1 bases: base indices at and above
2^31, tiles whose end lies within a window of 2^32, counters and lengths above 2^31.  The method, the places and the
cases are u32max_cases.py's; test_u32max_locality.py proves on the CPU that a window plus its halo is all a checker needs.

Group A, the operators of bounded reach: the device's result at every place against the operator's own CPU checker run
on the regenerated signal, bit for bit (integer depth wherever sums are involved: no sum can round).  At most three
34.4 GB vectors are alive at any moment: the two signals and one result, copy or second track."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, bits_equal
from oracle import cpu
import correlate_ref
import distance_ref
import histogram_ref
import keepsegments_ref
import localstats_ref
import matrixover_ref
import planted_cases as P
import profileover_ref
import segments_ref
import stepsignal_ref as S
import u32max_cases as U
from u32max_cases import CHROM, M, N, SEED, TRACK_CHROM, fetch, places
from xsum_ref import same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gd():
    import genodsp_amd
    return genodsp_amd


class Pool:
    """The three 34.4 GB vectors every test here works in, allocated once and handed round: giving one back and
    allocating the next costs one to six seconds at this size (profiles/u32max_ops.txt), more than any operator, so a
    test that allocated its own would mostly be waiting.  Two hold what tests share, by name (the signals, the planted
    vectors): get() fills one when it is first asked for, over a name outside `keep`.  The third is anybody's to
    overwrite: scratch() -- a result, a copy to work in place on, a second track."""

    def __init__(self, gd):
        self.gd, self.named, self.idle, self.spare = gd, {}, [], None

    def get(self, name, fill, keep):
        if name not in self.named:
            for other in [k for k in self.named if k not in keep]:
                self.idle.append(self.named.pop(other))
            assert len(self.named) < 2
            v = self.idle.pop() if self.idle else self.gd.DeviceVector(N)
            fill(v)
            self.gd.sync()
            self.named[name] = v
        return self.named[name]

    def scratch(self):
        if self.spare is None:
            self.spare = self.gd.DeviceVector(N)
        return self.spare


@pytest.fixture(scope="module")
def pool(gd):
    p = Pool(gd)
    yield p
    p.named.clear()
    p.idle.clear()
    p.spare = None


@pytest.fixture(scope="module")
def signal(gd, pool):
    """signal(mode) -> the chromosome's synthetic signal on the device (0: integer depth, 1: real-valued), never written"""
    names = {0: "depth", 1: "real"}
    return lambda mode: pool.get(names[mode], lambda v: gd.synth_coverage(SEED, CHROM, 0, N, mode, out=v), keep=names.values())


def copy_into(gd, out, v):
    gd.sync()
    gd.call("gdsp_memcpy_d2d", out.ptr, v.ptr, v.n * 8, None)
    return out


# ------------------------------------------------------------------------------------------------ group A ----

@pytest.fixture(scope="module")
def device_windows(gd, pool, signal):
    """device_windows(name) -> {place: (start, the device's values there)} of case `name`: one run of the operator, its
    windows kept on the host.  Only the case asked for last is held, so the parts of a case share one run in whatever
    order or selection the tests come."""
    held = {}

    def windows(name):
        if name not in held:
            held.clear()
            case = U.CASES[name]
            x, spare = signal(case.mode), pool.scratch()
            if case.tracks == 2:
                tracks = [x, gd.synth_coverage(SEED, TRACK_CHROM, 0, N, case.mode, out=spare)]
            else:
                tracks = [copy_into(gd, spare, x) if case.in_place else x]
            if not case.in_place:
                gd.fill(spare, float("nan"))                               # (whatever the last user left there)
            out = case.run(gd, tracks, spare)
            assert out is spare
            gd.sync()
            held[name] = {}
            for p in places():
                s, count = case.window(p)
                held[name][p] = (s, fetch(out, s, count))
        return held[name]

    return windows


PARTS = [(name, part) for name in sorted(U.CASES) for part in range(U.CASES[name].parts)]


@pytest.mark.parametrize("name,part", PARTS,
                         ids=["%s-part%d" % (n, k) if U.CASES[n].parts > 1 else n for n, k in PARTS])
def test_window_local_operator(device_windows, name, part):
    case = U.CASES[name]
    got = device_windows(name)
    if part == 0:
        assert 2 ** 31 in got and N - M in got and 0 in got and any(p >= 2 ** 32 - (1 << 19) for p in got)
    for p in places()[part::case.parts]:
        s, have = got[p]
        want = case.expected(s, have.size)
        assert have.size >= M and s + have.size <= N
        assert bits_equal(have, want), (name, p, s + int(np.flatnonzero(have.view(np.int64) != want.view(np.int64))[0]))


# ------------------------------------------------------------------------------------------------ group C ----
# Genome-wide reductions on a step signal: four levels with steps at 2^30, 2^31 and 3 2^30, single bases planted on top
# (one past 2^31, one at the last base), and a second track of two halves.  Every level's count is known, so the
# expected figures are stepsignal_ref's run-length arithmetic -- ranks, bin counts and run lengths above 2^30 and 2^31 --
# held to the array checkers on the CPU by test_stepsignal_ref.py.

STEPS = S.step_intervals(N, 2 ** 30, 2 ** 31, 3 * 2 ** 30, [(2 ** 31 + 12345, 1000.0), (N - 1, -500.0), (17, 0.375)])
HALVES = S.halves_intervals(N, 2 ** 31, [(2 ** 31 - 1, 64.0), (N - 2, -8.5)])
PERCENTILES = (0, 25000, 50000, 74999, 75000, 75001, 99999, 100000)


def plant(gd, v, intervals, level=0.0):
    """v becomes `level` with the intervals' values added (interval ingest at the top of the range: test_hip_u32max.py)"""
    gd.fill(v, level)
    gd.apply_intervals(v, np.array([a for a, _, _ in intervals], np.uint32), np.array([z for _, z, _ in intervals], np.uint32),
                       np.array([x for _, _, x in intervals], np.float64))
    return v


@pytest.fixture(scope="module")
def steps(gd, pool):
    return lambda: pool.get("steps", lambda v: plant(gd, v, STEPS), keep=("steps", "halves"))


@pytest.fixture(scope="module")
def halves(gd, pool):
    return lambda: pool.get("halves", lambda v: plant(gd, v, HALVES), keep=("steps", "halves"))


def same_all(got, want):
    return len(got) == len(want) and all(same(a, b) for a, b in zip(got, want))


def test_step_signals_are_what_was_planted(gd, steps, halves):
    for vec, intervals in ((steps(), STEPS), (halves(), HALVES)):
        runs, at = S.from_intervals(N, intervals), 0
        for length, value in runs:                                      # both edges of every run
            for p in sorted({at, at + length - 1}):
                assert fetch(vec, p, 1)[0] == value, (p, value)
            at += length
        assert at == N


@pytest.mark.parametrize("strategy", ["SELECT_AUTO", "SELECT_RADIX", "SELECT_BRACKET"])
def test_percentiles_of_a_step_signal(gd, steps, strategy):
    """ranks above 2^31 (75 % of 2^32 - 1 values and beyond), buckets that hold 2^30 equal values"""
    runs = S.from_intervals(N, STEPS)
    want = [S.percentile(runs, p) for p in PERCENTILES]
    assert want[0] == -499.5 and want[-1] == 1007.0 and len(set(want)) >= 5      # (both planted extremes, every level)
    assert gd.lib().gdsp_percentile_rank(N, 75001) > 2 ** 31
    count, got = gd.percentile([steps()], PERCENTILES, strategy=getattr(gd, strategy))
    assert count == N
    assert same_all(got, want), (got, want)


def test_minmax_of_a_step_signal(gd, steps):
    lo, hi, count = gd.genome_minmax([steps()])
    assert (lo, hi, count) == S.minmax(S.from_intervals(N, STEPS)) + (N,)


def test_stats_of_a_step_signal(gd, steps):
    want = S.stats(S.from_intervals(N, STEPS))
    got = gd.genome_stats([steps()])
    assert got["count"] == float(N)
    assert same_all([got[k] for k in ("count", "sum", "mean", "variance", "stddev")], want), (got, want)


@pytest.mark.parametrize("uniform", [True, False])
def test_histogram_of_a_step_signal(gd, steps, uniform):
    """bin counts above 2^30 with the uniform hint on and off (the table the driver makes of such counts, its atleast
    column and the mode: test_driver_reports_figures_above_2_31)"""
    edges = gd.histogram_uniform_edges(-4.0, 1.0, 12)
    assert edges.tobytes() == histogram_ref.uniform_edges(-4.0, 1.0, 12).tobytes()
    want = S.histogram_words(S.from_intervals(N, STEPS), edges)
    assert sum(1 for c in want[:12] if c >= 2 ** 30 - 2) == 4 and want[12] == 1 and want[13] == 1 and want[14] == N
    counts, below, above, n = gd.genome_histogram([steps()], lo=-4.0, width=1.0, bins=12, uniform=uniform)
    got = [int(c) for c in counts] + [below, above, n]
    assert got == want


def test_correlation_of_two_step_signals(gd, steps, halves):
    want = S.correlation(S.from_intervals(N, STEPS), S.from_intervals(N, HALVES))
    got = gd.genome_correlation([(steps(), halves())])
    assert same_all([got[k] for k in correlate_ref.FIGURES], want), (got, want)


def test_lag_correlation_of_two_step_signals(gd, steps, halves):
    """lags -2 .. 2: each lag's sum is overlap length times product, exactly; the pairs per lag are N - |lag|"""
    fig, counts, cov, corr = S.lag_curve(S.from_intervals(N, STEPS), S.from_intervals(N, HALVES), -2, 5)
    got = gd.genome_lag_correlation([(steps(), halves())], -2, 5)
    assert same_all([got[k] for k in correlate_ref.FIGURES], fig)
    assert [int(c) for c in got["pairs"]] == counts == [N - 2, N - 1, N, N - 1, N - 2]
    assert same_all(got["covariances"], cov) and same_all(got["correlations"], corr), (got, cov, corr)
    assert len(set(cov)) == 5


# ------------------------------------------------------------------------------------------------ group B ----
# Unbounded reach: distances, gap lengths, run lengths and segment statistics above 2^31, on vectors that are one level
# with a handful of planted features (planted_cases.py).  The expected output is a formula, held to the operator's
# checker over a whole short vector by test_planted_cases.py, and evaluated here at the usual places and at the places
# each case adds (the far end, the midpoint's tie, the run's centre and edges).

MID = 2 ** 31


def spots(extra=()):
    """window starts: places(), and a window around each extra base"""
    return list(dict.fromkeys(places() + [max(0, min(N - M, int(e) - M // 2)) for e in extra]))


def check_formula(vec, formula, extra=()):
    for p in spots(extra):
        want = np.ascontiguousarray(formula(np.arange(p, p + M, dtype=np.int64)), np.float64)
        got = fetch(vec, p, M)
        assert bits_equal(got, want), (p, p + int(np.flatnonzero(got.view(np.int64) != want.view(np.int64))[0]))


@pytest.mark.parametrize("name", sorted(P.distance_cases(N, MID)))
def test_distance_without_a_cap(gd, pool, name):
    """distances up to 2^32 - 2 (and n = 2^32 - 1 where there is no member), the tie at the midpoint, and minus the
    half-width of a member run longer than 2^31"""
    intervals, kw, formula, extra = P.distance_cases(N, MID)[name]
    v = gd.distance(plant(gd, pool.scratch(), intervals), **kw)
    check_formula(v, formula, extra)
    if name == "first-base-nearest":
        assert fetch(v, N - 1, 1)[0] == 4294967294.0
    if name == "first-base-right":
        assert fetch(v, N - 1, 1)[0] == 4294967295.0 and fetch(v, 0, 2).tolist() == [0.0, 4294967295.0]
    if name == "both-ends":
        assert fetch(v, MID - 2, 3).tolist() == [2147483646.0, 2147483647.0, 2147483646.0]


@pytest.mark.parametrize("name", sorted(P.fill_cases(N)))
def test_fill_gaps_without_a_limit(gd, pool, name):
    """one gap of 2^32 - 4 bases between two known values: i - l and r - l beyond 2^31 in the line's arithmetic, the
    nearest side flipping behind base 2^31 (the tie goes to the lower coordinate), and the ends"""
    kw, formula = P.fill_cases(N)[name]
    v = gd.fill_gaps(plant(gd, pool.scratch(), P.fill_intervals(N)), **kw)
    check_formula(v, formula)
    if name == "nearest":
        assert fetch(v, MID - 1, 3).tolist() == [P.FILL_A, P.FILL_A, P.FILL_B]


@pytest.mark.parametrize("above", [True, False], ids=["clump", "anticlump"])
def test_clump_around_planted_bumps(gd, pool, above):
    """(why a window around a bump is all the checker needs: the head of planted_cases' clump section)"""
    level, intervals = P.clump_vector(N, MID, above)
    v = gd.clump(plant(gd, pool.scratch(), intervals, level), P.CLUMP_AVERAGE, P.CLUMP_MIN_LENGTH, above=above)
    for a, z in P.clump_windows(N, MID):
        want = cpu.clump(P.window_of(N, level, intervals, a, z), P.CLUMP_AVERAGE, P.CLUMP_MIN_LENGTH, above=above)
        assert bits_equal(fetch(v, a, z - a), want), (a, z)
    inside = lambda p: any(a < p + M and p < z for a, z in P.clump_windows(N, MID))
    quiet = [p for p in places() if not inside(p)]
    assert len(quiet) >= 6
    for p in quiet:                                                     # in the level, away from every bump: nothing is marked
        assert not fetch(v, p, M).any(), p
    assert fetch(v, N - 1, 1)[0] == 1.0 and fetch(v, MID, 1)[0] == 1.0


@pytest.fixture(scope="module")
def regions(gd, pool):
    return lambda: pool.get("regions", lambda v: plant(gd, v, P.region_intervals(N, MID)), keep=("regions", "run"))


@pytest.fixture(scope="module")
def run(gd, pool):
    return lambda: pool.get("run", lambda v: plant(gd, v, P.long_run(N, MID)[0]), keep=("regions", "run"))


def rows_as_genome(rows):
    return [(0,) + r for r in rows]


@pytest.mark.parametrize("merge_gap", [0, 10])
def test_segments_of_planted_regions(gd, regions, merge_gap):
    """start, end, count, sum, mean, min, max and maxpos of every region, coordinates above 2^31 included; merge_gap joins
    the two regions either side of 2^31"""
    got = gd.segments(regions(), 0.0, merge_gap=merge_gap)
    segments_ref.same_table(got, rows_as_genome(P.region_rows(N, MID, merge_gap)))
    assert int(got["end"][-1]) == N and int(got["maxpos"][-1]) == N - 1 and int(got["maxpos"][1 if merge_gap else 2]) == MID + 3


def test_segments_longer_than_2_31(gd, pool, run):
    """one run longer than 2^31, and a vector of ones: one segment [0, N) with count = sum = N"""
    got = gd.segments(run(), 0.0)
    row = P.long_run(N, MID)[1]
    segments_ref.same_table(got, rows_as_genome([row]))
    assert int(got["end"][0]) - int(got["start"][0]) == int(got["count"][0]) > 2 ** 31
    ones = gd.fill(pool.scratch(), 1.0)
    got = gd.segments(ones, 0.0)
    segments_ref.same_table(got, [(0, 0, N, N, float(N), 1.0, 1.0, 1.0, 0)])


@pytest.mark.parametrize("as_", ["length", "sum"])
def test_keep_segments_paints_figures_above_2_31(gd, pool, run, regions, as_):
    """the run's length and sum as doubles above 2^31 over exactly its bases, `zero` elsewhere: at the places and at the
    run's two edges; then the planted regions' figures at every region's two edges"""
    (a, z, _), row = P.long_run(N, MID)[0][0], P.long_run(N, MID)[1]
    out = pool.scratch()
    got = gd.keep_segments(run(), out, 0.0, as_=as_, zero=-1.0)
    segments_ref.same_table(got, rows_as_genome([row]))
    figure = float(z - a)
    assert figure > 2.0 ** 31
    check_formula(out, lambda i: np.where((i >= a) & (i < z), figure, -1.0), extra=[a, z])
    assert fetch(out, a - 1, 2).tolist() == [-1.0, figure] and fetch(out, z - 1, 2).tolist() == [figure, -1.0]
    rows = P.region_rows(N, MID, 10)
    got = gd.keep_segments(regions(), out, 0.0, merge_gap=10, as_=as_, zero=-1.0)
    segments_ref.same_table(got, rows_as_genome(rows))

    def painted(i):
        want = np.full(i.size, -1.0)
        for r in rows:
            want[(i >= r[0]) & (i < r[1])] = keepsegments_ref.figure(r, as_)
        return want

    check_formula(out, painted, extra=[e for r in rows for e in (r[0], r[1] - 1)])


def test_interval_stats_up_to_the_last_base(gd, regions):
    """statsover over [0, N), over an interval that straddles 2^31 and over one that ends at N"""
    queries = P.interval_queries(N, MID)
    got = gd.interval_stats(regions(), [a for a, _ in queries], [z for _, z in queries])
    runs = S.from_intervals(N, P.region_intervals(N, MID))
    for k, (a, z) in enumerate(queries):
        want = S.interval_figures(runs, a, z)
        have = (int(got["count"][k]), got["sum"][k], got["mean"][k], got["min"][k], got["max"][k], int(got["maxpos"][k]))
        assert have[0] == want[0] == z - a and have[5] == want[5], (a, z, have, want)
        assert same_all(have[1:5], want[1:5]), (a, z, have, want)
    assert int(got["count"][0]) == N and int(got["maxpos"][0]) == N - 1 and int(got["maxpos"][1]) == MID + 3


def anchor_windows(mode=0):
    return [cpu.synth_coverage(SEED, CHROM, first, count, mode) for first, count, _ in P.anchor_groups(N, MID)]


def test_profile_around_anchors_up_to_the_last_base(gd, signal):
    """anchors on both strands near base 0, either side of 2^31 and within the flank of the last base, over the depth
    signal: every column's count, sum, mean, variance, stddev against profileover_ref fed the regenerated windows"""
    want = profileover_ref.profile(anchor_windows(), P.anchors_windowed(N, MID), -P.FLANK, 2 * P.FLANK + 1)
    got = gd.genome_profile([signal(0)], P.anchors_whole(N, MID), -P.FLANK, 2 * P.FLANK + 1)
    assert [int(c) for c in got["count"]] == [int(w[0]) for w in want]
    assert min(int(c) for c in got["count"]) < len(P.anchors_whole(N, MID))      # windows are cut at both ends
    for k, name in ((1, "sum"), (2, "mean"), (3, "variance"), (4, "stddev")):
        assert same_all(got[name], [w[k] for w in want]), name


@pytest.mark.parametrize("what", ["mean", "sum", "count", "min", "max"])
def test_matrix_around_anchors_up_to_the_last_base(gd, signal, what):
    want = matrixover_ref.matrix(anchor_windows(), P.anchors_windowed(N, MID), -P.FLANK, 2 * P.FLANK, 4, what)
    got = gd.genome_matrix([signal(0)], P.anchors_whole(N, MID), -P.FLANK, 2 * P.FLANK, 4, what)
    assert matrixover_ref.same_bits(got, want)
    assert np.isnan(want).any() or what in ("sum", "count")             # cells beyond the ends have nothing to look at


# ------------------------------------------------------------------------------------------------ group D ----

BIN = os.path.join(ROOT, "genodsp_amd", "genodsp_hip")


def test_driver_runs_four_more_operators_on_u32max_bases(tmp_path):
    """genodsp_hip chrU:4294967295 with reads near both ends and across 2^31, as test_hip_u32max.py's driver test, through
    segments and statsover (their tables print coordinates as unsigned decimals: none may come out negative), then
    distance --max=1000 and localstats W=101 --as=mean.  Far from every read the distance is the cap and so is its local
    mean, exactly: the final report is the three windows' runs joined by runs of 1000 that span up to 2^31 bases (its
    positions go through %d like the reference's, so those beyond 2^31 come out negative there).  Expected text from
    checker windows."""
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "genodsp_amd", "host")])
    rng = np.random.default_rng(12)
    spots = [(0, 3000), (2 ** 31 - 1500, 2 ** 31 + 1500), (N - 3000, N)]
    reads = []
    for lo, hi in spots:
        for _ in range(400):
            a = int(rng.integers(lo, hi - 1))
            z = min(hi, a + int(rng.integers(1, 200)))
            reads.append((a, z, int(rng.integers(1, 9))))
    reads.append((N - 1, N, 7))
    text = "".join("chrU\t%d\t%d\t%d\n" % r for r in reads)
    regions = [(0, N), (2 ** 31 - 500, 2 ** 31 + 700), (N - 2000, N), (5000, 6000), (2 ** 31 + 100, 2 ** 31 + 101)]
    with open(os.path.join(str(tmp_path), "regions.bed"), "w") as f:
        f.write("".join("chrU\t%d\t%d\n" % r for r in regions))
    p = subprocess.run([BIN, "chrU:%d" % N, "--precision=6",
                        "=", "segments", "60", "--mergegap=3", "--precision=6", "--output=segments.tsv",
                        "=", "statsover", "regions.bed", "--precision=6", "--output=stats.tsv",
                        "=", "distance", "--max=1000", "=", "localstats", "W=101", "--as=mean"],
                       input=text, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]

    margin = 1300                                                       # beyond the cap and the window's reach: level zero, distance 1000
    windows = []                                                        # (first base, the ingested depth there)
    for lo, hi in spots:
        a, z = max(0, lo - margin), min(N, hi + margin)
        x = np.zeros(z - a)
        for s, e, v in reads:
            if s >= a and e <= z:
                x[s - a:e - a] += v
        windows.append((a, x))

    # segments: every region lies inside a window
    number = lambda v: "%.6f" % v
    want = []
    for a, x in windows:
        for s, e, n, total, mean, mn, mx, pos in segments_ref.segments(x, 60.0, merge_gap=3):
            want.append("\t".join(["chrU", str(a + s), str(a + e), str(n), number(total), number(mean), number(mn), number(mx),
                                   str(a + pos)]))
    with open(os.path.join(str(tmp_path), "segments.tsv")) as f:
        got = f.read().splitlines()
    assert got == want and len(got) > 20
    assert "-" not in "".join(got) and int(got[-1].split("\t")[1]) > 2 ** 31 and int(got[-1].split("\t")[8]) > 2 ** 31

    # statsover: the windows' bases and zeros everywhere else (integer depth: the sum is exact in a double)
    want = []
    for s, e in regions:
        total, best, where, low = 0, 0.0, s, None
        covered = 0
        for a, x in windows:
            lo_, hi_ = max(s, a), min(e, a + x.size)
            if lo_ < hi_:
                part = x[lo_ - a:hi_ - a]
                total += int(part.sum())
                covered += part.size
                low = float(part.min()) if low is None else min(low, float(part.min()))
                if part.max() > best:
                    best, where = float(part.max()), lo_ + int(np.argmax(part))
        if covered < e - s:
            low = 0.0 if low is None else min(low, 0.0)
        want.append("\t".join(["chrU", str(s), str(e), str(e - s), number(float(total)), number(total / (e - s)), number(low),
                               number(best), str(where)]))
    with open(os.path.join(str(tmp_path), "stats.tsv")) as f:
        got = f.read().splitlines()
    assert got == want
    assert "-" not in "".join(got) and got[0].split("\t")[3] == str(N) and int(got[2].split("\t")[8]) > 2 ** 31

    # the final report: distance, then its local mean, window by window; between the windows everything is 1000
    runs = []
    for a, x in windows:
        d = distance_ref.distance(x, cap=1000)
        y, low, high = localstats_ref.local_stats(d, 101, "mean", tile=0)
        assert localstats_ref.same_bits(low, high).all()
        rs, re_, rv = cpu.report_runs(y)
        mine = [(a + s, a + e, v) for s, e, v in zip(rs.tolist(), re_.tolist(), rv.tolist())]
        if a > 0:
            assert mine[0][0] == a and mine[0][2] == 1000.0 and runs[-1][2] == 1000.0
            mine[0] = (runs.pop()[0], mine[0][1], 1000.0)               # the run of 1000 that began in the window before
        runs += mine
    want = ["chrU\t%d\t%d\t%.6f" % (ctypes.c_int32(s).value, ctypes.c_int32(e).value, v) for s, e, v in runs]
    got = p.stdout.splitlines()
    assert len(got) == len(want) and len(got) > 1000
    assert got == want
    assert max(e - s for s, e, _ in runs) > 2 ** 31 - 10000


def test_driver_reports_figures_above_2_31(tmp_path):
    """genodsp_hip chrU:4294967295 on a signal of three levels -- 0 below 2^30, 1 up to 3 2^29, 2 up to five bases before
    the end -- and a 7 on the last base.  `segments 0` finds one segment of 3 221 225 466 bases and one of a single base:
    its table, and the variables segments, covered and longest as `variables` shows them.  `histogram` counts 2 684 354 554
    bases in one bin: its table (counts, fractions, the atleast column), count and mode against histogram_ref's text of the
    run-length counts."""
    if not os.path.exists(BIN):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "genodsp_amd", "host")])
    a, b, z = 2 ** 30, 3 * 2 ** 29, N - 5
    reads = [(a, z, 1), (b, z, 1), (N - 1, N, 7)]
    text = "".join("chrU\t%d\t%d\t%d\n" % r for r in reads)
    p = subprocess.run([BIN, "chrU:%d" % N, "--nooutput",
                        "=", "segments", "0", "--precision=6", "--output=segments.tsv",
                        "=", "histogram", "--lo=0", "--width=1", "--bins=8", "--output=histogram.tsv",
                        "=", "variables"],
                       input=text, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode == 0 and p.stdout == "", p.stderr[-2000:]
    shown = {k: float(v) for k, v in re.findall(r"^\s*(\w+) = (\S+)$", p.stderr, flags=re.M)}

    longest = z - a
    assert longest == 3221225466 > 2 ** 31
    assert (shown["segments"], shown["covered"], shown["longest"]) == (2.0, float(longest + 1), float(longest))
    number = lambda v: "%.6f" % v
    total = (b - a) + 2 * (z - b)
    want = ["\t".join(["chrU", str(a), str(z), str(longest), number(float(total)), number(total / longest), number(1.0), number(2.0), str(b)]),
            "\t".join(["chrU", str(N - 1), str(N), "1", number(7.0), number(7.0), number(7.0), number(7.0), str(N - 1)])]
    with open(os.path.join(str(tmp_path), "segments.tsv")) as f:
        assert f.read().splitlines() == want

    runs = [(a, 0.0), (b - a, 1.0), (z - b, 2.0), (4, 0.0), (1, 7.0)]
    assert sum(n for n, _ in runs) == N
    edges = histogram_ref.uniform_edges(0.0, 1.0, 8)
    words = S.histogram_words(runs, edges)
    assert words[:8] == [a + 4, b - a, z - b, 0, 0, 0, 0, 1] and words[2] == 2684354554 > 2 ** 31 and words[8:] == [0, 0, N]
    with open(os.path.join(str(tmp_path), "histogram.tsv")) as f:
        got = f.read()
    assert got == histogram_ref.table_text(np.array(words, np.uint64), edges)
    assert got.splitlines()[5].split("\t")[4] == "%.17g" % ((N - a - 4) / N)                  # (atleast of the bin from 1 on)
    assert (shown["count"], shown["mode"]) == (float(N), 2.0) == (float(N), histogram_ref.mode_of(words, edges))
    assert "count is 4294967295\n" in p.stderr and "mode is 2\n" in p.stderr
