"""CPU: every construction of planted_cases.py at n = 50 000 (its middle standing for base 2^31), each formula held to the
operator's checker run over the whole vector -- so that on the device, at 2^32 - 1 bases, the formulas can stand in for
checkers that could never run there."""
import numpy as np
import pytest

from conftest import bits_equal
from oracle import cpu

import distance_ref
import fillgaps_ref
import keepsegments_ref
import planted_cases as P
import segments_ref
import stepsignal_ref as S
from xsum_ref import same

N, MID = 50000, 25000
EVERY = np.arange(N, dtype=np.int64)


@pytest.mark.parametrize("name", sorted(P.distance_cases(N, MID)))
def test_distance_formulas(name):
    intervals, kw, formula, extra = P.distance_cases(N, MID)[name]
    want = distance_ref.distance(P.build(N, 0.0, intervals), **kw)
    assert bits_equal(formula(EVERY), want)
    assert all(0 <= p < N for p in extra)
    if name == "both-ends":
        assert int(np.argmax(want)) in extra
    if name == "signed-long-run":
        assert int(np.argmin(want)) in extra and -want.min() > MID / 2


@pytest.mark.parametrize("name", sorted(P.fill_cases(N)))
def test_fillgaps_formulas(name):
    kw, formula = P.fill_cases(N)[name]
    v = P.build(N, 0.0, P.fill_intervals(N))
    want = fillgaps_ref.fill_gaps(v, **kw)
    assert bits_equal(formula(EVERY), want)
    if name == "nearest":
        tie = (P.fill_l(N) + N - 1) // 2
        assert (P.fill_l(N) + N - 1) % 2 == 0 and want[tie] == P.FILL_A and want[tie + 1] == P.FILL_B
        assert P.fill_l(2 ** 32 - 1) == 2 and (2 + 2 ** 32 - 2) // 2 == 2 ** 31      # the real thing ties at base 2^31


@pytest.mark.parametrize("above", [True, False])
def test_clump_is_local_to_a_bump(above):
    """the argument at the head of planted_cases' clump section, checked: every window gives what the whole vector gives,
    and outside the windows nothing is marked"""
    level, intervals = P.clump_vector(N, MID, above)
    whole = cpu.clump(P.build(N, level, intervals), P.CLUMP_AVERAGE, P.CLUMP_MIN_LENGTH, above=above)
    covered = np.zeros(N, bool)
    marked = 0
    for a, z in P.clump_windows(N, MID):
        got = cpu.clump(P.window_of(N, level, intervals, a, z), P.CLUMP_AVERAGE, P.CLUMP_MIN_LENGTH, above=above)
        assert bits_equal(got, whole[a:z]), (a, z)
        covered[a:z] = True
        marked += int(got.sum() > 0)
    assert not whole[~covered].any()
    assert marked == len(P.clump_bumps(N, MID)) - 1                       # every bump but the one that is too short
    assert whole[N - 1] == 1.0 and whole[MID] == 1.0                      # (marked up to the very last base, and across the middle)
    E = max((z - a) * (h - P.CLUMP_AVERAGE) for a, z, h in P.clump_bumps(N, MID))
    assert 2 * E + P.CLUMP_MIN_LENGTH < P.CLUMP_MARGIN


@pytest.mark.parametrize("merge_gap", [0, 10])
def test_region_rows(merge_gap):
    v = P.build(N, 0.0, P.region_intervals(N, MID))
    want = segments_ref.segments(v, 0.0, merge_gap=merge_gap)
    rows = P.region_rows(N, MID, merge_gap)
    assert len(rows) == len(want)
    for r, w in zip(rows, want):
        assert r[:3] == w[:3] and r[7] == w[7] and all(same(a, b) for a, b in zip(r[3:7], w[3:7])), (r, w)


def test_long_run_row_and_what_keepsegments_paints():
    intervals, row = P.long_run(N, MID)
    v = P.build(N, 0.0, intervals)
    assert [row] == segments_ref.segments(v, 0.0) and row[1] - row[0] > MID
    for mode in ("length", "sum"):
        want = keepsegments_ref.keep(v, 0.0, mode, zero=-1.0)
        assert set(np.unique(want).tolist()) == {-1.0, float(row[1] - row[0])}
        assert want[row[0]] == want[row[1] - 1] == float(row[1] - row[0]) and want[row[0] - 1] == want[row[1]] == -1.0


def test_interval_figures():
    intervals = P.region_intervals(N, MID)
    v = P.build(N, 0.0, intervals)
    runs = S.from_intervals(N, intervals)
    assert S.to_array(runs).tobytes() == v.tobytes()
    m = np.ones(N, bool)
    for a, z in P.interval_queries(N, MID):
        got = S.interval_figures(runs, a, z)
        want = segments_ref.figures(v, m, a, z)
        assert got[0] == want[0] == z - a and got[5] == want[5]
        assert all(same(p, q) for p, q in zip(got[1:5], want[1:5])), (got, want)


def test_anchor_windows_give_what_the_whole_vector_gives():
    import matrixover_ref
    import profileover_ref
    whole = cpu.synth_coverage(20240611, 3, 0, N, 0)
    windows = [whole[a:a + c] for a, c, _ in P.anchor_groups(N, MID)]
    far, near = P.anchors_whole(N, MID), P.anchors_windowed(N, MID)
    want = profileover_ref.profile([whole], far, -P.FLANK, 2 * P.FLANK + 1)
    got = profileover_ref.profile(windows, near, -P.FLANK, 2 * P.FLANK + 1)
    assert len(got) == len(want) and all(same(a, b) for g, w in zip(got, want) for a, b in zip(g, w))
    assert min(w[0] for w in want) < len(far) == max(w[0] for w in want)          # some columns are cut at the ends
    for what in ("mean", "count", "max"):
        assert matrixover_ref.same_bits(matrixover_ref.matrix(windows, near, -P.FLANK, 2 * P.FLANK, 4, what),
                                        matrixover_ref.matrix([whole], far, -P.FLANK, 2 * P.FLANK, 4, what))
