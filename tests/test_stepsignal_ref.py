"""CPU: stepsignal_ref's run-length arithmetic held to the array checkers on vectors short enough to build -- the step
signals of the 2^32 - 1 tests scaled down to n = 50 000 (steps at the quarters, single bases planted past the middle and
at the last base), and a ragged one whose runs share values.  Every figure bit for bit."""
import numpy as np
import pytest

from oracle import cpu

import correlate_ref
import histogram_ref
import lagcorr_ref
import stepsignal_ref as S
import xsum_ref
from sliding_percentile_ref import rank

N = 50000
PERCENTILES = (0, 25000, 50000, 74999, 75000, 75001, 99999, 100000)


def signals():
    x = S.step_intervals(N, N // 4, N // 2, 3 * (N // 4), [(N // 2 + 123, 1000.0), (N - 1, -500.0), (17, 0.375)])
    y = S.halves_intervals(N, N // 2, [(N // 2 - 1, 64.0), (N - 2, -8.5)])
    return x, y


def ragged():
    rng = np.random.default_rng(3)
    cuts = np.sort(rng.choice(np.arange(1, N), 40, replace=False)).tolist()
    vals = rng.choice([0.1, -0.7, 3.3, 1e-3, 12.0, -2.0 ** -20], 41).tolist()
    return [(a, z, v) for a, z, v in zip([0] + cuts, cuts + [N], vals)]


def array_of(intervals):
    s = np.array([a for a, _, _ in intervals], np.uint32)
    e = np.array([z for _, z, _ in intervals], np.uint32)
    return cpu.apply_intervals(np.zeros(N), s, e, np.array([v for _, _, v in intervals]))


def same_tuple(a, b):
    return len(a) == len(b) and all(xsum_ref.same(p, q) for p, q in zip(a, b))


CASES = {"steps": signals()[0], "halves": signals()[1], "ragged": ragged()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_runs_are_the_vector(name):
    runs = S.from_intervals(N, CASES[name])
    assert S.length(runs) == N
    assert S.to_array(runs).tobytes() == array_of(CASES[name]).tobytes()
    assert all(a[1] != b[1] for a, b in zip(runs[:-1], runs[1:]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_percentiles_minmax_stats_and_histogram(name):
    runs = S.from_intervals(N, CASES[name])
    v = array_of(CASES[name])
    ordered = np.sort(v)
    for p in PERCENTILES:
        assert S.percentile(runs, p) == ordered[rank(N, p)], p
    assert S.minmax(runs) == (ordered[0], ordered[-1])
    assert same_tuple(S.stats(runs), xsum_ref.stats(v))
    for edges in (histogram_ref.uniform_edges(-4.0, 1.0, 12), np.array([-600.0, -2.25, 0.0, 0.5, 0.50001, 7.0, 2000.0])):
        w = S.histogram_words(runs, edges)
        assert w == [int(c) for c in histogram_ref.words_of_sample(v, edges)]
        assert S.at_least(w) == [int((v >= e).sum()) for e in edges[:-1]]


def test_the_rank_rule_is_the_librarys():
    import genodsp_amd as gd
    for count in (1, 7, N, 2 ** 31 + 5, 2 ** 32 - 1):
        for p in PERCENTILES:
            assert rank(count, p) == gd.lib().gdsp_percentile_rank(count, p)


@pytest.mark.parametrize("pair", [("steps", "halves"), ("ragged", "steps"), ("steps", "steps")])
def test_correlation_and_lags(pair):
    xr, yr = (S.from_intervals(N, CASES[k]) for k in pair)
    x, y = (array_of(CASES[k]) for k in pair)
    assert same_tuple(S.correlation(xr, yr), correlate_ref.figures(x, y))
    fig, counts, cov, corr = S.lag_curve(xr, yr, -2, 5)
    wfig, wcounts, wcov, wcorr = lagcorr_ref.curve([(x, y)], -2, 5)
    assert same_tuple(fig, wfig) and counts == wcounts == [N - 2, N - 1, N, N - 1, N - 2]
    assert same_tuple(cov, wcov) and same_tuple(corr, wcorr)
    assert len(set(cov)) > 1                                            # the lags differ: the planted bases move


def test_shifted_pairs_count_every_overlap():
    xr, yr = (S.from_intervals(N, CASES[k]) for k in ("steps", "halves"))
    x, y = (array_of(CASES[k]) for k in ("steps", "halves"))
    for d in (-2, -1, 0, 1, 2, 777):
        got = {}
        for c, a, b in S.pairs_of(xr, yr, d):
            got[(a, b)] = got.get((a, b), 0) + c
        i0, i1 = max(0, -d), min(N, N - d)
        want = {}
        for a, b in zip(x[i0:i1].tolist(), y[i0 + d:i1 + d].tolist()):
            want[(a, b)] = want.get((a, b), 0) + 1
        assert got == want, d
