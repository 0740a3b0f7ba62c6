"""GPU: slidingsum on every route (gdsp_sums.hip: the LDS prefix form and the 16-element block form; gdsp_longwin.hip:
the whole-vector form) and `sum` over windows beyond 8192 bases (window_sum_wide_kernel) on real values, against the
truth.

Bound: |got[c] - exact[c]| <= allow[c] at every base, exact the exact window sum over the denominator rounded once and
allow what runsum_ref.py derives for the route: gamma_(2 (W + 4096) + 4) times the sum of |v| over the window and one
tile on either side for the tiled routes, the two prefixes' eps for the whole-vector route, gamma_len times the
window's sum of |v| for `sum`, each carried through the quotient.  None of them grows with the length of the vector
(the whole-vector route's grows with the position, as cumulativesum's does).  Where allow is 0 -- the `grid` signal,
multiples of 2^-30 whose sums cannot round -- the result is held bit for bit.  The bound does not see a lost low-order
bit; it does see a lost, doubled or misplaced term, a wrong carried value and a wrong denominator, because every case
asserts min|v| > 2 max(allow |denom|) first (test_runsum_ref.py shows each such mutant rejected on these signals).

Lengths sit around the kernels' own seams (runsum_cases.sliding_lengths): one base, the window +-1, one, two and three
workgroups' outputs +-1, and 130 003 bases; the whole-vector route also runs at 300 007, across cumulativesum's chunks
and groups.  All four signals pass the sensitivity condition on every route, `smooth` at 300 007 included.

OBSERVED keeps the largest |got - exact| / allow per (operator, route, signal): a record, not a threshold
(profiles/windowsum_real_bound.txt holds one run's)."""
import functools

import numpy as np
import pytest

import runsum_cases as rc
import runsum_ref as rr
from conftest import bits_equal, first_diff
from oracle import cpu

pytestmark = pytest.mark.gpu

OBSERVED = {}
KEPT = (rc.WINDOW_LONG_N, rc.WINDOW_N, 100003)             # lengths that many cases share: their exact prefixes are kept


@pytest.fixture(scope="module")
def gd():
    import genodsp_amd
    assert genodsp_amd.device_count() >= 1
    return genodsp_amd


@functools.lru_cache(maxsize=None)
def _kept(kind, n):
    return rr.Prefix(rc.window_signal(kind)[:n], "int64" if kind == "grid" else None)


def _truth(kind, n):
    """(v, its exact prefix sums)"""
    v = rc.window_signal(kind)[:n]
    return v, (_kept(kind, n) if n in KEPT else rr.Prefix(v, "int64" if kind == "grid" else None))


def _assert_within(got, v, exact, allow, denom, key, what):
    """denom: one number, or one per base where it matters"""
    assert np.abs(v).min() > 2 * (allow * np.abs(denom)).max(), (what, "the bound would not see a lost term")
    err = np.abs(got - exact)
    open_ = allow > 0
    if open_.any():
        worst = float((err[open_] / allow[open_]).max())
        OBSERVED[key] = max(OBSERVED.get(key, 0.0), worst)
        print("%s: largest |got - exact| / allow = %.3g" % (what, worst))
    bad = ~(err <= allow)                                   # (a NaN is bad)
    if bad.any():
        k = int(np.argmax(bad))
        pytest.fail("%s: base %d is %r, exact %r, allowed +-%r (%d bases off)" % (what, k, got[k], exact[k], allow[k], int(bad.sum())))
    assert bits_equal(got[~open_], exact[~open_]), (what, first_diff(got[~open_], exact[~open_]))


SLIDING = [(W, kind) for ws in rc.SLIDING_WINDOWS.values() for W in ws for kind in rc.WINDOW_SIGNALS]


@pytest.mark.parametrize("W,kind", SLIDING, ids=["%d-%s" % c for c in SLIDING])
def test_sliding_sum_real_within_exact_bound(W, kind, gd):
    route = rc.sliding_route(W)
    for n in rc.sliding_lengths(W):
        v, prefix = _truth(kind, n)
        sl = rr.Sliding(prefix, W)
        assert sl.tiled == (route != "whole-vector")
        d = gd.DeviceVector.from_numpy(v)
        for denom in rc.sliding_denoms(W):
            exact, allow = sl.over(denom)
            got = gd.sliding_sum(d, W, denom).numpy()
            _assert_within(got, v, exact, allow, denom, ("slidingsum", route, kind),
                           "slidingsum %s W=%d n=%d denom=%r" % (kind, W, n, denom))
            if kind == "grid" and denom in (1.0, 0.25) and (sl.tiled or n <= rc.WINDOW_LONG_N):
                assert not allow.any()                      # held bit for bit


SUMS = [(W, kind) for W in rc.SUM_WINDOWS for kind in rc.WINDOW_SIGNALS]


@pytest.mark.parametrize("W,kind", SUMS, ids=["%d-%s" % c for c in SUMS])
def test_window_sum_real_beyond_8192(W, kind, gd):
    """a vector shorter than W is one window of n bases (n = 8192 for W = 8193: the route of the shorter windows, held
    to the same bound)"""
    for n in rc.sum_lengths(W):
        v, prefix = _truth(kind, n)
        for denom, actual, zero in rc.sum_params(W):
            exact, allow, is_sum = rr.window_exact(prefix, W, denom, actual, zero)
            got = gd.window_sum(gd.DeviceVector.from_numpy(v), W, denom, actual, zero).numpy()
            what = "sum %s W=%d n=%d denom=%r actual=%r" % (kind, W, n, denom, actual)
            assert bits_equal(got[~is_sum], exact[~is_sum]), (what, "a base that is no window's first is not the zero value")
            lengths = np.minimum(W, n - np.flatnonzero(is_sum)).astype(np.float64)
            dens = lengths if actual else np.full(lengths.size, denom)
            for route, part in (("wide", lengths > 8192), ("window of 8192 bases or fewer", lengths <= 8192)):
                if part.any():                              # (the ragged last window, or a vector shorter than W)
                    _assert_within(got[is_sum][part], v, exact[is_sum][part], allow[is_sum][part], dens[part],
                                   ("sum", route, kind), what)
            if kind == "grid":
                assert bits_equal(got, exact), (what, first_diff(got, exact))


@pytest.mark.parametrize("W", [100, 1000, 1025, 8192])
def test_window_sum_real_actual_length_up_to_8192(W, gd):
    """--denom=actual on real values where `sum` adds in the reference's order: the reference's bits, ragged last window
    included"""
    for kind in ("mixed", "smooth"):
        v = rc.window_signal(kind)[:100003]
        got = gd.window_sum(gd.DeviceVector.from_numpy(v), W, 1.0, True, -1.0).numpy()
        want = cpu.window_sum(v, W, use_actual=True, zero=-1.0)
        assert bits_equal(got, want), (kind, first_diff(got, want))
        exact, allow, _ = rr.window_exact(v, W, 1.0, True, -1.0)
        assert np.all(np.abs(got - exact) <= allow)
