"""The numpy checker for prominence (tests/prominence_ref.py) against a literal loop of the definition and, for odd
windows, against scipy.signal.peak_prominences; prominence by bits, base by value (the sign of a zero base is open).
No GPU."""
import warnings

import numpy as np
import pytest

import prominence_ref as ref

DBL_MAX = float(np.finfo(np.float64).max)
KINDS = ["real", "depth", "constant", "up", "down", "zeros", "inf", "subnormal", "huge"]
SIZES = [1, 2, 5, 40, 97, 301]
WINDOWS = [1, 2, 3, 4, 11, 100, 101, 1001]                   # (1001: above every n)


def data(kind, n, rng):
    """the kinds of tests/test_sliding_percentile.py, minus nan"""
    if kind == "real":
        return rng.standard_normal(n) * 10.0
    if kind == "depth":
        return rng.integers(0, 8, n).astype(np.float64)
    if kind == "constant":
        return np.full(n, 3.25)
    if kind == "up":
        return np.sort(rng.standard_normal(n))
    if kind == "down":
        return -np.sort(rng.standard_normal(n))
    if kind == "zeros":
        return np.where(np.arange(n) % 2 == 0, 0.0, -0.0)
    if kind == "inf":
        return rng.choice(np.array([np.inf, -np.inf, 1.0, -1.0, 0.0]), n)
    if kind == "subnormal":
        return rng.integers(-50, 50, n).astype(np.float64) * 5e-324
    if kind == "huge":
        return rng.choice(np.array([DBL_MAX, -DBL_MAX, np.nextafter(DBL_MAX, 0), -np.nextafter(DBL_MAX, 0), 1e308]), n)
    raise ValueError(kind)


def same(got, want):
    """(prominence, base) pairs: prominence bit for bit, base by value"""
    return got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("kind", KINDS)
def test_checker_equals_the_literal_loop(kind):
    rng = np.random.default_rng(KINDS.index(kind))
    with np.errstate(over="ignore", invalid="ignore"):
        for n in SIZES:
            v = data(kind, n, rng)
            for W in WINDOWS:
                got, want = ref.prominence(v, W), ref.literal(v, W)
                assert same(got, want), (kind, n, W)
                assert not np.any(np.signbit(got[0])) and not np.any(np.isnan(got[0])), (kind, n, W)


def test_the_consequences_the_header_lists():
    v = np.array([1.0, 3.0, 3.0, 3.0, 2.0, 0.5, 2.5, 0.0, 7.0, 7.0, 1.0, 4.0])
    prom, base = ref.prominence(v, 101)
    assert prom.tolist() == [0, 2, 2, 2, 0, 0, 2, 0, 6, 6, 0, 0]       # plateaus share one figure; the ends get 0
    assert base[1] == 1.0 and base[6] == 0.5 and base[8] == 1.0 and base[0] == 1.0 and base[11] == 4.0
    prom, base = ref.prominence(v, 4)                                  # one base to the left, two to the right
    assert prom[8] == 6 and prom[9] == 0 and prom[6] == 2 and prom[1] == 0 and prom[3] == 0    # (a plateau wider than a reach)
    prom, base = ref.prominence(v, 1)
    assert not prom.any() and np.array_equal(base, v)
    prom, _ = ref.prominence(np.array([-np.inf, np.inf, np.inf, -np.inf, 0.0, -np.inf]), 11)
    assert prom.tolist() == [0, np.inf, np.inf, 0, np.inf, 0]


def test_clean_marks_the_windows_without_nan():
    v = np.zeros(30)
    v[10] = np.nan
    ok = ref.clean(v, 6)                                               # wL = 2, wR = 3: bases 7 .. 12 see base 10
    assert np.flatnonzero(~ok).tolist() == [7, 8, 9, 10, 11, 12]


@pytest.mark.parametrize("kind", ["real", "depth", "plateaus", "constant", "inf"])
def test_checker_equals_scipy_for_odd_windows(kind):
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(11 + len(kind))
    for n in (1, 2, 5, 40, 97, 301, 400):
        v = np.repeat(rng.integers(0, 9, n // 5 + 1), 5)[:n].astype(np.float64) if kind == "plateaus" else data(kind, n, rng)
        for W in (3, 5, 11, 101, 4095):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = signal.peak_prominences(v, np.arange(n), wlen=W)[0]
            got = ref.prominence(v, W)[0]
            if kind == "inf":                                          # (scipy subtracts equal infinities; the definition says 0)
                want = np.where(np.isnan(want), 0.0, want)
            assert got.tobytes() == (want + 0.0).tobytes(), (kind, n, W)
