"""CPU: the custom-tap FIR helpers (fir_ref.py) against exact rationals and against the restated reference -- the
evidence that the bits the GPU tests ask for are the right ones, and that they tell a fused chain from an unfused one,
before a GPU is involved."""
from fractions import Fraction

import numpy as np
import pytest

import fir_ref as fr
from conftest import bits_equal, first_diff
from oracle import cpu

EPS = 2.0 ** -53
SEED = 20240611


def _signal(kind, n, rng):
    if kind == "depth":
        return cpu.synth_coverage(SEED, 3, 0, n, 0)
    if kind == "real":
        return cpu.synth_coverage(SEED, 3, 0, n, 1)
    return rng.standard_normal(n) * 5


def test_one_step_is_the_correctly_rounded_rational():
    """the integer form of a step against float(Fraction), which CPython rounds correctly: ordinary values, ties,
    cancellation to zero, subnormal results and results that underflow to a signed zero"""
    rng = np.random.default_rng(1)
    cases = [(rng.standard_normal(), rng.standard_normal() * 5, rng.standard_normal() * 30) for _ in range(2000)]
    cases += [(1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, 2.0 ** -105),        # exact result needs 106 bits
              (3.0, 2.0 ** -53, 1.0), (1.0, 2.0 ** -53, 1.0),            # above a tie, and a tie (to even)
              (0.1, 10.0, -1.0), (0.1, 10.0, 0.0),                       # fused: the product's rounding error survives
              (2.5, 4.0, -10.0), (-2.5, 4.0, 10.0),                      # exact zero: +0.0
              (-0.0, 3.0, 0.0), (0.0, -3.0, 0.0),
              (5e-324, 0.5, 0.0), (5e-324, 0.75, 0.0), (-5e-324, 0.25, 0.0), (-1e-200, 1e-200, 0.0),
              (1e-160, 1e-160, 5e-324), (2.0 ** -1000, 2.0 ** -60, 2.0 ** -1070), (1e300, 1e-300, 1e-320)]
    for w, x, acc in cases:
        want = float(Fraction(w) * Fraction(x) + Fraction(acc))
        got = fr.fma_step(w, x, acc)
        assert got == want and np.signbit(got) == np.signbit(want), (w, x, acc, got, want)
    assert np.signbit(fr.fma_step(-1e-200, 1e-200, 0.0))                 # IEEE: a negative sum that rounds to nothing is -0.0
    assert fr.fma_step(0.1, 10.0, -1.0) == 2.0 ** -54                    # unfused: 0.1 * 10.0 rounds to 1.0 and this is 0.0


def test_fma_chain_is_the_chain_in_rationals():
    rng = np.random.default_rng(2)
    for W, n in ((1, 5), (7, 3), (7, 40), (101, 150), (101, 60)):
        x, w = rng.standard_normal(n) * 5, fr.taps("noise", W)
        h = (W - 1) // 2
        pos = fr.sample_positions(n, W, tile=16)
        got = fr.fma_chain(x, w, pos)
        for i, g in zip(pos, got):
            acc = 0.0
            for k in range(W):
                if 0 <= i - h + k < n:
                    acc = float(Fraction(float(w[k])) * Fraction(float(x[i - h + k])) + Fraction(acc))
            assert g == acc and np.signbit(g) == np.signbit(acc), (W, n, i)


def test_fma_chain_refuses_what_it_cannot_state():
    with pytest.raises(AssertionError):
        fr.fma_chain(np.array([1.0, np.inf]), np.ones(3), [0])
    with pytest.raises(AssertionError):
        fr.fma_chain(np.ones(4), np.array([1.0, np.nan, 1.0]), [0])
    with pytest.raises(AssertionError):
        fr.fma_chain(np.ones(4), np.ones(3), [4])


@pytest.mark.parametrize("W,n", [(1, 9), (9, 4), (101, 2500), (1027, 2400), (1027, 700), (2053, 4700)])
def test_fma_chain_equals_the_oracle_where_nothing_rounds(W, n):
    """dyadic taps on read depth: every product and every partial sum is a multiple of 2^-10 far below 2^43, so the
    reference's unfused loop and the fused chain are the same exact numbers"""
    x, w = _signal("depth", n, None), fr.taps("dyadic", W)
    assert np.all(x == np.floor(x)) and np.abs(x).max() < 2 ** 30
    pos = fr.sample_positions(n, W)
    got, want = fr.fma_chain(x, w, pos), cpu.fir(x, w)[pos]
    assert bits_equal(got, want), pos[first_diff(got, want)]


@pytest.mark.parametrize("W,n", [(101, 5000), (1027, 5000)])
@pytest.mark.parametrize("tk", ["noise", "sparse", "mirrored"])
def test_fma_chain_is_within_one_rounding_per_tap_of_the_oracle(W, n, tk):
    rng = np.random.default_rng(W + n)
    for sk in ("real", "noise"):
        x, w = _signal(sk, n, rng), fr.taps(tk, W)
        pos = fr.sample_positions(n, W)
        got, want = fr.fma_chain(x, w, pos), cpu.fir(x, w)[pos]
        scale = cpu.fir(np.abs(x), np.abs(w))[pos]
        assert np.all(np.abs(got - want) <= W * 2 * EPS * scale), (sk, float(np.max(np.abs(got - want) / scale)))


@pytest.mark.parametrize("W", [101, 1027])
def test_fused_and_unfused_differ_often_enough_to_be_told_apart(W):
    """on noise taps and a noise signal the fused chain and the reference's unfused loop disagree at most positions:
    a GPU kernel that meets fma_chain's bits is therefore known to fuse, and one that meets cpu.fir's not to"""
    n = 5000
    x, w = _signal("noise", n, np.random.default_rng(W)), fr.taps("noise", W)
    pos = fr.sample_positions(n, W)
    assert len(pos) >= 40
    got, want = fr.fma_chain(x, w, pos), cpu.fir(x, w)[pos]
    differ = int(np.count_nonzero(got.view(np.uint64) != want.view(np.uint64)))
    print("W=%d: fused differs from unfused at %d of %d positions" % (W, differ, len(pos)))
    assert 4 * differ >= len(pos), (differ, len(pos))


@pytest.mark.parametrize("W,n,impulses", [
    (1, 6, [0, 2, 5]),
    (7, 60, [0, 20, 30, 59]),                       # both ends
    (101, 700, [10, 300, 660]),                     # closer than h to either end
    (101, 60, [17]),                                # vector shorter than the window
    (101, 50, [0]), (101, 50, [49]),
    (1027, 2500, [3, 1200, 2499]),
    (1027, 400, [399]),
])
def test_impulse_readout_equals_the_oracle(W, n, impulses):
    w = fr.taps("distinct", W)
    x, want = fr.impulse_readout(n, w, impulses)
    assert x.sum() == len(impulses)
    got = cpu.fir(x, w)
    assert bits_equal(got, want), first_diff(got, want)
    pos = fr.sample_positions(n, W, tile=64)
    assert bits_equal(fr.fma_chain(x, w, pos), want[pos])
    flipped = cpu.fir(x, w[::-1].copy())            # what a tap index running the wrong way would give
    assert (W == 1) or not bits_equal(flipped, want)


def test_impulse_readout_refuses_impulses_that_share_an_output():
    with pytest.raises(AssertionError):
        fr.impulse_readout(300, fr.taps("distinct", 101), [10, 110])
    fr.impulse_readout(300, fr.taps("distinct", 101), [10, 111])
    with pytest.raises(AssertionError):
        fr.impulse_readout(300, fr.taps("sparse", 101), [10])


def test_spread_keeps_every_list_a_window_apart():
    want = [0, 2303, 2304, 4607, 4608, 9220] + list(range(19, 9221, 138))
    sets = fr.spread(want, 101)
    assert sorted(p for s in sets for p in s) == sorted(set(want))
    assert all(b - a >= 101 for s in sets for a, b in zip(s, s[1:]))
    assert len(sets) <= 3


def test_sample_positions_cover_ends_seams_and_respect_the_cap():
    pos = fr.sample_positions(9221, 101)
    for p in (0, 1, 49, 50, 51, 9221 - 51, 9221 - 50, 9220, 2301, 2302, 2303, 2304, 2305, 2306, 4607, 4608, 9215, 9216, 9218):
        assert p in pos
    assert pos == sorted(set(pos)) and len(pos) <= 64 and pos == fr.sample_positions(9221, 101)
    assert fr.sample_positions(1, 101) == [0] and fr.sample_positions(2, 1) == [0, 1]
    for W, n in ((1027, 9221), (2053, 9221), (3079, 10771), (5001, 14615)):
        pos = fr.sample_positions(n, W)
        assert 16 <= len(pos) <= fr.position_cap(W) and len(pos) * W <= 1.1 * fr.TAP_STEPS
        assert all(0 <= p < n for p in pos) and {0, n - 1, (W - 1) // 2, 2303, 2304} <= set(pos)
    assert fr.position_cap(2053) == 64 and fr.position_cap(3079) == 48 and fr.position_cap(5001) == 32


def test_tap_families_are_what_they_are_called():
    for W in (1, 3, 101, 1027, 2053, 5001):
        for kind in fr.TAP_KINDS:
            w = fr.taps(kind, W)
            assert w.shape == (W,) and w.dtype == np.float64 and np.isfinite(w).all()
            assert bits_equal(w, fr.taps(kind, W))
        m = fr.taps("mirrored", W)
        assert bits_equal(m, m[::-1])
        d = fr.taps("distinct", W)
        assert len(set(d.tolist())) == W and (d != 0).all()
        s = fr.taps("sparse", W)
        nz = set(np.flatnonzero(s).tolist())
        assert {0, W - 1, (W - 1) // 2} <= nz
        if W > 1026:
            assert {1025, 1026} <= nz and {k for k in range(1025, W, 1026)} <= nz
            assert np.signbit(s[s == 0]).any() and not np.signbit(s[s == 0]).all()
        if W >= 101:
            a = fr.taps("noise", W)
            assert not np.any(a[:W // 2] == a[::-1][:W // 2])
