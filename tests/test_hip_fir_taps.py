"""GPU: FIR plans with ARBITRARY taps (gdsp_fir_plan_create / gdsp_fir_apply, gd.FirPlan) on every route behind them:
the compile-time W=101 kernel, the run-time-W kernel with its LDS stages of 1026 taps, and the W=101 sliding-accumulator
kernels of gdsp_fir_slide.hip.  `smooth` runs the same kernels but only ever with Hann windows -- mirrored, positive,
free of zeros -- which cannot tell a tap index running the wrong way from the right one, or a kernel that assumes
w[W-1-k] == w[k] from one that does not.

Expected values: the restated reference's loop (cpu.fir) bit for bit in EXACT mode; in FMA mode the bits of one fused
multiply-add per tap in ascending order from +0.0 (fir_ref.fma_chain, exact integer arithmetic) at the positions where
the kernels' paths change, and the suite's bound W * 2^-52 * sum|w_k v_k| against cpu.fir everywhere; the taps
themselves for a signal of impulses (fir_ref.impulse_readout), in both modes.

Windows: 1 (a scalar), 3 / 9 / 11 (one and two groups of 9 taps), 99 / 103 (run-time kernel) around 101 (compiled),
1025 (one ragged stage), 1027 (a second stage of one tap), 2053 and 3079 (a last stage of one tap after two and three
full ones), 5001.  Lengths: 1, 2, around the half window and the window, around one and two tiles of 2304 outputs, and one
with whole interior tiles that take the aligned staging path."""
import contextlib
import functools

import numpy as np
import pytest

import fir_ref as fr
from conftest import bits_equal, first_diff
from oracle import cpu

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SEED = 20240611
TILE = fr.TILE
WINDOWS = [1, 3, 9, 11, 99, 101, 103, 1025, 1027, 2053, 3079, 5001]


def lengths(W):
    h = (W - 1) // 2
    interior = min(max(9221, 2 * TILE + 2 * W + 5), 15000)
    return sorted({n for n in (1, 2, h, h + 1, W - 1, W, W + 1, 2303, 2304, 2305, 4609, interior) if n >= 1})


GRID = [(W, n) for W in WINDOWS for n in lengths(W)]


@pytest.fixture(scope="module")
def gd():
    import genodsp_amd
    assert genodsp_amd.device_count() >= 1
    return genodsp_amd


@contextlib.contextmanager
def plan_of(gd, w):
    plan = gd.FirPlan(w)
    try:
        yield plan
    finally:
        plan.close()


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def signal(kind, n):
    """as test_hip_parity._signal (depth, real, noise), and "odd": noise with NaN, infinities, -0.0, 1e300 and 5e-324
    as test_hip_fir_slide._signal"""
    if kind == "depth":
        return _frozen(cpu.synth_coverage(SEED, 3, 0, n, 0))
    if kind == "real":
        return _frozen(cpu.synth_coverage(SEED, 3, 0, n, 1))
    rng = np.random.default_rng(n * 7 + (kind == "odd"))
    x = rng.standard_normal(n) * 5
    if kind == "odd":
        k = rng.integers(0, n, size=max(4, n // 300))
        x[k[0::4]] = np.nan
        x[k[1::4]] = np.inf
        x[k[2::4]] = -np.inf
        x[k[3::4]] = -0.0
        x[rng.integers(0, n, size=4)] = 1e300
        x[rng.integers(0, n, size=4)] = 5e-324
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def taps(kind, W):
    return _frozen(fr.taps(kind, W))


@functools.lru_cache(maxsize=None)
def oracle(W, n, tk, sk):
    """cpu.fir of the case, computed once for the tests that share it"""
    return _frozen(cpu.fir(signal(sk, n), taps(tk, W)))


def apply(gd, w, x, mode):
    with plan_of(gd, w) as plan:
        return plan.apply(gd.DeviceVector.from_numpy(x), mode=mode).numpy()


# ------------------------------------------------------------------------------------------------ impulse read-out ----

@pytest.mark.parametrize("mode", ["exact", "fma"])
@pytest.mark.parametrize("W", WINDOWS)
def test_impulses_read_the_taps_out_backwards(W, mode, gd):
    """1.0 every W + 37 bases (so the impulses drift across the tiles' seams and the taps' stages), at both ends and
    either side of the first two seams: every output is one tap, exactly, or +0.0"""
    w = taps("distinct", W)
    mode = gd.FIR_EXACT if mode == "exact" else gd.FIR_FMA
    with plan_of(gd, w) as plan:
        for n in lengths(W):
            wanted = list(range(19 % n, n, W + 37)) + [0, n - 1, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE]
            for impulses in fr.spread([p for p in wanted if p < n], W):
                x, want = fr.impulse_readout(n, w, impulses)
                got = plan.apply(gd.DeviceVector.from_numpy(x), mode=mode).numpy()
                assert bits_equal(got, want), (n, impulses[:4], first_diff(got, want))


# ------------------------------------------------------------------------------------------------------ EXACT mode ----

@pytest.mark.parametrize("W,n", GRID)
def test_exact_mode_gives_the_reference_bits(W, n, gd):
    for tk in ("noise", "sparse", "dyadic"):
        w = taps(tk, W)
        with plan_of(gd, w) as plan:
            for sk in ("depth", "real", "noise"):
                got = plan.apply(gd.DeviceVector.from_numpy(signal(sk, n)), mode=gd.FIR_EXACT).numpy()
                want = oracle(W, n, tk, sk)
                assert bits_equal(got, want), (tk, sk, first_diff(got, want))
            if n > 40:
                # NaN, infinities, signed zeros, huge and tiny magnitudes: the same NaNs in the same places (their sign
                # and payload are not pinned, as in test_pointwise_bit_exact), the same bits everywhere else
                got = plan.apply(gd.DeviceVector.from_numpy(signal("odd", n)), mode=gd.FIR_EXACT).numpy()
                want = oracle(W, n, tk, "odd")
                nan = np.isnan(want)
                assert np.array_equal(np.isnan(got), nan), (tk, first_diff(np.isnan(got) * 1.0, nan * 1.0))
                assert bits_equal(got[~nan], want[~nan]), (tk, first_diff(got[~nan], want[~nan]))


# -------------------------------------------------------------------------------------------------------- FMA mode ----

@pytest.mark.parametrize("W,n", GRID)
def test_fma_mode_is_the_ascending_fused_chain(W, n, gd):
    """both FIR kernels document one v_fma_f64 per tap in ascending tap order from +0.0: a bit-exact function of the
    input.  A kernel that fuses in another order, drops a tap worth less than the bound or contracts the wrong operation
    stays within the bound and fails here."""
    pos = fr.sample_positions(n, W)
    for tk in ("noise", "sparse"):
        w = taps(tk, W)
        with plan_of(gd, w) as plan:
            for sk in ("real", "noise"):
                x = signal(sk, n)
                got = plan.apply(gd.DeviceVector.from_numpy(x), mode=gd.FIR_FMA).numpy()
                want = oracle(W, n, tk, sk)
                scale = cpu.fir(np.abs(x), np.abs(w))
                assert np.all(np.abs(got - want) <= W * 2 * EPS * scale), (tk, sk, first_diff(got, want))
                chain = fr.fma_chain(x, w, pos)
                assert bits_equal(got[pos], chain), (tk, sk, pos[first_diff(got[pos], chain)])
    # nothing rounds: fused, unfused and any order are the same numbers
    got = apply(gd, taps("dyadic", W), signal("depth", n), gd.FIR_FMA)
    want = oracle(W, n, "dyadic", "depth")
    assert bits_equal(got, want), ("dyadic", first_diff(got, want))


@pytest.mark.parametrize("n", [2304, 9221])
@pytest.mark.parametrize("W", [21, 101, 301, 1027])
def test_smooth_fma_is_the_fused_chain_over_the_hann_window(W, n, gd):
    """the order smooth_local_extrema's FMA tests rely on, here pinned against exact arithmetic"""
    w = cpu.hann_window(W)
    pos = fr.sample_positions(n, W)
    for sk in ("real", "noise"):
        x = signal(sk, n)
        got = gd.smooth(gd.DeviceVector.from_numpy(x), W, mode=gd.FIR_FMA).numpy()
        chain = fr.fma_chain(x, w, pos)
        assert bits_equal(got[pos], chain), (sk, pos[first_diff(got[pos], chain)])


@pytest.mark.parametrize("W", [21, 101, 301, 1027])
def test_smooth_batch_fma_is_the_fused_chain_over_the_hann_window(W, gd):
    w = cpu.hann_window(W)
    xs = [signal(sk, n) for sk, n in (("real", 9221), ("noise", 2304), ("noise", 1), ("real", 4609), ("noise", 700))]
    outs = gd.smooth_batch([gd.DeviceVector.from_numpy(x) for x in xs], W, mode=gd.FIR_FMA)
    for x, o in zip(xs, outs):
        pos = fr.sample_positions(x.size, W, cap=32)
        got, chain = o.numpy()[pos], fr.fma_chain(x, w, pos)
        assert bits_equal(got, chain), (x.size, pos[first_diff(got, chain)])


# ---------------------------------------------------------------------------------------------------- W=101 routes ----

@pytest.mark.parametrize("tk", ["noise", "mirrored"])
@pytest.mark.parametrize("strip", [None, "512"])
@pytest.mark.parametrize("slide", [None, "0", "1", "2"])
def test_w101_plans_give_the_reference_bits_whatever_route_is_asked_for(slide, strip, tk, gd, monkeypatch):
    """GDSP_FIR_SLIDE (read per call) sends exact W=101 to the sliding-accumulator kernels, which compute w[m] x[j] once
    for taps m and 100-m: right for mirrored taps, a different filter for any others -- those must stay on the direct
    kernel whatever the variable says"""
    for name, value in (("GDSP_FIR_SLIDE", slide), ("GDSP_FIR_SLIDE_STRIP", strip)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    w = taps(tk, 101)
    with plan_of(gd, w) as plan:
        for n in (1, 50, 101, 526, 4110, 9221):
            for sk in ("real", "noise"):
                got = plan.apply(gd.DeviceVector.from_numpy(signal(sk, n)), mode=gd.FIR_EXACT).numpy()
                want = oracle(101, n, tk, sk)
                assert bits_equal(got, want), (n, sk, first_diff(got, want))


# -------------------------------------------------------------------------------------------------------- refusals ----

def test_plans_refuse_what_they_cannot_do(gd):
    v = gd.DeviceVector.from_numpy(np.ones(100))
    for bad in (np.ones(4), np.ones(100), np.zeros(0)):                    # even, and no taps at all
        with pytest.raises(gd.GdspError):
            gd.FirPlan(bad)
    for value in (np.nan, np.inf, -np.inf):                               # inf * 0 is NaN: zero padding would not be skipping
        for W, k in ((1, 0), (7, 0), (7, 6), (101, 50), (1027, 1026)):
            w = np.ones(W)
            w[k] = value
            with pytest.raises(gd.GdspError):
                gd.FirPlan(w)
    for W in (7, 101):
        with plan_of(gd, taps("noise", W)) as plan:
            with pytest.raises(gd.GdspError):
                plan.apply(v, mode=gd.FIR_HANN)                            # a plan has taps, not a window to take apart
            with pytest.raises(gd.GdspError):
                plan.apply(v, out=v)                                       # out of place only
            got = plan.apply(v).numpy()                                    # and it still works after refusing
            assert bits_equal(got, cpu.fir(np.ones(100), taps("noise", W)))


def test_an_empty_vector_is_left_alone(gd):
    a = gd.DeviceVector.from_numpy(np.full(8, 7.0))
    b = gd.DeviceVector.from_numpy(np.full(8, -3.0))
    for W in (7, 101):
        with plan_of(gd, taps("noise", W)) as plan:
            for mode in (gd.FIR_EXACT, gd.FIR_FMA):
                plan.apply(gd.DeviceVector(0, buf=a.buf), out=gd.DeviceVector(0, buf=b.buf), mode=mode)
    gd.sync()
    assert bits_equal(a.numpy(), np.full(8, 7.0)) and bits_equal(b.numpy(), np.full(8, -3.0))
