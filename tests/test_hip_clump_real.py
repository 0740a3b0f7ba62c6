"""GPU: clump / anticlump (gdsp_clump.hip) on values whose running sums round, against exact arithmetic.

On read depth every prefix sum is exact and the kernel is held to the reference bit for bit (test_hip_parity.py,
test_hip_fullsize.py).  On reals no two orders of summation agree, and the honest statement is what ANY evaluation of
the same sums could give: runsum_ref.py computes the prefix sums exactly and returns the output under the strictest and
under the most lenient reading of every comparison P[j] <= P[i] that an error of gamma_k sum|d| per prefix allows.
Every correct implementation lies between the two, position by position; where they coincide (all of the natural class,
as it turns out) that is bit for bit.  The bound comes from the operation, not from the kernel.

Each case first asserts, from the checker alone, that it can tell something: strict has at least 3 separate runs,
covers 2 % to 98 % of the bases, and differs from lenient on less than the class's cap (runsum_cases.CAPS)."""
import functools

import numpy as np
import pytest

import runsum_cases as rc
import runsum_ref as rr
from conftest import bits_equal
from oracle import cpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gd():
    import genodsp_amd
    assert genodsp_amd.device_count() >= 1
    return genodsp_amd


@functools.lru_cache(maxsize=None)
def _group(cls, kind, n, above, pct):
    """(v, T, what runsum_ref knows about them for every L)"""
    v, T = rc.clump_input(cls, kind, n, above, pct)
    return v, T, rr.Clump(v, T, above, "int64" if cls == "grid" else None)


def _check(gd, cls, v, T, L, above, clump, one=1.0, zero=0.0):
    strict, lenient = clump.bounds(L)
    open_share = float(np.mean(strict != lenient))
    assert rr.runs(strict) >= 3 and 0.02 <= strict.mean() <= 0.98 and open_share < rc.CAPS[cls], (
        "the case decides too little", L, rr.runs(strict), float(strict.mean()), open_share)

    got = gd.clump(gd.DeviceVector.from_numpy(v), T, L, above, one, zero).numpy()
    bits = got.view(np.uint64)
    is_one = bits == np.float64(one).view(np.uint64)
    is_zero = bits == np.float64(zero).view(np.uint64)
    bad = ~(is_one | is_zero) | (strict & ~is_one) | (~lenient & ~is_zero)
    if bad.any():
        t = int(np.argmax(bad))
        pytest.fail("base %d of %d: got %r, strict %s, lenient %s (L=%d, T=%r, %s, %d bases wrong, open share %.5f %%)" % (
            t, v.size, got[t], strict[t], lenient[t], L, T, "clump" if above else "anticlump", int(bad.sum()), 100 * open_share))
    if open_share == 0:                                     # nothing left to rounding: the reference's bits
        assert bits_equal(got, cpu.clump(v, T, L, above, one, zero)), (L, T)


NATURAL = rc.clump_groups(("natural",))
TENTHS = rc.clump_groups(("tenths",))
GRID = [(g, L) for g in rc.clump_groups(("grid",)) for L in rc.lengths(g[2], g[3], g[5])]


@pytest.mark.parametrize("group", NATURAL, ids=[g[0] for g in NATURAL])
def test_clump_natural_signals(group, gd):
    """scaled depth, noise with raised islands and Hann-smoothed depth (`= smooth W=101 = clump T`); L on both sides of
    the 64-base flag word and the 4096-base chunk, and R' shifted across two and three chunks; vectors with a ragged
    and a whole last chunk"""
    _, cls, kind, n, above, pct = group
    v, T, clump = _group(cls, kind, n, above, pct)
    for L in rc.lengths(kind, n, pct):
        _check(gd, cls, v, T, L, above, clump)


@pytest.mark.parametrize("group,L", GRID, ids=["%s-L%d" % (g[0], L) for g, L in GRID])
def test_clump_grid_five_million(group, L, gd):
    """5 000 011 bases: more than 1024 scan chunks in the offsets pass; eps grows to some hundredths by the end"""
    _, cls, kind, n, above, pct = group
    v, T, clump = _group(cls, kind, n, above, pct)
    _check(gd, cls, v, T, L, above, clump)


@pytest.mark.parametrize("group", TENTHS, ids=[g[0] for g in TENTHS])
def test_clump_tenths_where_rounding_decides(group, gd):
    """every term is +-0.1 or +-0.2: the exact prefix sums tie over and over and each implementation breaks the ties its
    own way (1 % to 8 % of the bases are open) -- everything else is still pinned"""
    _, cls, kind, n, above, pct = group
    v, T, clump = _group(cls, kind, n, above, pct)
    for L in rc.lengths(kind, n, pct):
        _check(gd, cls, v, T, L, above, clump)


@pytest.mark.parametrize("kind,n,pct,L,one,zero", [("noise", 100003, 85, 4096, 7.0, -1.0), ("smooth", 20011, 25, 64, -2.0, 3.0)])
def test_clump_real_one_and_zero_values(kind, n, pct, L, one, zero, gd):
    v, T, clump = _group("natural", kind, n, pct == 85, pct)
    _check(gd, "natural", v, T, L, pct == 85, clump, one, zero)
