"""GPU: cumulativesum (gdsp_sums.hip: the one-pass look-back, and the three launches kept behind GDSP_CUMSUM=3) against
the truth.

Bound: |got[k] - exact[k]| <= eps[k] = gamma_k sum|v[0..k]| at every k, exact[k] the exact prefix sum rounded once
(runsum_ref.py).  It is per position and it holds for any order of summation, so it does not see a lost low-order bit;
it does see a lost, doubled or misplaced term and a wrong carried prefix, because the inputs keep min|v| above
eps[n-1] (asserted).  On integer read depth nothing rounds and the result is np.cumsum's, bit for bit.

Lengths sit around the look-back's seams: chunks of 8192 bases, groups of 64 chunks (524 288 bases), and one case
beyond a super-group of 4096 chunks (33 554 432 bases)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import runsum_cases as rc
import runsum_ref as rr
from conftest import ROOT, bits_equal, first_diff
from oracle import cpu

pytestmark = pytest.mark.gpu

REAL = ("positive", "mixed", "smooth")


@pytest.fixture(scope="module")
def gd():
    import genodsp_amd
    assert genodsp_amd.device_count() >= 1
    return genodsp_amd


@functools.lru_cache(maxsize=None)
def _truth(kind):
    """(v, exact, eps) of the 1 000 003-base signal; a shorter case is a prefix of all three"""
    v = rc.cumsum_signal(kind)
    exact, eps = rr.cumsum_exact(v)
    return v, exact, eps


def _assert_within(got, v, exact, eps, what):
    n = got.size
    assert n <= 1 or np.abs(v).min() > eps[-1], (what, "the bound would not see a lost term")
    bad = ~(np.abs(got - exact) <= eps)                     # (a NaN is bad)
    if bad.any():
        k = int(np.argmax(bad))
        pytest.fail("%s n=%d: base %d is %r, exact %r, allowed +-%r (%d bases off)" % (what, n, k, got[k], exact[k], eps[k], int(bad.sum())))


def _assert_depth(got, v, what):
    want = np.cumsum(v)
    assert bits_equal(got, want), (what, v.size, first_diff(got, want))


@pytest.mark.parametrize("n", rc.CUMSUM_LENGTHS)
@pytest.mark.parametrize("kind", REAL)
def test_cumsum_real_within_exact_bound(kind, n, gd):
    v, exact, eps = _truth(kind)
    got = gd.cumulative_sum(gd.DeviceVector.from_numpy(v[:n])).numpy()
    _assert_within(got, v[:n], exact[:n], eps[:n], kind)


@pytest.mark.parametrize("n", rc.CUMSUM_LENGTHS)
def test_cumsum_depth_bit_identical(n, gd):
    v = rc.cumsum_signal("depth")[:n]
    _assert_depth(gd.cumulative_sum(gd.DeviceVector.from_numpy(v)).numpy(), v, "depth")


def test_cumsum_real_across_a_super_group(gd):
    """33 554 432 + 8192 + 5 multiples of 2^-30 in [16, 48): the third level of the look-back carries a real prefix"""
    v = rc.super_group(True)
    exact, eps = rr.cumsum_exact(v, "int64")
    got = gd.cumulative_sum(gd.DeviceVector.from_numpy(v)).numpy()
    _assert_within(got, v, exact, eps, "super-group")


def test_cumsum_depth_across_a_super_group(gd):
    v = rc.super_group(False)
    _assert_depth(gd.cumulative_sum(gd.DeviceVector.from_numpy(v)).numpy(), v, "super-group depth")


@pytest.mark.parametrize("with_nan", [True, False])
def test_cumsum_special_values(with_nan, gd):
    """an ordinary NaN at 40 000, +inf at 70 000 and -inf at 70 010 (same chunk) in read depth, and the infinities alone:
    the finite prefix and the stretch of +inf are the reference's bits, NaN from the same base on; sign and payload of a
    NaN are not pinned"""
    v = np.array(rc.cumsum_signal("depth")[:100003])
    if with_nan:
        v[40000] = np.nan
    v[70000], v[70010] = np.inf, -np.inf
    with np.errstate(invalid="ignore"):
        want = cpu.cumulative_sum(v)
    first_nan = 40000 if with_nan else 70010
    assert np.isfinite(want[:min(first_nan, 70000)]).all() and np.isnan(want[first_nan:]).all()
    got = gd.cumulative_sum(gd.DeviceVector.from_numpy(v)).numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)), first_diff(np.isnan(got).astype(np.float64), np.isnan(want).astype(np.float64))
    assert bits_equal(got[:first_nan], want[:first_nan]), first_diff(got[:first_nan], want[:first_nan])


CHILD = """
import sys
import numpy as np
sys.path[:0] = [%r, %r]
import runsum_cases as rc
import genodsp_amd as gd
out = []
for kind in ("depth",) + %r:
    v = rc.cumsum_signal(kind)
    for n in rc.CUMSUM_LENGTHS:
        out.append(gd.cumulative_sum(gd.DeviceVector.from_numpy(v[:n])).numpy())
np.save(sys.argv[1], np.concatenate(out))
"""


def test_cumsum_three_launch_form(tmp_path, gd):
    """GDSP_CUMSUM=3 is read once per process, so the three launches run in a fresh child; the parent applies the same
    two assertions to what it wrote"""
    path = str(tmp_path / "cumsum3.npy")
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), REAL)
    try:
        done = subprocess.run([sys.executable, "-c", code, path], env={**os.environ, "GDSP_CUMSUM": "3"}, timeout=120,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired as e:
        pytest.fail("the child ran out of time: %s" % (e.stderr,))
    assert done.returncode == 0, done.stderr
    got = np.load(path)
    assert got.size == 4 * sum(rc.CUMSUM_LENGTHS)
    at = 0
    for kind in ("depth",) + REAL:
        for n in rc.CUMSUM_LENGTHS:
            part, at = got[at:at + n], at + n
            if kind == "depth":
                _assert_depth(part, rc.cumsum_signal("depth")[:n], "three launches, depth")
            else:
                v, exact, eps = _truth(kind)
                _assert_within(part, v[:n], exact[:n], eps[:n], "three launches, " + kind)
