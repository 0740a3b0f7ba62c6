"""GPU: localmax/localmin/bestmax/bestmin on NaN, infinities, signed zeros, the largest and smallest doubles and
plateaus, on every route of gdsp_extrema.hip and gdsp_longwin.hip and at their seams, held to the reference's table
(tests/extrema_cases.py; tests/test_extrema_cases.py holds the oracle itself to it).  dilate/erode through the block
form and slidingpercentile's P = 0 / 100 claim ride along on the same inputs."""
import functools

import numpy as np
import pytest

import extrema_cases as ec
from conftest import bits_equal, first_diff
from oracle import cpu

pytestmark = pytest.mark.gpu

FILLS = (0.0, cpu.DBL_MAX, -7.0, float("nan"))
BATCH_WINDOWS = tuple(W for W in ec.WINDOWS if W <= 8190)       # the batch entry points stop where one LDS tile does


@pytest.fixture(scope="module")
def gd():
    import genodsp_amd
    assert genodsp_amd.device_count() >= 1
    return genodsp_amd


def seam(W):
    """outputs per workgroup (per segment in gdsp_longwin.hip): where one tile's answers end and the next one's begin"""
    if W <= 4:
        return 4096                                              # EX_TILE, direct scan
    if W <= 3584:
        G = 16 if W >= 17 else (8 if W >= 9 else 4)
        return (256 - ((W - 1) // G + 1)) * G                    # block form; 2 fewer when the staged tile is shifted
    if W <= 8190:
        tile = 1024                                              # extrema_launch's choice for the segment scans
        while tile < 2 * (W - 1) and 2 * (2 * tile + W + 2) <= 18432:
            tile *= 2
        return tile
    return W


@functools.lru_cache(maxsize=None)
def vectors(W):
    """[(name, vector)]: the cases themselves, then each at a seam.  A NaN run starts at the seam's last base, on it
    and one past it (and two bases earlier, where the shifted block form has its seam); the other cases begin five
    bases before a seam -- where the cases are longer than several tiles anyway (above 3584) only the NaN runs."""
    rng = np.random.default_rng(W)
    out = list(ec.special_cases(W, rng).items())
    s = seam(W)
    _, first = ec.nan_runs(W, np.random.default_rng(0))
    at = -(-(first + 3) // s) * s                                # the first seam the run can be moved to
    for k in ((-3, -2, -1, 0, 1) if 5 <= W <= 3584 else (-1, 0, 1)):
        x, start = ec.nan_runs(W, rng, lead=at + k - first)
        assert start == at + k and np.isnan(x[start]) and not np.isnan(x[start - 1])
        out.append(("nan_runs@%+d" % k, x))
    if W <= 3584:
        for name, x in ec.special_cases(W, rng).items():
            if name not in ec.NAN_CASES:
                out.append((name + "@seam", np.concatenate([rng.standard_normal(s - 5) * 5, x])))
    return out


@functools.lru_cache(maxsize=None)
def classes(W, index, window):
    return ec.classify(vectors(W)[index][1], window)


def _params(windows):
    """one test per window; above 4096 one per vector (every tie of a long plateau costs the oracle a rescan)"""
    for W in windows:
        if W <= ec.BIG_W:
            yield pytest.param(W, None, id=str(W))
        else:
            for i, name in enumerate(ec.CASES):
                yield pytest.param(W, i, id="%d-%s" % (W, name))
            yield pytest.param(W, -1, id="%d-seams" % W)


def _chosen(W, which):
    v = vectors(W)
    if which is None:
        return list(range(len(v)))
    return [which] if which >= 0 else list(range(len(ec.CASES), len(v)))


@pytest.mark.parametrize("W,which", _params(ec.WINDOWS))
def test_best_extrema_on_special_values(W, which, gd):
    """Fails at an all-NaN window without ex_best: the kernels' picks ignore NaN and hand back their pad, -inf from
    bestmax and +inf from bestmin, where the reference answers NaN."""
    for i in _chosen(W, which):
        name, x = vectors(W)[i]
        d = gd.DeviceVector.from_numpy(x)
        for want_max in (True, False):
            got = gd.best_extrema(d, W, want_max).numpy()
            bad = ec.check_best(got, x, W, want_max, classes(W, i, W))
            assert bad is None, (name, x.size, want_max, bad, got[bad[0]])


@pytest.mark.parametrize("W,which", _params(ec.WINDOWS))
def test_local_extrema_on_special_values(W, which, gd):
    N = W | 1
    for i in _chosen(W, which):
        name, x = vectors(W)[i]
        d = gd.DeviceVector.from_numpy(x)
        for want_max in (True, False):
            for fill in FILLS:
                got = gd.local_extrema(d, N, want_max, fill).numpy()
                bad = ec.check_local(got, x, N, want_max, fill, classes(W, i, N))
                assert bad is None, (name, x.size, want_max, fill, bad, got[bad[0]])
    if which is None:
        name, x = vectors(W)[0]                                  # the two spellings of the command line
        d = gd.DeviceVector.from_numpy(x)
        assert ec.check_local(gd.localmax(d, N).numpy(), x, N, True, 0.0, classes(W, 0, N)) is None
        assert ec.check_local(gd.localmin(d, N).numpy(), x, N, False, cpu.DBL_MAX, classes(W, 0, N)) is None


@pytest.mark.parametrize("W", BATCH_WINDOWS)
def test_batched_extrema_on_special_values(W, gd):
    """every vector of a window in one *_batch call: more than the 32 of one launch table; then once more with a
    vector shorter than the half window, which sends extrema_batch vector by vector.  Both are held to the checkers,
    not to the single call."""
    N = W | 1 if W < 8190 else W - 1                             # (8191 is past what the batch entry points take)
    rng = np.random.default_rng(W + 1)
    vecs = [x for _, x in vectors(W)]
    own = len(vecs)
    lead = 0
    while len(vecs) < 34:                                        # NaN runs at other alignments fill the table
        lead += 1
        vecs.append(ec.nan_runs(W, rng, lead=lead)[0])
    assert all(x.size >= W for x in vecs)
    short = ec.nan_runs(2, rng)[0][:max(1, (W - 1) // 2 - 1)]
    cls_w = [classes(W, i, W) if i < own else ec.classify(x, W) for i, x in enumerate(vecs)]
    cls_n = [classes(W, i, N) if i < own else ec.classify(x, N) for i, x in enumerate(vecs)]
    for extra in ([], [short]):
        xs = vecs + extra
        cw = cls_w + [ec.classify(x, W) for x in extra]
        cn = cls_n + [ec.classify(x, N) for x in extra]
        ds = [gd.DeviceVector.from_numpy(x) for x in xs]
        for want_max in (True, False):
            outs = gd.best_extrema_batch(ds, W, want_max)
            for i, (x, o) in enumerate(zip(xs, outs)):
                got = o.numpy()
                bad = ec.check_best(got, x, W, want_max, cw[i])
                assert bad is None, ("best", i, x.size, want_max, len(extra), bad, got[bad[0]])
            fill = FILLS[(W + want_max + len(extra)) % 4]
            outs = gd.local_extrema_batch(ds, N, want_max, fill)
            for i, (x, o) in enumerate(zip(xs, outs)):
                got = o.numpy()
                bad = ec.check_local(got, x, N, want_max, fill, cn[i])
                assert bad is None, ("local", i, x.size, want_max, fill, len(extra), bad, got[bad[0]])


@pytest.mark.parametrize("L", [17, 101, 1001])
def test_dilate_erode_block_form_on_nan_and_infinities(L, gd):
    """dilate asks `v > T` at base 0 and `!(v <= T)` elsewhere, erode `v > T`: with T = -inf the two part ways on NaN
    and agree on -inf.  The reaches here take gdsp_morph_blocks; the NaN case starts with a NaN at base 0."""
    left, right = gd.split_length(L)
    assert 17 <= left + right + 1 <= 3584                       # gdsp_morph_blocks_available
    cases = ec.special_cases(L, np.random.default_rng(L))
    for name in ("nan_runs", "infinities"):
        x = cases[name]
        d = gd.DeviceVector.from_numpy(x)
        for T in (0.0, -np.inf):
            for lr in ((left, right), (right, left), (0, L), (L, 0)):
                got = gd.dilate(d, lr[0], lr[1], T).numpy()
                want = cpu.dilate(x, lr[0], lr[1], T)
                assert bits_equal(got, want), ("dilate", name, T, lr, first_diff(got, want))
                got = gd.erode(d, lr[0], lr[1], T).numpy()
                want = cpu.erode(x, lr[0], lr[1], T)
                assert bits_equal(got, want), ("erode", name, T, lr, first_diff(got, want))


def test_sliding_percentile_ends_are_best_extrema_on_infinities_and_subnormals(gd):
    """P = 0 and P = 100 print what bestmin and bestmax print (README), here on +-inf, +-DBL_MAX and subnormals"""
    W = 101
    cases = ec.special_cases(W, np.random.default_rng(W))
    for name in ec.NO_NAN_NO_MINUS_ZERO:
        x = cases[name]
        d = gd.DeviceVector.from_numpy(x)
        for p, want_max in ((0, 0), (100000, 1)):
            got = gd.sliding_percentile(d, W, p).numpy()
            want = cpu.best_extrema(x, W, want_max)
            assert bits_equal(got, want), (name, p, first_diff(got, want))
