"""The inputs of the real-valued running-sum tests (test_runsum_ref.py on the CPU, test_hip_clump_real.py,
test_hip_cumsum_real.py and test_hip_windowsum_real.py on the GPU): fixed seeds, nothing here touches a GPU.

clump classes
  natural  three signals with islands of about 700, 3000 and 12 000 bases (shorter in short vectors) so that every L
           finds clumps: read depth (+1: a third of the synthetic depth is 0, which would put the 10th and the 25th
           percentile on a tie) times U(0.5, 1.5) times an enrichment, N(0, 5) noise plus a raise, and the enriched
           depth smoothed by the Hann window of 101.  An enriched island is raised a lot in 30 % of its 256-base
           blocks and little or not at all in the rest: that is what lets stretches that hold far more than 15 % of
           the chromosome average above its 85th percentile.  Depleted islands serve anticlump.
  grid     the noise signal rounded to multiples of 2^-30, 5 000 011 bases (more than 1024 scan chunks; int64 back end)
  tenths   where((t//50)%2==0, 0.3, 0.1) + 0.1 ((t//1000)%7==3) against 0.2: every term is +-0.1 or +-0.2, the exact
           prefix sum returns to the same values again and again and rounding decides
"""
import functools

import numpy as np

from oracle import cpu

SEED = 20240611
LENGTHS = (1, 7, 63, 64, 100, 4095, 4096, 4097, 5000, 9000)
SHORT = (1, 7, 63, 64, 100)
HIGH = 6.0                                      # an enriched island's raised blocks (depth and smooth)


def depth(n):
    return cpu.synth_coverage(SEED, 3, 0, n, 0)


def _islands(n):
    """(start, length, kind) with kind +1 enriched / -1 depleted, laid out left to right with gaps"""
    if n >= 50000:
        plan = [(12000, 1), (5600, -1), (12000, 1), (5600, -1), (12000, 1), (5600, -1), (3000, 1), (700, -1), (700, 1),
                (3000, -1), (700, 1)] * max(1, n // 100000)
    else:
        plan = [(700, 1), (300, -1), (150, 1), (300, -1), (700, 1), (150, -1), (300, 1)]
        plan = plan * (1 + n // 4000)
    total = sum(p[0] for p in plan)
    scale = min(1.0, 0.66 * n / total)
    gap = int((n - scale * total) / (len(plan) + 1))
    out, at = [], gap
    for length, kind in plan:
        length = max(8, int(length * scale))
        if at + length > n:
            break
        out.append((at, length, kind))
        at += length + gap
    return out


def _profile(n, base, low, high, down):
    """per base: `base` outside the islands, `down` in depleted ones, `high` in 30 % of the 256-base blocks of an
    enriched one and `low` in its other blocks"""
    f = np.full(n, base, np.float64)
    for at, length, kind in _islands(n):
        if kind < 0:
            f[at:at + length] = down
        else:
            blocks = (np.arange(length // 256 + 1) * 3) % 10 < 3
            f[at:at + length] = np.where(np.repeat(blocks, 256)[:length], high, low)
    return f


@functools.lru_cache(maxsize=None)
def natural(kind, n):
    rng = np.random.default_rng(SEED + n)
    if kind == "depth":
        v = (depth(n) + 1.0) * rng.uniform(0.5, 1.5, n) * _profile(n, 1.0, 1.0, HIGH, 0.01)
    elif kind == "noise":
        v = rng.standard_normal(n) * 5 + _profile(n, 0.0, 6.0, 32.0, -14.0)
    elif kind == "smooth":
        v = cpu.smooth((depth(n) + 1.0) * _profile(n, 1.0, 1.0, HIGH, 0.01), 101)
    else:
        raise ValueError(kind)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def grid(n=5000011):
    v = np.rint(natural("noise", n) * 2.0 ** 30) * 2.0 ** -30
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def tenths(n):
    t = np.arange(n)
    v = np.where((t // 50) % 2 == 0, 0.3, 0.1) + 0.1 * ((t // 1000) % 7 == 3)
    v.setflags(write=False)
    return v


def threshold(v, above, pct=None, on_grid=False):
    """above: the 85th percentile; anticlump: the 10th or 25th; + 0.0131 so that it is none of the signal's own values (a
    smoothed plateau that equals the threshold is a tie by construction); rounded to the grid if asked"""
    T = float(np.percentile(v, 85 if above else pct)) + 0.0131
    return float(np.rint(T * 2.0 ** 30) * 2.0 ** -30) if on_grid else T


# What the checker alone says about these inputs decides which L a (signal, n, percentile) is run with: a case is kept
# where `strict` has at least 3 separate runs, 2 % to 98 % of its bases set and an open share under the class's cap.
# Three stretches of 4095 or more bases cannot all average below a vector's 10th percentile, nor three of 9000 below
# its 25th; a vector of 4096 has no three stretches of 100 noisy bases above its 85th percentile; the tenths signal
# repeats every 7000 bases.
_LONG = (4095, 4096, 4097, 5000, 9000)
_DROPPED = {("depth", 100003, 10): _LONG, ("depth", 100003, 25): (9000,),
            ("noise", 100003, 10): _LONG, ("noise", 4095, 85): (63, 64, 100), ("noise", 4096, 85): (100,), ("noise", 4097, 85): (100,),
            ("smooth", 4095, 10): (100,), ("smooth", 4096, 10): (100,), ("smooth", 4097, 10): (100,),
            ("smooth", 100003, 10): (9000,), ("smooth", 100003, 25): (9000,),
            ("grid", 5000011, 10): _LONG, ("tenths", 20011, 20): _LONG, ("tenths", 100003, 20): (9000,)}
CAPS = {"natural": 0.001, "grid": 0.005, "tenths": 0.10}
NATURAL_N = (4095, 4096, 4097, 8193, 20011, 100003)
GRID_N = 5000011


def lengths(kind, n, pct):
    every = LENGTHS if n > 50000 else SHORT
    return tuple(L for L in every if L not in _DROPPED.get((kind, n, pct), ()))


def clump_groups(classes=("natural", "grid", "tenths")):
    """[(id, class, kind, n, above, pct)]: one (signal, threshold, direction) each; pct 85 means clump, 10 and 25 anticlump"""
    out = []
    if "natural" in classes:
        out += [("%s-%d-p%d" % (kind, n, pct), "natural", kind, n, pct == 85, pct)
                for kind in ("depth", "noise", "smooth") for n in NATURAL_N for pct in (85, 10, 25)]
    if "grid" in classes:
        out += [("grid-p%d" % pct, "grid", "grid", GRID_N, pct == 85, pct) for pct in (85, 10, 25)]
    if "tenths" in classes:
        out += [("tenths-%d" % n, "tenths", "tenths", n, False, 20) for n in (20011, 100003)]
    return out


def clump_input(cls, kind, n, above, pct):
    """(v, T) of a group"""
    if cls == "tenths":
        return tenths(n), 0.2
    v = grid(n) if cls == "grid" else natural(kind, n)
    return v, threshold(v, above, pct, cls == "grid")


# ---- cumulativesum

CUMSUM_LENGTHS = (1, 2, 8191, 8192, 8193, 16385, 524287, 524288, 524289, 532481, 1000003)
SUPER_N = 33554432 + 8192 + 5


@functools.lru_cache(maxsize=None)
def cumsum_signal(kind):
    """1 000 003 bases; the shorter cases are its prefixes (so are their exact sums)"""
    n = CUMSUM_LENGTHS[-1]
    rng = np.random.default_rng(SEED + 17)
    if kind == "depth":
        v = depth(n)
    elif kind == "positive":
        v = depth(n) * rng.uniform(0.5, 1.5, n) + 16
    elif kind == "mixed":
        v = rng.standard_normal(n) * 5
        v = np.where(np.abs(v) < 1, np.copysign(1.0, v) + v, v)           # |v| >= 1
    elif kind == "smooth":
        v = natural("smooth", n)
    else:
        raise ValueError(kind)
    v = np.array(v)
    v.setflags(write=False)
    return v


def super_group(real):
    """one base more than a super-group of 4096 chunks plus a chunk plus 5: integer depth, or multiples of 2^-30 in [16, 48)"""
    if not real:
        return depth(SUPER_N)
    rng = np.random.default_rng(SEED + 33)
    return 16.0 + rng.integers(0, 32 << 30, SUPER_N).astype(np.float64) * 2.0 ** -30


# ---- slidingsum and sum on real values (test_hip_windowsum_real.py; the checker's own tests use prefixes of these)

WINDOW_SIGNALS = ("positive", "mixed", "smooth", "grid")
WINDOW_N = 300007                               # crosses cumulativesum's chunks (8192) and groups (524 288 / 64 chunks)
WINDOW_LONG_N = 130003                          # "about 130 000": more than 30 tiles of either tiled form

# gdsp_sliding_sum's routes (W <= 14332) and gdsp_sliding_sum_any's whole-vector route; every form's first and last
# window, both parities, and the block form's switch from blocks added one by one to a running sum over block totals
# (more than 8 whole blocks between: W >= 161)
SLIDING_WINDOWS = {"prefix-short": (3, 4, 16),
                   "blocks": (17, 18, 33, 100, 101, 160, 161, 1000, 2047, 2048),
                   "prefix-long": (2049, 4001, 8192, 8193, 14332),
                   "whole-vector": (14333, 20000, 65536, 400000)}          # 400 000: longer than every vector here
SLIDING_ODD_DENOMS = (4, 16, 100, 161, 2049, 14332, 14333, 65536)           # two per form: 3.0 and float(W) as well

SUM_WINDOWS = (8193, 9000, 50000)               # window_sum_wide_kernel


@functools.lru_cache(maxsize=None)
def window_signal(kind):
    """300 007 bases; the shorter cases are its prefixes.  grid: multiples of 2^-30 in [16, 48), as super_group(True)
    draws them -- no sum of 2^17 of them rounds (below 2^23 at quantum 2^-30)"""
    if kind == "grid":
        rng = np.random.default_rng(SEED + 34)
        v = 16.0 + rng.integers(0, 32 << 30, WINDOW_N).astype(np.float64) * 2.0 ** -30
    else:
        v = np.array(cumsum_signal(kind)[:WINDOW_N])
    v.setflags(write=False)
    return v


def sliding_route(W):
    return next(route for route, ws in SLIDING_WINDOWS.items() if W in ws)


def sliding_outs(W):
    """outputs per workgroup, as gdsp_sliding_sum lays the tiles out: the block form gives up (W-1)//16 + 1 of its 256
    blocks of 16 to the halo and 2 more outputs where the alignment shift is needed; the prefix form writes 4096"""
    if 17 <= W <= 2048:
        sh = ((W - 1) // 2) & 1
        return (256 - ((W - 1) // 16 + 1)) * 16 - 2 * sh
    return 4096


def sliding_lengths(W):
    if W > 14332:
        every = {1, W - 1, W, W + 1, WINDOW_LONG_N, WINDOW_N}
    else:
        outs = sliding_outs(W)
        every = {1, W - 1, W, W + 1, outs - 1, outs, outs + 1, 2 * outs + 3, 3 * outs + 5, WINDOW_LONG_N}
    return tuple(sorted(n for n in every if 1 <= n <= WINDOW_N))


def sliding_denoms(W):
    return (1.0, 0.25, 3.0, float(W)) if W in SLIDING_ODD_DENOMS else (1.0, 0.25)


def sum_lengths(W):
    return tuple(sorted({W - 1, W, W + 1, 3 * W + W // 3, 100003}))


def sum_params(W):
    """(denom, use_actual, zero)"""
    return ((1.0, False, 0.0), (float(W), False, 0.0), (1.0, True, -1.0))
