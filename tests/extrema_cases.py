"""Inputs and checkers for localmax/localmin/bestmax/bestmin on NaN, infinities, signed zeros, the largest and the
smallest doubles and plateaus (test_extrema_cases.py on the CPU, test_hip_extrema_special.py on the GPU): fixed
seeds, nothing here touches a GPU.

What the reference (oracle.cpu, restating minmax.c) pins, window by window -- test_extrema_cases.py holds the oracle
itself to this table, so it is the reference's and not ours:

  localmax/localmin, any input     out = (E > v) ? fill : v  (E < v for localmin), E the extreme of the window's
                                   numbers: bit for bit at every base
  bestmax/bestmin
    clean  no NaN in the window    the window's extreme, bit for bit ...
    zero   ... unless that is a zero and the window holds zeros of both signs: some zero, the sign depends on the
           reference's scan history
    all_nan  every base NaN        NaN (sign and payload not pinned)
    mixed  NaN and numbers         the numbers' extreme or NaN, depending on scan history
"""
import numpy as np

from oracle import cpu

DBL_MAX = cpu.DBL_MAX
MIN_NORMAL = 2.2250738585072014e-308
DENORM = 5e-324
BIG_W = 4096                                       # above it the NaN case is cut down so that the oracle stays fast

# the windows of the GPU test, by the route each takes through the kernels
WINDOWS_DIRECT = (2, 3, 4)
WINDOWS_BLOCKS = (5, 8, 9, 16, 17, 33, 101, 1001, 3584)
WINDOWS_SEGMENTS = (3585, 8190)
WINDOWS_LONG = (9001, 20000)
WINDOWS = WINDOWS_DIRECT + WINDOWS_BLOCKS + WINDOWS_SEGMENTS + WINDOWS_LONG

_NANS = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000123], np.uint64).view(np.float64)


def _noise(rng, n):
    return rng.standard_normal(n) * 5


def _nan_run(rng, n):
    """NaNs of both signs and one with a payload: a kernel that rebuilds its NaN shows against the localmax rule,
    which hands the centre back bit for bit"""
    return _NANS[rng.integers(0, 3, n)] if n > 3 else _NANS[:n].copy()


def nan_runs(W, rng, lead=0):
    """runs of 1, 2, W-1, W, W+1 and 2W+3 NaNs between 4W+5 bases of noise, six NaNs at either end of the vector;
    `lead` bases of noise in front.  Returns the vector and the start of the first run that is not at an end.
    A run shorter than W makes mixed windows only, one of W bases exactly one all-NaN window, longer ones a stretch
    of them; the gaps are long enough for windows without NaN between any two runs."""
    runs = (1, W + 1) if W > BIG_W else (1, 2, W - 1, W, W + 1, 2 * W + 3)
    gap = 2 * W + 5 if W > BIG_W else 4 * W + 5
    parts, first, at = [_noise(rng, lead), _nan_run(rng, 6)], None, lead + 6
    for r in runs:
        parts.append(_noise(rng, gap))
        at += gap
        first = at if first is None else first
        parts.append(_nan_run(rng, r))
        at += r
    parts += [_noise(rng, gap), _nan_run(rng, 6)]
    return np.concatenate(parts), first


def infinities(W, rng):
    """scattered +-inf; a run of -inf longer than W, where bestmax must answer -inf (the very value a kernel's
    "nothing seen yet" would leak), and a run of +inf longer than W for bestmin"""
    n = 6 * W + 40
    x = _noise(rng, n)
    step = W // 2 + 7
    x[3::2 * step] = np.inf
    x[3 + step::2 * step] = -np.inf
    x[W + 11:2 * W + 14] = -np.inf
    x[4 * W + 20:5 * W + 23] = np.inf
    return x


def magnitudes(W, rng):
    """+-DBL_MAX and its neighbour, +-5e-324, +-2.2250738585072014e-308 and other subnormals side by side, in
    stretches longer than W drawn from one palette each: a comparison in lower precision ties DBL_MAX with its
    neighbour, one with subnormals flushed ties every tiny value with zero"""
    below = np.nextafter(DBL_MAX, 0.0)
    palettes = (
        [DENORM, -DENORM, 1e-320, MIN_NORMAL, -MIN_NORMAL, 1e-310],
        [-DENORM, -1e-323, -MIN_NORMAL, -3e-308],
        [DENORM, 1e-323, MIN_NORMAL, 3e-308],
        [DBL_MAX, below, -DBL_MAX, -below, 1e308],
        [DBL_MAX, -DBL_MAX, DENORM, -DENORM, MIN_NORMAL, -MIN_NORMAL, 1.0, -1.0],
    )
    return np.concatenate([np.array(p)[rng.integers(0, len(p), W + 5)] for p in palettes])


def signed_zeros(W, rng):
    """zeros of one sign and of both among negative values (the zero is the maximum) and among positive values (the
    minimum), then a plateau of -0.0 with one +0.0 at either end, among both as well.  Where one sign only is in the
    window the reference hands back that very zero, so a pick that returns +0.0 for two -0.0 shows."""
    m = (W + 7) if W > BIG_W else (2 * W + 7)
    parts = []
    for sign in (-1.0, 1.0):                       # the values around the zeros
        for kind in ("minus", "plus", "both"):
            s = sign * (np.abs(_noise(rng, m)) + 0.5)
            z = rng.random(m) < (0.02 if W > BIG_W else 0.3)       # (every tie costs the oracle a rescan of W bases)
            zeros = {"minus": np.full(m, -0.0), "plus": np.zeros(m),
                     "both": np.where(rng.random(m) < 0.5, -0.0, 0.0)}[kind]
            parts.append(np.where(z, zeros, s))
        plateau = np.full(W // 8 + 4 if W > BIG_W else W + 4, -0.0)
        plateau[0] = plateau[-1] = 0.0
        parts += [sign * (np.abs(_noise(rng, W + 3)) + 0.5), plateau, sign * (np.abs(_noise(rng, W + 3)) + 0.5)]
    return np.concatenate(parts)


def plateaus(W, rng):
    """equal non-zero values, longer than W (windows that see nothing else) and shorter, above the noise and below
    it; a long one at the first base and a short one at the last (plateaus_rev: the other way round)"""
    long_, short = W + 3, max(1, W // 2)
    gap = W // 2 + 5 if W > BIG_W else 2 * W + 5
    return np.concatenate([np.full(long_, 20.0), _noise(rng, gap), np.full(short, -20.0), _noise(rng, gap),
                           np.full(long_, -20.0), _noise(rng, gap), np.full(short, 20.0)])


def special_cases(W, rng):
    """name -> vector for a window of W bases"""
    p = plateaus(W, rng)
    return {
        "nan_runs": nan_runs(W, rng)[0],
        "infinities": infinities(W, rng),
        "magnitudes": magnitudes(W, rng),
        "signed_zeros": signed_zeros(W, rng),
        "plateaus": p,
        "plateaus_rev": p[::-1].copy(),
    }


CASES = ("nan_runs", "infinities", "magnitudes", "signed_zeros", "plateaus", "plateaus_rev")
NAN_CASES = ("nan_runs",)
NO_NAN_NO_MINUS_ZERO = ("infinities", "magnitudes")


# --------------------------------------------------------------------------------------------- classifier ----

def _window_counts(flag, lft, rgt):
    """how many bases of the clamped window [i-lft, i+rgt] have the flag, from prefix counts"""
    n = flag.size
    c = np.concatenate([[0], np.cumsum(flag, dtype=np.int64)])
    i = np.arange(n, dtype=np.int64)
    return c[np.minimum(i + rgt, n - 1) + 1] - c[np.maximum(i - lft, 0)]


class Classes:
    """the table's classes for every base's window; `extreme`, `zero` and `bits` are indexed by want_max (0/1)"""

    def __init__(self, x, W):
        x = np.ascontiguousarray(x, np.float64)
        n = x.size
        lft = (W - 1) // 2
        rgt = W - 1 - lft
        i = np.arange(n, dtype=np.int64)
        size = np.minimum(i + rgt, n - 1) - np.maximum(i - lft, 0) + 1
        nan = np.isnan(x)
        nans = _window_counts(nan, lft, rgt)
        self.all_nan = nans == size
        self.mixed = (nans > 0) & ~self.all_nan
        self.clean = nans == 0
        both = (_window_counts((x == 0) & np.signbit(x), lft, rgt) > 0) & \
               (_window_counts((x == 0) & ~np.signbit(x), lft, rgt) > 0)
        self.extreme, self.zero, self.bits = [None, None], [None, None], [None, None]
        for want_max in (0, 1):
            # the numbers' extreme: NaN stands back behind everything, as outside the vector does
            e = cpu.best_extrema(np.where(nan, -np.inf if want_max else np.inf, x), W, want_max)
            self.extreme[want_max] = e
            self.zero[want_max] = self.clean & both & (e == 0)
            self.bits[want_max] = self.clean & ~self.zero[want_max]


def classify(x, W):
    return Classes(x, W)


def _first(bad, names):
    """(first offending index, its class) or None"""
    idx = np.flatnonzero(bad)
    if idx.size == 0:
        return None
    i = int(idx[0])
    return i, next(name for name, mask in names if mask[i])


def check_best(got, x, W, want_max, cls=None):
    """bestmax/bestmin output against the table; None, or the first offending index and its class"""
    cls = cls if cls is not None else classify(x, W)
    m = 1 if want_max else 0
    got = np.ascontiguousarray(got, np.float64)
    if got.shape != cls.all_nan.shape:
        return -1, "shape"
    e = cls.extreme[m]
    bad = np.zeros(got.size, bool)
    bad |= cls.bits[m] & (got.view(np.uint64) != e.view(np.uint64))
    bad |= cls.zero[m] & ~(got == 0.0)
    bad |= cls.all_nan & ~np.isnan(got)
    bad |= cls.mixed & ~(np.isnan(got) | (got == e))
    return _first(bad, (("clean", cls.bits[m]), ("zero", cls.zero[m]), ("all_nan", cls.all_nan), ("mixed", cls.mixed)))


def local_rule(x, N, want_max, fill, cls=None):
    """(expected output, mask of the bases that take the fill) by the window-local rule"""
    h = (N - 1) // 2
    cls = cls if cls is not None else classify(x, 2 * h + 1)
    e = cls.extreme[1 if want_max else 0]
    with np.errstate(invalid="ignore"):
        out_ = (e > x) if want_max else (e < x)
    return np.where(out_, fill, x), out_


def check_local(got, x, N, want_max, fill, cls=None):
    """localmax/localmin output against the rule, bit for bit (a NaN fill as NaN); None, or the first offending
    index and its class: "kept" where the rule keeps the centre, "filled" where it writes the fill"""
    x = np.ascontiguousarray(x, np.float64)
    got = np.ascontiguousarray(got, np.float64)
    if got.shape != x.shape:
        return -1, "shape"
    want, filled = local_rule(x, N, want_max, fill, cls)
    bad = got.view(np.uint64) != want.view(np.uint64)
    if np.isnan(fill):
        bad = np.where(filled, ~np.isnan(got), bad)
    return _first(bad, (("filled", filled), ("kept", ~filled)))


def literal_classes(x, W, want_max):
    """the window rule as a literal O(n W) loop: per base (class, extreme of the window's numbers or None)"""
    n = len(x)
    lft = (W - 1) // 2
    rgt = W - 1 - lft
    out = []
    for i in range(n):
        win = [float(v) for v in x[max(0, i - lft):min(n - 1, i + rgt) + 1]]
        nums = [v for v in win if v == v]
        ext = (max(nums) if want_max else min(nums)) if nums else None
        if not nums:
            kind = "all_nan"
        elif len(nums) < len(win):
            kind = "mixed"
        elif ext == 0 and len({np.signbit(v) for v in nums if v == 0}) == 2:
            kind = "zero"
        else:
            kind = "clean"
        out.append((kind, ext))
    return out
