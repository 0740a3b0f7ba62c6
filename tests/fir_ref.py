"""What a zero-padded FIR with ARBITRARY taps must return (gdsp_fir_plan_create / gdsp_fir_apply, gdsp_fir.hip), stated
without the kernels and without the restated reference.  CPU only: numpy and Python ints.

    out[i] = sum over k = 0 .. W-1, ascending, of w[k] x[i-h+k],     h = (W-1)/2,     terms outside [0,n) skipped

fma_chain        the bits of GDSP_FIR_FMA: one correctly rounded w[k] x[j] + acc per tap from acc = +0.0.  Every finite
                 double is an integer over a power of two, so w[k] x[j] + acc is formed exactly in Python ints and
                 rounded once by CPython's int / int, which is correctly rounded (round-half-even, gradual underflow,
                 a negative result that underflows to nothing is -0.0, an exact zero is +0.0: all as IEEE 754's fma).
impulse_readout  the output for a signal of 1.0 at a few places and +0.0 elsewhere: the taps themselves, read backwards
                 around every impulse.  Exact in both modes, and a wrong, shifted, flipped or missing tap shows by index.
sample_positions where the kernels' paths change: the vector's ends, the half window, the seams of the 256 * 9 outputs
                 of one workgroup, and a few seeded positions in between.
taps             the families of taps the tests use, none of them a Hann window's (mirrored, positive, free of zeros).

The hann-window tests never tell a tap index running the wrong way from the right one; `noise`, `sparse` and `distinct`
taps do.
"""
import numpy as np

TILE = 2304                                     # outputs of one workgroup of the direct kernels: 256 threads * 9
STAGE = 1026                                    # taps per LDS stage of the run-time-W kernel
TAP_STEPS = 150_000                             # about what one case may spend in fma_chain


def _ratio(a):
    """finite doubles as (numerator, log2 of the denominator): a[i] = num / 2^k exactly"""
    out = []
    for v in a:
        num, den = float(v).as_integer_ratio()
        out.append((num, den.bit_length() - 1))
    return out


def fma_step(w, x, acc):
    """round_to_nearest (w * x + acc) with the product and the sum formed exactly"""
    (wn, wk), (xn, xk) = _ratio([w])[0], _ratio([x])[0]
    return _step(wn, wk, xn, xk, acc)


def _step(wn, wk, xn, xk, acc):
    an, ad = acc.as_integer_ratio()
    ak, pk = ad.bit_length() - 1, wk + xk
    if pk >= ak:
        return (wn * xn + (an << (pk - ak))) / (1 << pk)
    return (((wn * xn) << (ak - pk)) + an) / (1 << ak)


def fma_chain(x, w, positions):
    """out[i] for i in positions as one fused multiply-add per tap gives it: acc = +0.0, then for ascending k with
    0 <= i-h+k < n: acc = round_to_nearest (w[k] x[i-h+k] + acc).  Finite inputs only."""
    x = np.ascontiguousarray(x, np.float64)
    w = np.ascontiguousarray(w, np.float64)
    assert np.isfinite(x).all() and np.isfinite(w).all()
    assert w.size % 2 == 1
    n, W = x.size, w.size
    h = (W - 1) // 2
    wr = _ratio(w)
    xr = {}                                     # converted on first use: the positions touch a fraction of a long vector
    out = np.empty(len(positions), np.float64)
    for t, i in enumerate(positions):
        assert 0 <= i < n
        acc = 0.0
        for k in range(max(0, h - i), min(W, n + h - i)):
            j = i - h + k
            r = xr.get(j)
            if r is None:
                r = xr[j] = _ratio(x[j:j + 1])[0]
            acc = _step(wr[k][0], wr[k][1], r[0], r[1], acc)
        out[t] = acc
    return out


def impulse_readout(n, w, impulses):
    """(signal, expected output) for 1.0 at every p of impulses and +0.0 elsewhere: out[i] = w[p - i + h] where that
    index is a tap, +0.0 where no impulse is within the window.  Impulses at least W apart (no output sees two), taps
    finite and nonzero: then w * 1.0 is w and every other term is a zero that changes nothing, in either mode."""
    w = np.ascontiguousarray(w, np.float64)
    W = w.size
    h = (W - 1) // 2
    assert W % 2 == 1 and np.isfinite(w).all() and (w != 0).all()
    ps = sorted(int(p) for p in impulses)
    assert all(0 <= p < n for p in ps)
    assert all(b - a >= W for a, b in zip(ps, ps[1:]))
    x = np.zeros(n, np.float64)
    out = np.zeros(n, np.float64)
    for p in ps:
        x[p] = 1.0
        lo, hi = max(0, p - h), min(n, p + h + 1)
        i = np.arange(lo, hi)
        out[lo:hi] = w[p - i + h]
    return x, out


def spread(impulses, W):
    """the wanted impulse positions dealt into as few lists as keep every list's impulses W apart"""
    sets = []
    for p in sorted(set(int(p) for p in impulses)):
        for s in sets:
            if p - s[-1] >= W:
                s.append(p)
                break
        else:
            sets.append([p])
    return sets


def position_cap(W):
    """positions one case may hand to fma_chain: 64 up to three stages of taps, beyond that what TAP_STEPS allows to the
    nearest 16 (48 at W=3079, 32 at W=5001)"""
    if W <= 2 * STAGE + 1:
        return 64
    return max(16, min(64, (TAP_STEPS + 8 * W) // (16 * W) * 16))


def sample_positions(n, W, tile=TILE, seed=0, cap=None):
    """sorted positions in [0, n): the vector's ends and the half window's, three either side of every multiple of
    `tile`, about 20 seeded ones; at most `cap` (position_cap): the ends first, then both sides of every seam, a few
    seeded ones, the seams' wider surroundings, the remaining seeded ones"""
    h = (W - 1) // 2
    cap = position_cap(W) if cap is None else cap
    rng = np.random.default_rng(seed * 1_000_003 + n * 7 + W)
    rand = [int(p) for p in rng.integers(0, n, size=20)] if n > 0 else []
    seams = list(range(tile, n + 3, tile))
    want = [0, 1, h - 1, h, h + 1, n - h - 1, n - h, n - 1]
    want += [m + off for off in (-1, 0) for m in seams] + rand[:4]
    want += [m + off for off in (-2, 1, -3, 2) for m in seams] + rand[4:]
    got = []
    for p in want:
        if (0 <= p < n) and (p not in got) and (len(got) < cap):
            got.append(p)
    return sorted(got)


TAP_KINDS = ("noise", "dyadic", "sparse", "mirrored", "distinct")


def taps(kind, W, seed=0):
    """W taps of one family:
    noise     standard normal: asymmetric, both signs
    dyadic    (-1)^k (k % 61 + 1) 2^-10: against integers below 2^30 no product and no sum rounds at any W used here, so
              exact mode, fused mode and any order of summation give the same bits
    sparse    zeros, every third of them -0.0, but for the first, the last and the middle tap and, beyond one LDS stage
              of the run-time kernel, taps 1025, 1026, 1027 and the last and first tap of every stage
    mirrored  noise with w[W-1-k] = w[k] copied: the same doubles, as in a Hann window
    distinct  (-1)^k (k + 1) / 8: no two alike, none zero: impulse_readout names the tap it finds"""
    assert W % 2 == 1 and W >= 1
    rng = np.random.default_rng([seed, W, TAP_KINDS.index(kind)])
    k = np.arange(W)
    sign = np.where(k % 2 == 0, 1.0, -1.0)
    if kind == "noise":
        return rng.standard_normal(W)
    if kind == "dyadic":
        return sign * (k % 61 + 1) * 2.0 ** -10
    if kind == "distinct":
        return sign * (k + 1) / 8.0
    if kind == "mirrored":
        w = rng.standard_normal(W)
        w[W - 1 - k[:W // 2]] = w[:W // 2]
        return w
    if kind == "sparse":
        w = np.where(k % 3 == 1, -0.0, 0.0)
        keep = {0, W - 1, (W - 1) // 2}
        if W > STAGE:
            keep |= {1025, 1026, 1027}
            keep |= {s - 1 for s in range(STAGE, W, STAGE)} | {s for s in range(STAGE, W, STAGE)}
        keep = np.array(sorted(p for p in keep if p < W))
        v = rng.standard_normal(keep.size)
        v[v == 0] = 1.0
        w[keep] = v
        return w
    raise ValueError(kind)
