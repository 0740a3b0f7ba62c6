"""Exact checker for the operators that keep one running sum along the whole chromosome: clump / anticlump
(gdsp_clump.hip) and cumulativesum (gdsp_sums.hip), and for the window sums formed from such sums: slidingsum and `sum`
over windows beyond 8192 bases (gdsp_sums.hip, gdsp_longwin.hip).  CPU only: numpy and Python ints.

Like xsum_ref.py it rests on every finite double being an integer times a power of two, so the prefix sums

    P[k] = sum of d[0..k]  (P[-1] = 0),      A[k] = sum of |d[0..k]|

are computed without any rounding.  d is the operator's term: v for cumulativesum, fl(v - T) for clump and fl(T - v)
for anticlump -- that one rounding is part of the operator's definition and the same in every implementation.

What a correct implementation may return is then stated without reference to any particular order of summation.  A
floating-point sum of d[0..k] in ANY order or tree (the reference's left-to-right accumulator, a chunk-relative prefix
plus the chunk's offset, whatever comes later) differs from P[k] by at most

    eps[k] = gamma_k A[k],   gamma_k = k u / (1 - k u),   u = 2^-53                        (Higham, ASNA 2nd ed., 4.4)

and by nothing at all while every partial sum is exactly representable: when the terms d[0..k] are multiples of a
common power of two q and A[k] <= 2^53 q, every sum of a subset of them is an integer multiple of q below 2^53 q in
magnitude and no addition rounds, so eps[k] = 0 there (read depth against a dyadic threshold).  eps never decreases.

clump.  Base t is marked <=> there are j < t <= i with i - j >= L and P[j] <= P[i] (j >= -1); with from(i) = the
earliest j >= -1 with P[j] <= P[i], that is: mark (from(i), i] for every i with i - from(i) >= L.  Every maximal run of
marked bases is then trimmed to its first and last base on the threshold's side.  With computed prefixes P~,
|P~ - P| <= eps:    P~[j] <= P~[i]  =>  P[j] <= P[i] + 2 eps[i],     P[j] <= P[i] - 2 eps[i]  =>  P~[j] <= P~[i]    (j < i)
and both marking and trimming are monotone in the set of admitted pairs, so the output under the second test
("strict") is contained in every correct output, which is contained in the output under the first ("lenient").

Window sums.  slidingsum's window at base c is [lo, hi] = [max(0, c-lft), min(n-1, c+rgt)], rgt = (W-1)//2,
lft = W-1-rgt (sum.c:436-455; an even W reaches one base further to the left); `sum`'s windows are [s, min(s+W, n)-1]
for s = 0, W, 2W, ... (the last one ragged), the result goes to base s and the zero value to the window's other bases
(sum.c:230-249).  In both S = P[hi] - P[lo-1] is formed in integers, and what a correct evaluation may return is
|x~ - S| <= E with E stated per route, again without reference to one order of summation:

  tiled slidingsum (W <= TILED_MAX_W = 14332: the prefix form and the block form of gdsp_sliding_sum).  A workgroup
    stages the windows of its outputs and sums inside what it staged: at most TILE = 4096 bases beyond the window on
    either side.  It may associate those terms in any way (a running sum from the tile's first base, block totals, a
    running sum over block totals) and may form the window as the difference of two such partial sums.  Each partial
    sum has at most W + TILE terms out of the span Z = [c-lft-TILE, c+rgt+TILE] (clipped to the vector), so it is off
    by at most gamma_(W+TILE-1) A(Z); the difference adds the two errors and one rounding of its own, u (|S| + both
    errors) <= u (1 + 2 gamma) A(Z); and the exact value this checker returns is itself rounded once, u |S| <= u A(Z).
    In all fewer than 2 (W + TILE) + 4 factors (1 + delta), |delta| <= u, per term:
        E[c] = gamma_m A(Z),    m = 2 (W + TILE) + 4
    and E[c] = 0 where A(Z) <= 2^53 q: then no sum of any of the span's terms rounds and the result is S, bit for bit.
  whole-vector slidingsum (W > TILED_MAX_W: gdsp_sliding_sum_any copies the vector, runs cumulativesum over the copy
    and subtracts two of its values).  E[c] = eps[hi] + eps[lo-1], eps exactly what cumsum_exact grants each prefix
    (eps[-1] = 0: nothing is subtracted there).  This is a little stronger than "any order": it leaves the
    subtraction's own rounding, u |S|, no room of its own.  Where something is subtracted (lo >= 1) hi >= W-1 >= 14332,
    so that rounding is at most 1/14332 of eps[hi], which a prefix of that length only uses up if it is one chain of
    hi additions whose every rounding goes the same way; cumulativesum's chunked look-back is far from that.
  `sum`.  One window of len = hi-lo+1 terms in any order or tree: len-1 additions, and one more factor for the
    rounding of the checker's own exact value:  E = gamma_len A(window), 0 where A(window) <= 2^53 q.

The quotient.  got = fl(x~ / denom), so |got - S/denom| <= (E + u (|S| + E)) / |denom|: that, rounded up, is `allow`.
Dividing by a power of two does not round and the u term is dropped.  `exact` is S / denom rounded once (to nearest,
from the integers: never the quotient of an already rounded S).

Two back ends, same results where both apply:
  "int"    Python ints, any finite doubles; a few microseconds per base
  "int64"  numpy int64 for values (and threshold) that are multiples of 2^-30 with sum |d| 2^30 < 2^62; a second or
           so at 5 000 000 bases
"""
import bisect
import itertools

import numpy as np

U_BITS = 53
GRID_BITS = 30                                  # the int64 back end's quantum is 2^-30
TILE = 4096                                     # gdsp_sliding_sum's `tile` (prefix form) and SLB_ELEMS (block form): no
                                                # workgroup stages, or sums, more than this beyond a window on either side
TILED_MAX_W = 14332                             # gdsp_sliding_sum: 18432 doubles of LDS - tile - 4; longer windows go
                                                # through gdsp_sliding_sum_any's whole-vector route
MAX_INT64_N = 1 << 26                           # k A[k] is formed in two limbs that assume k < 2^26


# ---------------------------------------------------------------------------------------------- exact prefix sums ----

def _terms(v, T, above):
    v = np.ascontiguousarray(v, np.float64)
    assert np.isfinite(v).all()
    if T is None:
        return v
    return v - np.float64(T) if above else np.float64(T) - v


def on_grid(v, T=None):
    """every value (and the threshold) is a multiple of 2^-30 below 2^22 in magnitude"""
    x = np.ldexp(np.asarray(v, np.float64), GRID_BITS)
    ok = bool(np.all(x == np.rint(x)) and np.all(np.abs(x) < 2.0 ** 52))
    if ok and T is not None:
        t = float(T) * 2.0 ** GRID_BITS
        ok = t == round(t) and abs(t) < 2.0 ** 52
    return ok


def _as_ints(d, E=None):
    """finite doubles as Python ints times 2^E: (list, E).  E: the lowest exponent among the terms unless given (then
    every term must be a multiple of 2^E)"""
    m, e = np.frexp(d)
    mi = np.ldexp(m, U_BITS).astype(np.int64)              # exact: |mi| < 2^53
    ex = e.astype(np.int64) - U_BITS
    nz = mi != 0
    tz = np.frexp((mi & -mi).astype(np.float64))[1].astype(np.int64) - 1        # trailing zeros (a power of two: exact)
    mi, ex = mi >> np.where(nz, tz, 0), ex + np.where(nz, tz, 0)
    lowest = int(ex[nz].min()) if nz.any() else 0
    if E is None:
        E = lowest
    assert E <= lowest or not nz.any()
    sh = np.where(nz, ex - E, 0)
    return [a << s for a, s in zip(mi.tolist(), sh.tolist())], E


def _quantum(D):
    """the largest power of two that divides every term (in the terms' unit; 1 if all are zero)"""
    if isinstance(D, np.ndarray):
        bits = int(np.bitwise_or.reduce(np.abs(D))) if D.size else 0
    else:
        bits = 0
        for x in D:
            bits |= abs(x)
    return (bits & -bits) or 1


def _ceil_kA_over_den(A, k=None):
    """ceil(k A[k] / (2^53 - k)) for k = 0 .. n-1 (or the k given: one number or one per entry, below 2^26) in int64,
    exactly: k A[k] < 2^88 is held as hi 2^31 + lo and divided eight (seven) bits at a time, so that no intermediate
    reaches 2^63"""
    n = A.size
    if k is None:
        assert n <= MAX_INT64_N and (n == 0 or (0 <= int(A[0]) and int(A[-1]) < (1 << 62)))
        k = np.arange(n, dtype=np.int64)
    else:
        k = np.broadcast_to(np.asarray(k, np.int64), A.shape)
        assert n == 0 or (0 <= int(k.min()) and int(k.max()) <= MAX_INT64_N and 0 <= int(A.min()) and int(A.max()) < (1 << 62))
    den = (np.int64(1) << U_BITS) - k
    low = k * (A & ((1 << 31) - 1))                         # < 2^57
    hi = k * (A >> 31) + (low >> 31)                        # < 2^58
    lo = low & ((1 << 31) - 1)
    q, r = np.divmod(hi, den)                               # r < 2^53
    shift = 31
    for bits in (8, 8, 8, 7):
        shift -= bits
        r = (r << bits) | ((lo >> shift) & ((1 << bits) - 1))          # < 2^61
        step, r = np.divmod(r, den)
        q = (q << bits) + step
    return q + (r > 0)


class Prefix:
    """P, A and eps of the terms d, in units of 2^E (Python ints in lists, or int64 arrays).  slack=False forces eps to
    0 (the literal definition, for the checker's own tests)."""

    def __init__(self, d, backend=None, slack=True, unit=None):
        d = np.ascontiguousarray(d, np.float64)
        assert np.isfinite(d).all()
        self.n = n = int(d.size)
        self.backend = backend or ("int64" if on_grid(d) and n <= MAX_INT64_N else "int")
        if self.backend == "int64":
            assert on_grid(d), "int64 back end: a term is no multiple of 2^-30"
            assert float(np.abs(d).sum()) * 2.0 ** GRID_BITS < 2.0 ** 62 * (1 - 2.0 ** -20), "int64 back end: sum |d| 2^30 >= 2^62"
            self.E = -GRID_BITS
            D = np.ldexp(d, GRID_BITS).astype(np.int64)
            self.P = np.cumsum(D)
            self.A = np.cumsum(np.abs(D))
            assert n == 0 or int(self.A[-1]) < (1 << 62)
            self.eps = np.zeros(n, np.int64)
            self.exact_below = min(_quantum(D) << U_BITS, 1 << 62)            # 2^53 q: no sum with A up to here rounds
            rounds = int(np.searchsorted(self.A, self.exact_below, "right"))                            # the first k with A[k] above it
            if slack and rounds < n:
                self.eps[rounds:] = _ceil_kA_over_den(self.A)[rounds:]
        else:
            assert self.backend == "int"
            D, self.E = _as_ints(d, unit)
            self.P = list(itertools.accumulate(D))
            self.A = list(itertools.accumulate(map(abs, D)))
            self.exact_below = _quantum(D) << U_BITS
            if slack:
                one, exact = 1 << U_BITS, self.exact_below
                self.eps = [0 if a <= exact else -((-k * a) // (one - k)) for k, a in enumerate(self.A)]
            else:
                self.eps = [0] * n
        self._from = None
        self._padded = None

    # -- as doubles
    def _to_float(self, ints, up):
        x = np.array(ints, dtype=np.float64) if self.n else np.zeros(0)          # int -> double: rounded once, to nearest
        if up:
            x = np.where(x > 0, np.nextafter(x, np.inf), x)                      # never below the integer
        return np.ldexp(x, self.E)

    def exact(self):
        """P rounded once"""
        return self._to_float(self.P, False)

    def eps_float(self):
        """eps, rounded up"""
        return self._to_float(self.eps, True)

    # -- window sums
    def padded(self):
        """(P, A, eps) as arrays with a 0 in front: entry k+1 belongs to base k, entry 0 to "before the vector" (int64,
        or Python ints in object arrays)"""
        if self._padded is None:
            dt = np.int64 if self.backend == "int64" else object
            self._padded = tuple(np.concatenate((np.zeros(1, dt), np.array(x, dtype=dt))) if self.n else np.zeros(1, dt)
                                 for x in (self.P, self.A, self.eps))
        return self._padded

    def gamma_times(self, m, A):
        """ceil(gamma_m A) = ceil(m A / (2^53 - m)) where A is above 2^53 q, 0 where no sum of such terms can round"""
        if self.backend == "int64":
            g = _ceil_kA_over_den(A, m)
        else:
            m = np.broadcast_to(np.asarray(m), A.shape).astype(object)          # (Python ints: an int64 times a long int is a float)
            g = -((-m * A) // ((1 << U_BITS) - m))
        return np.where(A <= self.exact_below, 0, g) if A.size else A

    def quotient(self, S, E, den):
        """(S / den rounded once, (E + u (|S| + E)) / |den| rounded up; the u term only where den is no power of two);
        den: one double or one per entry"""
        n = S.size
        den = np.broadcast_to(np.asarray(den, np.float64), S.shape)
        assert np.all(np.isfinite(den)) and np.all(den != 0.0)
        m, e = np.frexp(den)
        pow2 = np.abs(m) == 0.5
        exact = self._to_float(S, False) / den if n else np.zeros(0)            # a power of two: scaled, not rounded again
        allow = self._to_float(E, True)
        if not pow2.all():
            D = np.ldexp(m, U_BITS).astype(np.int64).tolist()                    # den = D 2^(e-53), exactly
            ints, rest = S.tolist(), np.flatnonzero(~pow2)
            q = np.array([ints[i] / D[i] for i in rest.tolist()], np.float64)    # int / int: rounded once, to nearest
            exact[rest] = np.ldexp(q, self.E - (e[rest].astype(np.int64) - U_BITS))
            absS = np.abs(S) if self.backend == "int64" else np.array([abs(x) for x in ints], dtype=object)
            up = lambda x: np.where(x > 0, np.nextafter(x, np.inf), x)
            allow = np.where(pow2, allow, up(allow + np.ldexp(self._to_float(absS + E, True), -U_BITS)))
        allow = allow / np.abs(den)
        return exact, np.where(allow > 0, np.nextafter(allow, np.inf), allow)

    # -- clump
    def froms(self):
        """(strict, lenient): per i the earliest j >= -1 with P[j] <= P[i] -+ 2 eps[i]; n where there is none"""
        if self._from is None:
            if self.backend == "int64":
                negQ = -np.minimum.accumulate(np.concatenate((np.zeros(1, np.int64), self.P)))     # never decreases
                self._from = (np.searchsorted(negQ, 2 * self.eps - self.P, "left").astype(np.int64) - 1,
                              np.searchsorted(negQ, -2 * self.eps - self.P, "left").astype(np.int64) - 1)
            else:
                negQ = [-q for q in itertools.accumulate([0] + self.P, min)]
                self._from = (np.array([bisect.bisect_left(negQ, 2 * e - p) - 1 for p, e in zip(self.P, self.eps)], np.int64),
                              np.array([bisect.bisect_left(negQ, -2 * e - p) - 1 for p, e in zip(self.P, self.eps)], np.int64))
        return self._from


def _mark(frm, L):
    """the union of (frm[i], i] over the i with i - frm[i] >= L"""
    n = frm.size
    i = np.arange(n, dtype=np.int64)
    sel = (i - frm) >= L
    diff = np.bincount(frm[sel] + 1, minlength=n + 1) - np.bincount(i[sel] + 1, minlength=n + 1)
    return np.cumsum(diff[:n]) > 0


def _trim(marked, onside):
    """every maximal run of marked bases cut back to its first and last on-side base (nothing left if it has none)"""
    n = marked.size
    idx = np.arange(n, dtype=np.int64)
    hit = marked & onside
    last_hit = np.maximum.accumulate(np.where(hit, idx, -1))
    last_gap = np.maximum.accumulate(np.where(marked, -1, idx))
    next_hit = np.minimum.accumulate(np.where(hit, idx, n)[::-1])[::-1]
    next_gap = np.minimum.accumulate(np.where(marked, n, idx)[::-1])[::-1]
    return marked & (last_hit > last_gap) & (next_hit < next_gap)


class Clump:
    """everything about one (v, T, direction) that does not depend on L"""

    def __init__(self, v, T, above=True, backend=None, slack=True, unit=None):
        v = np.ascontiguousarray(v, np.float64)
        if backend == "int64":
            assert on_grid(v, T), "int64 back end: a value or the threshold is no multiple of 2^-30"
        elif backend is None:
            backend = "int64" if on_grid(v, T) and v.size <= MAX_INT64_N else "int"
        self.prefix = Prefix(_terms(v, T, above), backend, slack, unit)
        self.onside = (v >= T) if above else (v <= T)

    def bounds(self, L):
        """(strict, lenient) as boolean arrays"""
        assert L >= 1
        strict, lenient = self.prefix.froms()
        return _trim(_mark(strict, L), self.onside), _trim(_mark(lenient, L), self.onside)


def clump_bounds(v, T, L, above=True, backend=None, slack=True, unit=None):
    return Clump(v, T, above, backend, slack, unit).bounds(L)


def cumsum_exact(v, backend=None, unit=None):
    """(the exact prefix sums rounded once, eps rounded up), per position"""
    p = Prefix(_terms(v, None, True), backend, True, unit)
    return p.exact(), p.eps_float()


class Sliding:
    """slidingsum of one vector at one W: S and E per base in the prefix's unit, whatever the denominator"""

    def __init__(self, prefix, W):
        assert W >= 1
        self.prefix, self.W, n = prefix, W, prefix.n
        self.tiled = W <= TILED_MAX_W
        rgt = (W - 1) // 2
        lft = W - 1 - rgt
        c = np.arange(n, dtype=np.int64)
        self.lo, self.hi = np.maximum(c - lft, 0), np.minimum(c + rgt, n - 1)
        P, A, eps = prefix.padded()
        self.S = P[self.hi + 1] - P[self.lo]
        if self.tiled:
            a, b = np.maximum(c - lft - TILE, 0), np.minimum(c + rgt + TILE, n - 1)
            self.E = prefix.gamma_times(2 * (W + TILE) + 4, A[b + 1] - A[a])
        else:
            self.E = eps[self.hi + 1] + eps[self.lo]

    def over(self, denom):
        """(exact, allow) per base"""
        return self.prefix.quotient(self.S, self.E, float(denom))


def sliding_exact(v, W, denom=1.0, backend=None):
    """slidingsum: (the exact window sums over denom rounded once, what a correct result may differ by), per base.
    v: the values, or their Prefix"""
    p = v if isinstance(v, Prefix) else Prefix(_terms(v, None, True), backend)
    return Sliding(p, W).over(denom)


def window_exact(v, W, denom=1.0, use_actual=False, zero=0.0, backend=None):
    """`sum`: (exact, allow, is_sum) per base: at a window's first base the exact sum over denom (over the window's own
    length with use_actual) rounded once and its allowance; `zero` and 0 at every other base"""
    assert W >= 1
    p = v if isinstance(v, Prefix) else Prefix(_terms(v, None, True), backend)
    n = p.n
    s = np.arange(0, n, W, dtype=np.int64)
    e = np.minimum(s + W, n)
    P, A, _ = p.padded()
    E = p.gamma_times(e - s, A[e] - A[s])
    q, a = p.quotient(P[e] - P[s], E, (e - s).astype(np.float64) if use_actual else float(denom))
    exact, allow, is_sum = np.full(n, float(zero)), np.zeros(n), np.zeros(n, bool)
    exact[s], allow[s], is_sum[s] = q, a, True
    return exact, allow, is_sum


def runs(b):
    """number of separate runs of True"""
    b = np.asarray(b, bool)
    return int(b[0]) + int(np.count_nonzero(b[1:] & ~b[:-1])) if b.size else 0
