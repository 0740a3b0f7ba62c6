"""Exact checker for the operators that keep one running sum along the whole chromosome: clump / anticlump
(gdsp_clump.hip) and cumulativesum (gdsp_sums.hip).  CPU only: numpy and Python ints.

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


def _ceil_kA_over_den(A):
    """ceil(k A[k] / (2^53 - k)) for k = 0 .. n-1 in int64, exactly: k A[k] < 2^88 is held as hi 2^31 + lo and divided
    eight (seven) bits at a time, so that no intermediate reaches 2^63"""
    n = A.size
    assert n <= MAX_INT64_N and (n == 0 or (0 <= int(A[0]) and int(A[-1]) < (1 << 62)))
    k = np.arange(n, dtype=np.int64)
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
            rounds = int(np.searchsorted(self.A, min(_quantum(D) << U_BITS, 1 << 62), "right"))          # the first k with A[k] above it
            if slack and rounds < n:
                self.eps[rounds:] = _ceil_kA_over_den(self.A)[rounds:]
        else:
            assert self.backend == "int"
            D, self.E = _as_ints(d, unit)
            self.P = list(itertools.accumulate(D))
            self.A = list(itertools.accumulate(map(abs, D)))
            if slack:
                one, exact = 1 << U_BITS, _quantum(D) << U_BITS
                self.eps = [0 if a <= exact else -((-k * a) // (one - k)) for k, a in enumerate(self.A)]
            else:
                self.eps = [0] * n
        self._from = None

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


def runs(b):
    """number of separate runs of True"""
    b = np.asarray(b, bool)
    return int(b[0]) + int(np.count_nonzero(b[1:] & ~b[:-1])) if b.size else 0
