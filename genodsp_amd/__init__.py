"""genodsp_amd -- MI355X-native genomic-signal DSP (genodsp-compatible hot path).

This package is the thin Python face of the C ABI in include/genodsp_hip.h
(genodsp_amd/libgenodsp_hip.so: hand-written HIP kernels for gfx950).  It exists
for tests and bench.py; the drop-in product is the C library plus the C host
driver under genodsp_amd/host/.  There is no CPU fallback anywhere in here.

    import genodsp_amd as gd
    v = gd.DeviceVector.from_numpy(x)        # f64 chromosome vector in HBM
    out = gd.smooth(v, 101)                  # op_smooth_apply, sum.c:616-676
    out.numpy()
"""
import ctypes as C

import numpy as np

from ._lib import GdspError, SIGNATURES, SO_PATH, build, call, lib

FIR_EXACT, FIR_FMA, FIR_HANN = 0, 1, 2
OVERLAP_SUM, OVERLAP_MIN, OVERLAP_MAX = 0, 1, 2
DBL_MAX = float(np.finfo(np.float64).max)
DBL_MIN = float(np.finfo(np.float64).tiny)


def device_count():
    n = C.c_int(0)
    call("gdsp_device_count", C.byref(n))
    return n.value


def current_device():
    d = C.c_int(0)
    call("gdsp_get_device", C.byref(d))
    return d.value


def set_device(i):
    call("gdsp_set_device", int(i))


def _sp(stream):
    return C.c_void_p(stream) if stream else None


class Stream:
    def __init__(self):
        h = C.c_void_p()
        call("gdsp_stream_create", C.byref(h))
        self.handle = h.value

    def sync(self):
        call("gdsp_stream_sync", C.c_void_p(self.handle))

    def wait_event(self, event):
        """what is queued on this stream from now on starts after `event`"""
        call("gdsp_stream_wait_event", C.c_void_p(self.handle), C.c_void_p(event.handle))

    def close(self):
        if self.handle:
            call("gdsp_stream_destroy", C.c_void_p(self.handle))
            self.handle = None


def sync(stream=None):
    """Wait for `stream`; with no stream, for EVERY stream of the current device (the library's streams are
    non-blocking, so the NULL stream alone would not order a copy behind a kernel launched on one of them)."""
    if stream:
        call("gdsp_stream_sync", _sp(stream))
    else:
        call("gdsp_device_sync")


class Event:
    def __init__(self):
        h = C.c_void_p()
        call("gdsp_event_create", C.byref(h))
        self.handle = h.value

    def record(self, stream=None):
        call("gdsp_event_record", C.c_void_p(self.handle), _sp(stream))

    def elapsed_ms(self, later):
        ms = C.c_float()
        call("gdsp_event_elapsed_ms", C.c_void_p(self.handle), C.c_void_p(later.handle), C.byref(ms))
        return ms.value


class DeviceBuffer:
    """Raw HBM allocation (hipMalloc), 256-byte aligned."""

    def __init__(self, nbytes):
        p = C.c_void_p()
        call("gdsp_malloc", C.byref(p), int(nbytes))
        self.ptr = p.value
        self.nbytes = int(nbytes)

    def free(self):
        if self.ptr:
            call("gdsp_free", C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def upload(self, arr, offset=0, stream=None):
        arr = np.ascontiguousarray(arr)
        assert offset + arr.nbytes <= self.nbytes
        sync(stream)                     # nothing launched earlier, on whatever stream, may still be using the bytes
        call("gdsp_memcpy_h2d", C.c_void_p(self.ptr + offset), arr.ctypes.data_as(C.c_void_p), arr.nbytes, _sp(stream))
        sync(stream)

    def download(self, dtype, count, offset=0, stream=None):
        out = np.empty(count, dtype)
        assert offset + out.nbytes <= self.nbytes
        sync(stream)                     # producers on other (non-blocking) streams included when stream is None
        call("gdsp_memcpy_d2h", out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr + offset), out.nbytes, _sp(stream))
        sync(stream)
        return out


class DeviceVector:
    """A chromosome's worth of f64 values in HBM (the reference's spec.valVector)."""

    def __init__(self, n, buf=None, offset=0):
        self.n = int(n)
        self.buf = buf if buf is not None else DeviceBuffer(max(self.n, 2) * 8)
        self.offset = offset
        assert offset % 16 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.buf.ptr + self.offset)

    @classmethod
    def from_numpy(cls, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        v = cls(arr.size)
        if arr.size:
            v.buf.upload(arr, v.offset)
        return v

    def numpy(self):
        return self.buf.download(np.float64, self.n, self.offset)

    def like(self):
        return DeviceVector(self.n)

    def copy(self, stream=None):
        out = self.like()
        if self.n:
            sync(stream)
            call("gdsp_memcpy_d2d", out.ptr, self.ptr, self.n * 8, _sp(stream))
        return out


def _dev_array(arr, dtype):
    arr = np.ascontiguousarray(arr, dtype=dtype)
    buf = DeviceBuffer(max(arr.nbytes, 16))
    if arr.nbytes:
        buf.upload(arr)
    return buf


# ----------------------------------------------------------------- sum.c ----

def hann_taps(W):
    w = np.empty(W, np.float64)
    call("gdsp_hann_taps", W, w.ctypes.data_as(C.c_void_p))
    return w


class FirPlan:
    def __init__(self, taps):
        taps = np.ascontiguousarray(taps, dtype=np.float64)
        h = C.c_void_p()
        call("gdsp_fir_plan_create", C.byref(h), taps.ctypes.data_as(C.c_void_p), taps.size)
        self.handle = h.value
        self.W = taps.size

    def apply(self, v, out=None, mode=FIR_EXACT, stream=None):
        out = out if out is not None else v.like()
        call("gdsp_fir_apply", C.c_void_p(self.handle), v.ptr, out.ptr, v.n, mode, _sp(stream))
        return out

    def close(self):
        if self.handle:
            call("gdsp_fir_plan_destroy", C.c_void_p(self.handle))
            self.handle = None


def smooth(v, W=101, out=None, mode=FIR_EXACT, stream=None):
    out = out if out is not None else v.like()
    call("gdsp_smooth", v.ptr, out.ptr, v.n, W, mode, _sp(stream))
    return out


def smooth_local_extrema(v, W, N, want_max, fill, out=None, mode=FIR_EXACT, stream=None):
    """`= smooth W = localmax|localmin N` fused (bit-identical to the two calls in sequence)."""
    out = out if out is not None else v.like()
    call("gdsp_smooth_local_extrema", v.ptr, out.ptr, v.n, W, mode, N, int(want_max), float(fill), _sp(stream))
    return out


def _long_work(v):
    nbytes = lib().gdsp_long_window_work(v.n)
    return DeviceBuffer(nbytes), nbytes


def sliding_sum(v, W, denom=1.0, out=None, stream=None):
    out = out if out is not None else v.like()
    if W <= 8192:
        call("gdsp_sliding_sum", v.ptr, out.ptr, v.n, W, float(denom), _sp(stream))
        return out
    work, nbytes = _long_work(v)
    call("gdsp_sliding_sum_any", v.ptr, out.ptr, v.n, W, float(denom), C.c_void_p(work.ptr), nbytes, _sp(stream))
    sync(stream)
    return out


def window_sum(v, W, denom=1.0, use_actual=False, zero=0.0, stream=None):
    call("gdsp_window_sum", v.ptr, v.n, W, float(denom), int(use_actual), float(zero), _sp(stream))
    return v


def cumulative_sum(v, stream=None):
    work = DeviceBuffer(lib().gdsp_cumulative_sum_work(v.n))
    call("gdsp_cumulative_sum", v.ptr, v.n, C.c_void_p(work.ptr), _sp(stream))
    sync(stream)
    return v


# -------------------------------------------------------------- minmax.c ----

def local_extrema(v, N, want_max, fill, out=None, stream=None):
    out = out if out is not None else v.like()
    if N <= 4096:
        call("gdsp_local_extrema", v.ptr, out.ptr, v.n, N, int(want_max), float(fill), _sp(stream))
        return out
    work, nbytes = _long_work(v)
    call("gdsp_local_extrema_any", v.ptr, out.ptr, v.n, N, int(want_max), float(fill), C.c_void_p(work.ptr), nbytes, _sp(stream))
    sync(stream)
    return out


def localmax(v, N=3, zero=0.0, **kw):
    return local_extrema(v, N, True, zero, **kw)


def localmin(v, N=3, infinity=DBL_MAX, **kw):
    return local_extrema(v, N, False, infinity, **kw)


def best_extrema(v, W, want_max, out=None, stream=None):
    out = out if out is not None else v.like()
    if W <= 4096:
        call("gdsp_best_extrema", v.ptr, out.ptr, v.n, W, int(want_max), _sp(stream))
        return out
    work, nbytes = _long_work(v)
    call("gdsp_best_extrema_any", v.ptr, out.ptr, v.n, W, int(want_max), C.c_void_p(work.ptr), nbytes, _sp(stream))
    sync(stream)
    return out


# -------------------------------- slidingpercentile / median (not in the reference) ----

SLIDING_PERCENTILE_MAX_WINDOW = 4095          # GDSP_SLIDING_PERCENTILE_MAX_WINDOW


def sliding_percentile(v, W, p_thousandths, out=None, stream=None):
    """out[i] = the exact p-th percentile (in thousandths of a percent) of v over the window of base i: bestmax's
    window, truncated at the ends; the k-th smallest with k = gdsp_percentile_rank(bases in the window, p)."""
    out = out if out is not None else v.like()
    call("gdsp_sliding_percentile", v.ptr, out.ptr, v.n, int(W), int(p_thousandths), _sp(stream))
    return out


def median(v, W, out=None, stream=None):
    return sliding_percentile(v, W, 50000, out=out, stream=stream)


# ------------------------------------------------- prominence (not in the reference) ----

PROMINENCE_MAX_WINDOW = 4095                  # GDSP_PROMINENCE_MAX_WINDOW
PROMINENCE_WHAT = {"prominence": 0, "base": 1}    # GDSP_PROMINENCE_VALUE, GDSP_PROMINENCE_BASE


def _prominence_what(as_):
    if as_ not in PROMINENCE_WHAT:
        raise ValueError("as_ must be 'prominence' or 'base', not %r" % (as_,))
    return PROMINENCE_WHAT[as_]


def prominence(v, W, as_="prominence", out=None, stream=None):
    """out[i] = how far v[i] stands above the higher of the two lowest values met while walking left and right from i,
    inside bestmax's window, up to the first strictly greater value (gdsp_prominence in include/genodsp_hip.h; for odd
    W scipy.signal.peak_prominences with wlen=W at every base).  as_="base" writes that level instead."""
    what = _prominence_what(as_)
    out = out if out is not None else v.like()
    call("gdsp_prominence", v.ptr, out.ptr, v.n, int(W), what, _sp(stream))
    return out


# ------------------------------------------------- localstats (not in the reference) ----

LOCALSTATS_MAX_WINDOW = 12287                 # GDSP_LOCALSTATS_MAX_WINDOW
LOCALSTATS_WHAT = {"zscore": 0, "mean": 1, "variance": 2, "stddev": 3, "difference": 4, "ratio": 5}    # GDSP_LOCALSTATS_*


def _localstats_params(W, as_, floor, minsd):
    if as_ not in LOCALSTATS_WHAT:
        raise ValueError("as_ must be one of %s, not %r" % (", ".join(LOCALSTATS_WHAT), as_))
    return (int(W), LOCALSTATS_WHAT[as_], int(floor is not None), float(floor or 0.0),
            int(minsd is not None), float(minsd or 0.0))


def local_stats(v, W, as_="zscore", floor=None, minsd=None, out=None, stream=None):
    """out[c] = v[c] against the mean and the population variance of slidingsum's window around c, cut off at the ends
    of the vector (gdsp_localstats in include/genodsp_hip.h): the z-score, or with as_ the mean, variance, stddev,
    difference or ratio.  floor: max(mean, floor) stands for the mean in mean, difference and ratio; minsd: max(stddev,
    minsd) for the stddev in stddev and zscore."""
    params = _localstats_params(W, as_, floor, minsd)
    out = out if out is not None else v.like()
    call("gdsp_localstats", v.ptr, out.ptr, v.n, *params, _sp(stream))
    return out


# ------------------------------------------- localmad / hampel (not in the reference) ----

LOCALMAD_MAX_WINDOW = 4095                    # GDSP_LOCALMAD_MAX_WINDOW
LOCALMAD_WHAT = {"zscore": 0, "median": 1, "mad": 2, "difference": 3, "clean": 4, "outlier": 5}        # GDSP_LOCALMAD_*


def _localmad_params(W, as_, scale, threshold, minmad):
    if as_ not in LOCALMAD_WHAT:
        raise ValueError("as_ must be one of %s, not %r" % (", ".join(LOCALMAD_WHAT), as_))
    return (int(W), LOCALMAD_WHAT[as_], float(scale), float(threshold), int(minmad is not None), float(minmad or 0.0))


def localmad_tile(W):
    """outputs per workgroup tile of the kernel for window W; 0 outside 1 .. LOCALMAD_MAX_WINDOW (host code)"""
    return lib().gdsp_localmad_tile(int(W))


def local_mad(v, W, as_="zscore", scale=1.4826, threshold=3.0, minmad=None, out=None, stream=None):
    """out[i] = v[i] against the median and the median absolute deviation (MAD) of slidingpercentile's window around i,
    cut off at the ends of the vector (gdsp_localmad in include/genodsp_hip.h): the robust z-score
    (v - median) / (scale * MAD), or with as_ the median, mad, difference, clean (the median where |difference| >
    threshold * scale * MAD, else v: the Hampel filter) or outlier (1 there, else 0).  minmad: max(MAD, minmad) stands
    for the MAD."""
    params = _localmad_params(W, as_, scale, threshold, minmad)
    out = out if out is not None else v.like()
    call("gdsp_localmad", v.ptr, out.ptr, v.n, *params, _sp(stream))
    return out


def hampel(v, W, as_="clean", scale=1.4826, threshold=3.0, minmad=None, out=None, stream=None):
    """the Hampel filter: local_mad with as_="clean" """
    return local_mad(v, W, as_=as_, scale=scale, threshold=threshold, minmad=minmad, out=out, stream=stream)


# ----------------------------------------------- localcorrelate (not in the reference) ----

LOCALCORR_MAX_WINDOW = 4097                   # GDSP_LOCALCORR_MAX_WINDOW
LOCALCORR_WHAT = {"correlation": 0, "covariance": 1, "slope": 2, "intercept": 3}      # GDSP_LOCALCORR_*


def _localcorr_what(as_):
    if as_ not in LOCALCORR_WHAT:
        raise ValueError("as_ must be one of %s, not %r" % (", ".join(LOCALCORR_WHAT), as_))
    return LOCALCORR_WHAT[as_]


def localcorr_tile(W):
    """outputs per workgroup tile of the kernel for window W; 0 outside 1 .. LOCALCORR_MAX_WINDOW (host code)"""
    return lib().gdsp_localcorr_tile(int(W))


def local_correlation(x, y, W, as_="correlation", stream=None):
    """y[c] = the correlation of x and y over slidingsum's window around c, cut off at the ends of the vectors
    (gdsp_localcorr in include/genodsp_hip.h), or with as_ their covariance, or the slope or intercept of y regressed
    on x.  y is overwritten and returned; x is only read."""
    what = _localcorr_what(as_)
    if x.n != y.n:
        raise ValueError("x and y must have the same length (%d, %d)" % (x.n, y.n))
    call("gdsp_localcorr", x.ptr, y.ptr, x.n, int(W), what, _sp(stream))
    return y


# --------------------------------------------------- distance (not in the reference) ----

DISTANCE_TO = {"nearest": 0, "left": 1, "right": 2}    # GDSP_DISTANCE_*


def _distance_params(T, ties_above, to, signed, cap):
    if to not in DISTANCE_TO:
        raise ValueError("to must be one of %s, not %r" % (", ".join(DISTANCE_TO), to))
    if cap is not None and int(cap) < 1:
        raise ValueError("cap must be at least 1 (None: no cap), not %r" % (cap,))
    return float(T), int(bool(ties_above)), DISTANCE_TO[to], int(bool(signed)), int(cap or 0)


def distance(v, T=0.0, ties_above=False, to="nearest", signed=False, cap=None, stream=None):
    """v[i] = the distance in bases from i to the nearest member (v > T, or >= with ties_above) on the side(s) `to`
    names, len(v) where there is none; signed: members get minus their distance to the nearest non-member; cap: no
    result beyond it (gdsp_distance in include/genodsp_hip.h).  In place."""
    call("gdsp_distance", v.ptr, v.n, *_distance_params(T, ties_above, to, signed, cap), _sp(stream))
    return v


# --------------------------------------------------- fillgaps (not in the reference) ----

FILL_KNOWN = {"above": 0, "nonzero": 1}                           # GDSP_FILL_KNOWN_*
FILL_HOW = {"linear": 0, "nearest": 1, "left": 2, "right": 3}     # GDSP_FILL_LINEAR ..
FILL_ENDS = {"extend": 0, "keep": 1}                              # GDSP_FILL_ENDS_*


def _fill_params(T, ties_above, known, how, ends, maxgap):
    for what, value, names in (("known", known, FILL_KNOWN), ("how", how, FILL_HOW), ("ends", ends, FILL_ENDS)):
        if value not in names:
            raise ValueError("%s must be one of %s, not %r" % (what, ", ".join(names), value))
    if maxgap is not None and int(maxgap) < 1:
        raise ValueError("maxgap must be at least 1 (None: no limit), not %r" % (maxgap,))
    return float(T), int(bool(ties_above)), FILL_KNOWN[known], FILL_HOW[how], FILL_ENDS[ends], int(maxgap or 0)


def fill_gaps(v, T=0.0, ties_above=False, known="above", how="linear", ends="extend", maxgap=None, stream=None):
    """the unknown bases of v (not above T, or >= with ties_above; with known="nonzero": zero or NaN) take their values from
    the known bases before and behind their gap: on the line between the two, or the nearest's, the left's, the right's;
    ends: what a base does whose side does not exist; maxgap: longer gaps are left alone (gdsp_fillgaps in
    include/genodsp_hip.h).  In place."""
    call("gdsp_fillgaps", v.ptr, v.n, *_fill_params(T, ties_above, known, how, ends, maxgap), _sp(stream))
    return v


# ---------------------------------------------------------- morphology.c ----

def split_length(length):
    """dilate/erode <length> -> (left, right), morphology.c:917-920 / :1369-1372."""
    left = int(float(length) / 2)
    return left, int(length) - left


def dilate(v, left, right, T=0.0, one=1.0, zero=0.0, out=None, stream=None):
    out = out if out is not None else v.like()
    work, nbytes = _long_work(v) if left + right > 200000 else (None, 0)
    call("gdsp_dilate_any", v.ptr, out.ptr, v.n, left, right, float(T), float(one), float(zero),
         C.c_void_p(work.ptr) if work else None, nbytes, _sp(stream))
    if work:
        sync(stream)
    return out


def erode(v, left, right, T=0.0, one=1.0, zero=0.0, out=None, stream=None):
    out = out if out is not None else v.like()
    work, nbytes = _long_work(v) if left + right > 200000 else (None, 0)
    call("gdsp_erode_any", v.ptr, out.ptr, v.n, left, right, float(T), float(one), float(zero),
         C.c_void_p(work.ptr) if work else None, nbytes, _sp(stream))
    if work:
        sync(stream)
    return out


def dilate_erode(v, d_left, d_right, e_left, e_right, d_T=0.0, d_one=1.0, d_zero=0.0, e_T=0.0, e_one=1.0,
                 e_zero=0.0, binarize=None, out=None, stream=None):
    """`= dilate = erode [= binarize]` fused; binarize = (T, ties_above, one, zero) or None."""
    out = out if out is not None else v.like()
    b = binarize if binarize is not None else (0.0, False, 1.0, 0.0)
    call("gdsp_dilate_erode", v.ptr, out.ptr, v.n, d_left, d_right, float(d_T), float(d_one), float(d_zero),
         e_left, e_right, float(e_T), float(e_one), float(e_zero), int(binarize is not None),
         float(b[0]), int(b[1]), float(b[2]), float(b[3]), _sp(stream))
    return out


def close(v, length, T=0.0, one=1.0, zero=0.0, out=None, stream=None):
    out = out if out is not None else v.like()
    work, nbytes = _long_work(v) if length > 100000 else (None, 0)
    call("gdsp_close_any", v.ptr, out.ptr, v.n, float(length), float(T), float(one), float(zero),
         C.c_void_p(work.ptr) if work else None, nbytes, _sp(stream))
    if work:
        sync(stream)
    return out


def open_(v, length, T=0.0, one=1.0, zero=0.0, out=None, stream=None):
    out = out if out is not None else v.like()
    work, nbytes = _long_work(v) if length > 100000 else (None, 0)
    call("gdsp_open_any", v.ptr, out.ptr, v.n, float(length), float(T), float(one), float(zero),
         C.c_void_p(work.ptr) if work else None, nbytes, _sp(stream))
    if work:
        sync(stream)
    return out


def morph_bits(op, v, *args, **kw):
    """the workspace form of dilate / erode / close / open whatever the length (GDSP_MORPH_FORCE_BITS is read once per
    process by the library, so tests call the entry points with workspace and the variable set before the first call)"""
    out = v.like()
    work, nbytes = _long_work(v)
    a = [float(x) if isinstance(x, float) else x for x in args]
    call("gdsp_%s_any" % op, v.ptr, out.ptr, v.n, *a, C.c_void_p(work.ptr), nbytes, _sp(kw.get("stream")))
    sync(kw.get("stream"))
    return out


# --------------------------------------------- logical.c, mask.c, add.c ----

def binarize(v, T=0.0, ties_above=False, one=1.0, zero=0.0, stream=None):
    call("gdsp_binarize", v.ptr, v.n, float(T), int(ties_above), float(one), float(zero), _sp(stream))
    return v


def clip(v, lo=None, hi=None, stream=None):
    call("gdsp_clip", v.ptr, v.n, lo is not None, 0.0 if lo is None else float(lo),
         hi is not None, 0.0 if hi is None else float(hi), _sp(stream))
    return v


def erase(v, lo=None, hi=None, keep_inside=False, zero=0.0, stream=None):
    call("gdsp_erase", v.ptr, v.n, lo is not None, 0.0 if lo is None else float(lo),
         hi is not None, 0.0 if hi is None else float(hi), int(keep_inside), float(zero), _sp(stream))
    return v


def add_constant(v, c, stream=None):
    call("gdsp_add_constant", v.ptr, v.n, float(c), _sp(stream))
    return v


def abs_(v, stream=None):
    call("gdsp_abs", v.ptr, v.n, _sp(stream))
    return v


def invert(v, mid, stream=None):
    call("gdsp_invert", v.ptr, v.n, float(mid), _sp(stream))
    return v


def map_values(v, knots_in, knots_out, stream=None):
    """op_map_apply: piecewise-linear mapping through knots sorted by knots_in."""
    a = _dev_array(knots_in, np.float64)
    b = _dev_array(knots_out, np.float64)
    call("gdsp_map", v.ptr, v.n, C.c_void_p(a.ptr), C.c_void_p(b.ptr), len(knots_in), _sp(stream))
    sync(stream)
    return v


def clump(v, average, min_length, above=True, one=1.0, zero=0.0, stream=None):
    """op_clump_apply (above) / op_skimp_apply: in place."""
    work = DeviceBuffer(lib().gdsp_clump_work(v.n))
    call("gdsp_clump", v.ptr, v.n, float(average), int(min_length), int(bool(above)), float(one), float(zero),
         C.c_void_p(work.ptr), _sp(stream))
    sync(stream)
    return v


def fill(v, val, stream=None):
    call("gdsp_fill", v.ptr, v.n, float(val), _sp(stream))
    return v


def genome_minmax(vecs, window=1, lo=-DBL_MAX, hi=DBL_MAX, stream=None):
    """(min, max, count) over the sampled values of all vectors."""
    acc = DeviceBuffer(32)
    call("gdsp_minmax_init", C.c_void_p(acc.ptr), _sp(stream))
    for v in vecs:
        call("gdsp_minmax_update", v.ptr, v.n, window, float(lo), float(hi), C.c_void_p(acc.ptr), _sp(stream))
    r = acc.download(np.float64, 3, stream=stream)
    return float(r[0]), float(r[1]), int(r[2])


# ---------------------------------------------------------- percentile.c ----

# digit schedule over the 64-bit key: sign+exponent first, then the mantissa
SELECT_DIGITS = [(52, 12), (39, 13), (26, 13), (13, 13), (0, 13)]


def radix_select(histogram, p_thousandths, allreduce=None):
    """Host side of the exact order statistic (percentile.c:587-710), shared by every backend.

    histogram(shift, bits, prefix) -> np.uint64 array of (1<<bits)+2 words for THIS rank's
    chromosomes: the digit counts, then the smallest and the largest matching key.
    allreduce(array, op) -> the "sum" / "min" / "max" of the array over ranks (None: one rank).
    Returns (count, [values])."""
    L = lib()
    results = []
    count = None
    first = None           # the prefix-free first pass is shared by every requested percentile

    def reduced(shift, bits, prefix):
        nb = 1 << bits
        h = np.array(histogram(shift, bits, prefix), dtype=np.uint64)
        if allreduce is not None:
            h[:nb] = allreduce(h[:nb].copy(), "sum")
            h[nb:nb + 1] = allreduce(h[nb:nb + 1].copy(), "min")
            h[nb + 1:] = allreduce(h[nb + 1:].copy(), "max")
        return h

    for pt in p_thousandths:
        prefix, value, k = 0, None, None
        for di, (shift, bits) in enumerate(SELECT_DIGITS):
            nb = 1 << bits
            if di == 0:
                if first is None:
                    first = reduced(shift, bits, 0)
                    count = int(first[:nb].sum())
                if count == 0:
                    return 0, []
                hist = first
                k = L.gdsp_percentile_rank(count, int(pt))
            else:
                hist = reduced(shift, bits, prefix)
            if hist[nb] == hist[nb + 1]:           # one distinct candidate left
                value = L.gdsp_key_to_double(int(hist[nb]))
                break
            b, kw = C.c_uint32(), C.c_uint64()
            call("gdsp_select_pick", hist.ctypes.data_as(C.c_void_p), bits, C.c_uint64(k), C.byref(b), C.byref(kw))
            prefix |= b.value << shift
            k = kw.value
        if value is None:
            value = L.gdsp_key_to_double(prefix)
        results.append(value)
    return count, results


class SelectSource(C.Structure):
    """gdsp_select_source of include/genodsp_hip.h"""
    _fields_ = [("d_v", C.c_void_p), ("n", C.c_uint32), ("device", C.c_int), ("stream", C.c_void_p)]


REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.c_int)
DEVICE_REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
SELECT_AUTO, SELECT_RADIX, SELECT_BRACKET = 0, 1, 2


import contextlib as _contextlib
import threading as _threading
_PERCENTILE_HOOK = _threading.RLock()


def _reduce_hook(allreduce, failure):
    """allreduce(np.uint64 array, "sum"|"min"|"max") -> the reduced array, as the gdsp_reduce_fn of a library call (a
    NULL one for None).  An exception must not unwind through the C frames: it is kept in `failure` and the library is
    told that the reduction failed."""
    if allreduce is None:
        return C.cast(None, REDUCE_FN)

    def reduce(_ctx, words, n, op):
        try:
            arr = np.ctypeslib.as_array(words, shape=(n,))
            arr[:] = allreduce(arr.copy(), ("sum", "min", "max")[op])
            return 0
        except Exception as e:
            failure.append(e)
            return 1

    return REDUCE_FN(reduce)


@_contextlib.contextmanager
def _hook_failure_first(failure):
    """The library's complaint about a failed hook becomes the exception the hook raised."""
    try:
        yield
    except GdspError:
        if failure:
            raise failure[0]
        raise


def percentile(vecs, p_thousandths, window=1, lo=-DBL_MAX, hi=DBL_MAX, allreduce=None, stream=None,
               strategy=SELECT_AUTO, sample_target=0, device_allreduce=None):
    """Exact percentiles of the sampled genome (percentile.c:392-751), non-destructive: gdsp_percentiles.
    vecs: this rank's chromosome vectors (current device).  Across ranks, one of
      device_allreduce(ptr, count, "sum"|"min"|"max", stream): all-reduce `count` u64 words at DEVICE address `ptr`
        in place, ordered on `stream` (RCCL through torch.distributed in bench.py: nothing leaves HBM);
      allreduce(np.uint64 array, op) -> the reduced array (host words; the gloo tests).
    Returns (count, [values])."""
    device = current_device()
    src = (SelectSource * max(1, len(vecs)))()
    for i, v in enumerate(vecs):
        src[i].d_v, src[i].n, src[i].device, src[i].stream = v.ptr, v.n, device, stream
    pts = (C.c_uint32 * len(p_thousandths))(*[int(p) for p in p_thousandths])
    vals = (C.c_double * len(p_thousandths))()
    count = C.c_uint64(0)
    failure = []

    def device_reduce(_ctx, d_words, n, op, s):
        try:
            device_allreduce(d_words, n, ("sum", "min", "max")[op], s)
            return 0
        except Exception as e:
            failure.append(e)
            return 1

    assert allreduce is None or device_allreduce is None
    cb = _reduce_hook(allreduce, failure)
    dcb = DEVICE_REDUCE_FN(device_reduce) if device_allreduce is not None else None
    # the device hook is state of the library (one per process): installed, used and cleared under one lock, so that
    # two threads calling percentile() cannot swap or clear each other's hook in mid-call
    with _PERCENTILE_HOOK:
        try:
            with _hook_failure_first(failure):
                if dcb is not None:
                    call("gdsp_percentiles_use_device_reduce", dcb, None)
                call("gdsp_percentiles", src, len(vecs), int(window), float(lo), float(hi), pts, len(p_thousandths),
                     int(strategy), int(sample_target), cb, None, vals, C.byref(count))
        finally:
            if dcb is not None:
                call("gdsp_percentiles_use_device_reduce", None, None)
    if count.value == 0:
        return 0, []
    return int(count.value), [float(x) for x in vals]


# ------------------------------------------------ stats / normalize (not in the reference) ----

XSUM_WORDS, XSUM_DIGITS = 72, 68                   # GDSP_XSUM_WORDS, GDSP_XSUM_DIGITS
XSUM_WORD_COUNT, XSUM_WORD_INF, XSUM_WORD_FLUSHES = 68, 69, 70


class XsumSource(C.Structure):
    """gdsp_xsum_source of include/genodsp_hip.h"""
    _fields_ = [("d_v", C.c_void_p), ("n", C.c_uint32), ("first", C.c_uint32), ("device", C.c_int), ("stream", C.c_void_p)]


def xsum_sources(vecs, stream=None):
    """The source table of gdsp_genome_stats / gdsp_xsum_*: each item a DeviceVector (a whole chromosome), or a tuple
    (vector, start, count[, first]) for values [start, start+count) of the vector whose chromosome position is `first`
    (default: start) -- the window counts from the chromosome's first base."""
    device = current_device()
    src = (XsumSource * max(1, len(vecs)))()
    for i, item in enumerate(vecs):
        if isinstance(item, DeviceVector):
            v, start, count, first = item, 0, item.n, 0
        else:
            v, start, count = item[0], int(item[1]), int(item[2])
            first = int(item[3]) if len(item) > 3 else start
        assert 0 <= start and start + count <= v.n
        src[i].d_v, src[i].n, src[i].first = v.ptr.value + 8 * start, count, first
        src[i].device, src[i].stream = device, stream
    return src


def genome_stats(vecs, window=1, lo=-DBL_MAX, hi=DBL_MAX, allreduce=None, stream=None):
    """count, sum, mean, variance, stddev of the sampled genome, each exact and rounded once (gdsp_genome_stats): every
    window-th value counted from each chromosome's first base with lo <= v <= hi (never NaN or +-inf).  vecs: as
    xsum_sources.  allreduce(np.uint64 array, "sum") -> the array summed over ranks (None: one rank), percentile's hook.
    count 0: sum 0.0 and the rest NaN."""
    src = xsum_sources(vecs, stream)
    out = (C.c_double * 5)()
    failure = []
    cb = _reduce_hook(allreduce, failure)
    with _hook_failure_first(failure):
        call("gdsp_genome_stats", src, len(vecs), int(window), float(lo), float(hi), cb, None, out)
    return dict(zip(("count", "sum", "mean", "variance", "stddev"), [float(x) for x in out]))


def genome_stats_last():
    """What the last genome_stats did: n, lane flushes into LDS in pass 1 and pass 2, squares that were +inf."""
    out = (C.c_uint64 * 4)()
    lib().gdsp_genome_stats_last(out)
    return dict(zip(("count", "flushes1", "flushes2", "inf_squares"), [int(x) for x in out]))


def xsum_accumulate(vecs, acc, window=1, lo=-DBL_MAX, hi=DBL_MAX, mean=None, stream=None):
    """One pass into the accumulator `acc` (a DeviceBuffer of XSUM_WORDS u64 words): v, or fl(fl(v - mean)^2) when mean
    is given.  The image is not folded."""
    src = xsum_sources(vecs, stream)
    if mean is None:
        call("gdsp_xsum_accumulate_batch", src, len(vecs), int(window), float(lo), float(hi), C.c_void_p(acc.ptr), _sp(stream))
    else:
        call("gdsp_xsum_accumulate_sq_batch", src, len(vecs), int(window), float(lo), float(hi), float(mean),
             C.c_void_p(acc.ptr), _sp(stream))


def xsum_image(vecs, window=1, lo=-DBL_MAX, hi=DBL_MAX, mean=None, stream=None, fold=True):
    """The (folded) accumulator image of one pass over vecs, as np.uint64[XSUM_WORDS]."""
    acc = DeviceBuffer(XSUM_WORDS * 8)
    call("gdsp_xsum_init", C.c_void_p(acc.ptr), _sp(stream))
    xsum_accumulate(vecs, acc, window, lo, hi, mean, stream)
    if fold:
        call("gdsp_xsum_fold", C.c_void_p(acc.ptr), _sp(stream))
    return acc.download(np.uint64, XSUM_WORDS, stream=stream)


def xsum_round(image):
    """Host, no GPU: the value of an image rounded once."""
    img = np.ascontiguousarray(image, dtype=np.uint64)
    assert img.size == XSUM_WORDS
    return lib().gdsp_xsum_round(img.ctypes.data_as(C.c_void_p))


def xsum_div_round(image, n):
    """Host, no GPU: the value of an image divided by n, rounded once."""
    img = np.ascontiguousarray(image, dtype=np.uint64)
    assert img.size == XSUM_WORDS
    return lib().gdsp_xsum_div_round(img.ctypes.data_as(C.c_void_p), int(n))


def xsum_add_host(image, x):
    """Host, no GPU: add x to an image (np.uint64[XSUM_WORDS], in place) and 1 to its count."""
    assert image.dtype == np.uint64 and image.flags.c_contiguous and image.size == XSUM_WORDS
    lib().gdsp_xsum_add_host(image.ctypes.data_as(C.c_void_p), float(x))
    return image


# ------------------------------------------------------ correlate (not in the reference) ----

CORRELATION_FIGURES = ("count", "sumx", "sumy", "meanx", "meany", "varx", "vary", "sdx", "sdy", "covariance", "correlation",
                       "slope", "intercept")          # the GDSP_CORR_* order of include/genodsp_hip.h


class XsumPair(C.Structure):
    """gdsp_xsum_pair of include/genodsp_hip.h"""
    _fields_ = [("d_x", C.c_void_p), ("d_y", C.c_void_p), ("n", C.c_uint32), ("first", C.c_uint32), ("device", C.c_int),
                ("stream", C.c_void_p)]


def xsum_pair_tile():
    """Pairs per tile of the pair kernel's walk."""
    return int(lib().gdsp_xsum_pair_tile())


def xsum_pairs(pairs, stream=None):
    """The pair table of gdsp_genome_correlation / gdsp_xsum_pair_*: each item (x, y), x and y each as an item of
    xsum_sources (a DeviceVector, or (vector, start, count[, first])) of equal counts; `first` is x's."""
    device = current_device()
    tab = (XsumPair * max(1, len(pairs)))()
    for i, (x, y) in enumerate(pairs):
        sx, sy = xsum_sources([x], stream)[0], xsum_sources([y], stream)[0]
        assert sx.n == sy.n
        tab[i].d_x, tab[i].d_y, tab[i].n, tab[i].first = sx.d_v, sy.d_v, sx.n, sx.first
        tab[i].device, tab[i].stream = device, stream
    return tab


def genome_correlation(pairs, window=1, lo=-DBL_MAX, hi=DBL_MAX, ylo=-DBL_MAX, yhi=DBL_MAX, allreduce=None, stream=None):
    """The figures of CORRELATION_FIGURES over the pair sample, each exact and rounded once or derived from such on the
    host (gdsp_genome_correlation): every window-th position counted from each chromosome's first base with
    lo <= x <= hi and ylo <= y <= yhi (never NaN or +-inf).  pairs: as xsum_pairs.  allreduce: genome_stats' hook.
    count 0: sums 0.0 and the rest NaN."""
    tab = xsum_pairs(pairs, stream)
    out = (C.c_double * len(CORRELATION_FIGURES))()
    failure = []
    cb = _reduce_hook(allreduce, failure)
    with _hook_failure_first(failure):
        call("gdsp_genome_correlation", tab, len(pairs), int(window), float(lo), float(hi), float(ylo), float(yhi), cb, None, out)
    return dict(zip(CORRELATION_FIGURES, [float(x) for x in out]))


def genome_correlation_last():
    """What the last genome_correlation did: n, lane flushes into LDS in pass 1 and pass 2, and the qxx, qyy, qxy that
    were not finite."""
    out = (C.c_uint64 * 8)()
    lib().gdsp_genome_correlation_last(out)
    return dict(zip(("count", "flushes1", "flushes2", "nonfinite_qxx", "nonfinite_qyy", "nonfinite_qxy"), [int(x) for x in out]))


def xsum_pair_image(pairs, window=1, lo=-DBL_MAX, hi=DBL_MAX, ylo=-DBL_MAX, yhi=DBL_MAX, means=None, stream=None, fold=True):
    """The (folded) accumulator images of one pass over pairs, as np.uint64[k, XSUM_WORDS]: k = 2 (the sums of x and of y)
    or, with means = (meanx, meany), k = 3 (the sums of qxx, qyy, qxy)."""
    k = 2 if means is None else 3
    acc = DeviceBuffer(k * XSUM_WORDS * 8)
    for i in range(k):
        call("gdsp_xsum_init", C.c_void_p(acc.ptr + i * XSUM_WORDS * 8), _sp(stream))
    tab = xsum_pairs(pairs, stream)
    if means is None:
        call("gdsp_xsum_pair_accumulate_batch", tab, len(pairs), int(window), float(lo), float(hi), float(ylo), float(yhi),
             C.c_void_p(acc.ptr), _sp(stream))
    else:
        call("gdsp_xsum_pair_accumulate_dev_batch", tab, len(pairs), int(window), float(lo), float(hi), float(ylo), float(yhi),
             float(means[0]), float(means[1]), C.c_void_p(acc.ptr), _sp(stream))
    if fold:
        for i in range(k):
            call("gdsp_xsum_fold", C.c_void_p(acc.ptr + i * XSUM_WORDS * 8), _sp(stream))
    return acc.download(np.uint64, k * XSUM_WORDS, stream=stream).reshape(k, XSUM_WORDS)


# ------------------------------------- crosscorrelate / autocorrelate (not in the reference) ----

LAG_MAX_LAGS = 4096


def lag_tile():
    """Positions per tile of the lag kernel's walk."""
    return int(lib().gdsp_lag_tile())


def lag_block():
    """Lags a workgroup of the lag kernel owns."""
    return int(lib().gdsp_lag_block())


def lag_products(pairs, lag_lo, nlags, meanx, meany, stream=None):
    """The folded images of the lagged products of pairs (as xsum_pairs, whole chromosomes), np.uint64[nlags, XSUM_WORDS]:
    image k sums fl(fl(x[i] - meanx) * fl(y[i + lag_lo + k] - meany)) exactly (gdsp_lag_products_batch); its count word
    is the number of products taken, its INF word those that were not finite."""
    nlags = int(nlags)
    acc = DeviceBuffer(max(1, nlags) * XSUM_WORDS * 8)
    acc.upload(np.zeros(max(1, nlags) * XSUM_WORDS, np.uint64), stream=stream)
    tab = xsum_pairs(pairs, stream)
    call("gdsp_lag_products_batch", tab, len(pairs), int(lag_lo), nlags, float(meanx), float(meany), C.c_void_p(acc.ptr), _sp(stream))
    return acc.download(np.uint64, nlags * XSUM_WORDS, stream=stream).reshape(nlags, XSUM_WORDS)


def genome_lag_correlation(pairs, lag_lo, nlags, allreduce=None, stream=None):
    """Covariance and correlation of x against y shifted by each of the lags lag_lo .. lag_lo + nlags - 1, each exact and
    rounded once (gdsp_genome_lag_correlation): the figures of CORRELATION_FIGURES over the bases where both are finite,
    and under "lags", "pairs", "covariances", "correlations" one np array entry per lag.  pairs: as xsum_pairs, whole
    chromosomes.  allreduce: genome_stats' hook."""
    nlags = int(nlags)
    tab = xsum_pairs(pairs, stream)
    fig = (C.c_double * len(CORRELATION_FIGURES))()
    count = np.zeros(max(1, nlags), np.uint64)
    cov = np.zeros(max(1, nlags), np.float64)
    corr = np.zeros(max(1, nlags), np.float64)
    failure = []
    cb = _reduce_hook(allreduce, failure)
    with _hook_failure_first(failure):
        call("gdsp_genome_lag_correlation", tab, len(pairs), int(lag_lo), nlags, cb, None, fig,
             count.ctypes.data_as(C.c_void_p), cov.ctypes.data_as(C.c_void_p), corr.ctypes.data_as(C.c_void_p))
    out = dict(zip(CORRELATION_FIGURES, [float(x) for x in fig]))
    out["lags"] = np.arange(nlags, dtype=np.int64) + int(lag_lo)
    out["pairs"], out["covariances"], out["correlations"] = count[:nlags], cov[:nlags], corr[:nlags]
    return out


def genome_lag_correlation_last():
    """What the last genome_lag_correlation did: N, the products taken over all lags, lane flushes into the device images,
    and the products that were not finite."""
    out = (C.c_uint64 * 8)()
    lib().gdsp_genome_lag_correlation_last(out)
    return dict(zip(("count", "products", "flushes", "nonfinite_products"), [int(x) for x in out]))


# ------------------------------------------------------ profileover (not in the reference) ----

PROFILE_MAX_OFFSETS = 16384                        # GDSP_PROFILE_MAX_OFFSETS


class ProfileSource(C.Structure):
    """gdsp_profile_source of include/genodsp_hip.h"""
    _fields_ = [("d_v", C.c_void_p), ("n", C.c_uint32), ("device", C.c_int), ("stream", C.c_void_p),
                ("h_pos", C.c_void_p), ("h_minus", C.c_void_p), ("nanchors", C.c_uint32)]


def profile_block():
    """Offsets a workgroup of the profile kernel owns."""
    return int(lib().gdsp_profile_block())


def profile_set_launch_anchors(anchors):
    """Anchors per launch of the profile kernel (0: the library's own number).  For tests that force several launches."""
    call("gdsp_profile_set_launch_anchors", int(anchors))


def _profile_anchors(anchors, nvecs):
    """anchors: rows (vector index, position, strand +1 / -1) -> int64[count, 3]"""
    a = np.asarray(anchors, dtype=np.int64).reshape(-1, 3)
    assert np.all((a[:, 0] >= 0) & (a[:, 0] < max(nvecs, 1))) and np.all((a[:, 1] >= 0) & (a[:, 1] <= 0xFFFFFFFF))
    assert np.all(np.abs(a[:, 2]) == 1)
    return a


def _anchor_items(vecs, stream):
    """-> (src, items): vecs as xsum_sources, and the same whole chromosomes as the read-only BatchItem table"""
    return xsum_sources(vecs, stream), _read_only_items(vecs)


def _anchor_upload(a, stream):
    """-> (buffer, count): the anchors on the device, their positions and then their code words (vector * 2 + minus)"""
    anc = DeviceBuffer(max(1, 2 * len(a)) * 4)
    if len(a):
        anc.upload(np.concatenate([a[:, 1].astype(np.uint32), (a[:, 0] * 2 + (a[:, 2] < 0)).astype(np.uint32)]), stream=stream)
    return anc, len(a)


def _anchor_sources(src, a, stream, with_rows=None):
    """-> (tab, keep): the ProfileSource table, each vector with its own anchors in their order, and per vector the arrays
    the table points into: (where in a, positions, minus flags, rows to fill: with_rows columns each, or None)"""
    tab = (ProfileSource * len(src))()
    keep = []
    for i in range(len(src)):
        where = np.flatnonzero(a[:, 0] == i)
        pos = np.ascontiguousarray(a[where, 1], dtype=np.uint32)
        minus = np.ascontiguousarray(a[where, 2] < 0, dtype=np.uint32)
        mine = None if with_rows is None else np.zeros((max(1, pos.size), max(1, with_rows)), np.float64)
        keep.append((where, pos, minus, mine))
        tab[i].d_v, tab[i].n, tab[i].device, tab[i].stream = src[i].d_v, src[i].n, src[i].device, stream
        tab[i].h_pos, tab[i].h_minus, tab[i].nanchors = pos.ctypes.data, minus.ctypes.data, pos.size
    return tab, keep


def profile_images(vecs, anchors, off_lo, noffsets, lo=-DBL_MAX, hi=DBL_MAX, mean=None, stream=None):
    """The canonical images of one pass of gdsp_profile_accumulate_batch, np.uint64[noffsets, XSUM_WORDS]: image k sums the
    sampled values at offset off_lo + k from the anchors -- or, with mean (one per offset), their fl(fl(v - mean[k])^2).
    vecs: as xsum_sources, whole chromosomes; anchors: rows (vector index, position, strand +1 / -1)."""
    noffsets = int(noffsets)
    _, items = _anchor_items(vecs, stream)
    anc, na = _anchor_upload(_profile_anchors(anchors, len(vecs)), stream)
    acc = DeviceBuffer(max(1, noffsets) * XSUM_WORDS * 8)
    acc.upload(np.zeros(max(1, noffsets) * XSUM_WORDS, np.uint64), stream=stream)
    d_mean = None
    if mean is not None:
        m = np.ascontiguousarray(mean, dtype=np.float64)
        assert m.size == noffsets
        d_mean = DeviceBuffer(max(1, noffsets) * 8)
        d_mean.upload(m, stream=stream)
    call("gdsp_profile_accumulate_batch", items, len(vecs), C.c_void_p(anc.ptr), C.c_void_p(anc.ptr + 4 * na), na,
         int(off_lo), noffsets, float(lo), float(hi), C.c_void_p(d_mean.ptr) if d_mean is not None else None,
         C.c_void_p(acc.ptr), _sp(stream))
    return acc.download(np.uint64, noffsets * XSUM_WORDS, stream=stream).reshape(noffsets, XSUM_WORDS)


def genome_profile(vecs, anchors, off_lo, noffsets, bin=1, lo=-DBL_MAX, hi=DBL_MAX, allreduce=None, stream=None):
    """The aggregate profile of the signal around anchors (gdsp_genome_profile): per column of `bin` offsets out of
    off_lo .. off_lo + noffsets - 1, the count, sum, mean, variance and stddev of the values found that far from the
    anchors in their own direction, each exact and rounded once, and stderr = stddev / sqrt(count).  vecs: as
    xsum_sources, whole chromosomes; anchors: rows (vector index, position, strand +1 / -1); allreduce: genome_stats'
    hook.  Returns a dict of np arrays, one entry per column ("offsets": each column's lowest offset)."""
    noffsets, bin = int(noffsets), int(bin)
    tab, keep = _anchor_sources(xsum_sources(vecs, stream), _profile_anchors(anchors, len(vecs)), stream)
    ncols = noffsets // bin if bin >= 1 and noffsets >= 1 else 0
    count = np.zeros(max(1, ncols), np.uint64)
    figs = [np.zeros(max(1, ncols), np.float64) for _ in range(4)]
    failure = []
    cb = _reduce_hook(allreduce, failure)
    with _hook_failure_first(failure):
        call("gdsp_genome_profile", tab, len(vecs), int(off_lo), noffsets, bin, float(lo), float(hi), cb, None,
             count.ctypes.data_as(C.c_void_p), *[f.ctypes.data_as(C.c_void_p) for f in figs])
    out = {"offsets": np.arange(ncols, dtype=np.int64) * bin + int(off_lo), "count": count[:ncols]}
    for k, f in zip(("sum", "mean", "variance", "stddev"), figs):
        out[k] = f[:ncols]
    with np.errstate(invalid="ignore", divide="ignore"):
        out["stderr"] = out["stddev"] / np.sqrt(out["count"].astype(np.float64))
    return out


def genome_profile_last():
    """What the last genome_profile did: its anchors, the samples taken over all offsets, lane flushes into the device
    images (both passes), and the q that were not finite."""
    out = (C.c_uint64 * 4)()
    lib().gdsp_genome_profile_last(out)
    return dict(zip(("anchors", "samples", "flushes", "nonfinite_squares"), [int(x) for x in out]))


# ------------------------------------------------------- matrixover (not in the reference) ----

MATRIX_FIGURES = {"mean": 0, "sum": 1, "count": 2, "min": 3, "max": 4}       # GDSP_MATRIX_*


def _matrix_figure(what):
    return MATRIX_FIGURES[what] if isinstance(what, str) else int(what)


def _matrix_columns(noffsets, bin):
    return noffsets // bin if bin >= 1 and noffsets >= 1 and noffsets % bin == 0 else 0


def matrix_set_launch_rows(rows):
    """Rows per launch of genome_matrix (0: the library's own number).  For tests that force several launches."""
    call("gdsp_matrix_set_launch_rows", int(rows))


def matrix_rows(vecs, anchors, off_lo, noffsets, bin=1, what="mean", lo=-DBL_MAX, hi=DBL_MAX, stream=None):
    """One gdsp_matrix_rows_batch: (rows, todo).  rows is np.float64[len(anchors), noffsets // bin] as the device left it,
    todo the np.uint32 indices row * ncols + column of the cells it could not finish exactly (in no particular order),
    whose entries of rows mean nothing.  vecs: as xsum_sources, whole chromosomes; anchors: rows (vector index, position,
    strand +1 / -1)."""
    noffsets, bin = int(noffsets), int(bin)
    _, items = _anchor_items(vecs, stream)
    anc, na = _anchor_upload(_profile_anchors(anchors, len(vecs)), stream)
    ncols = _matrix_columns(noffsets, bin)
    cells = na * ncols
    out = DeviceBuffer(max(1, cells) * 8)
    todo = DeviceBuffer((max(1, cells) + 1) * 4)                        # the counter, then the list
    todo.upload(np.zeros(1, np.uint32), stream=stream)
    call("gdsp_matrix_rows_batch", items, len(vecs), C.c_void_p(anc.ptr), C.c_void_p(anc.ptr + 4 * na), na, int(off_lo),
         noffsets, bin, _matrix_figure(what), float(lo), float(hi), C.c_void_p(out.ptr), C.c_void_p(todo.ptr + 4),
         C.c_void_p(todo.ptr), _sp(stream))
    ntodo = int(todo.download(np.uint32, 1, stream=stream)[0])
    assert ntodo <= cells
    rows = out.download(np.float64, cells, stream=stream).reshape(na, ncols) if cells else np.zeros((na, ncols))
    left = todo.download(np.uint32, 1 + ntodo, stream=stream)[1:].copy()
    return rows, left


def genome_matrix(vecs, anchors, off_lo, noffsets, bin=1, what="mean", lo=-DBL_MAX, hi=DBL_MAX, stream=None):
    """The signal around each anchor (gdsp_genome_matrix): np.float64[len(anchors), noffsets // bin], row i the figure
    `what` ("mean", "sum", "count", "min" or "max") of anchor i over each column of `bin` offsets out of
    off_lo .. off_lo + noffsets - 1, in the anchor's own direction; every value exact and rounded once, NaN where a mean,
    min or max has nothing to look at.  vecs: as xsum_sources, whole chromosomes; anchors: rows (vector index, position,
    strand +1 / -1), and the rows come back in their order."""
    noffsets, bin = int(noffsets), int(bin)
    a = _profile_anchors(anchors, len(vecs))
    ncols = _matrix_columns(noffsets, bin)
    tab, keep = _anchor_sources(xsum_sources(vecs, stream), a, stream, with_rows=ncols)
    rows = (C.c_void_p * len(keep))(*[mine.ctypes.data for _, _, _, mine in keep])
    call("gdsp_genome_matrix", tab, len(vecs), int(off_lo), noffsets, bin, _matrix_figure(what), float(lo), float(hi), rows)
    out = np.zeros((a.shape[0], ncols), np.float64)
    for where, pos, _, mine in keep:
        out[where] = mine[:pos.size, :ncols]
    return out


def genome_matrix_last():
    """What the last genome_matrix did: its rows, its cells, the cells the host finished, and the launches."""
    out = (C.c_uint64 * 4)()
    lib().gdsp_genome_matrix_last(out)
    return dict(zip(("rows", "cells", "host cells", "launches"), [int(x) for x in out]))


# ------------------------------------------------------ regionsover (not in the reference) ----

REGIONS_MAX_COLUMNS = 16384


class RegionSource(C.Structure):
    """gdsp_region_source of include/genodsp_hip.h"""
    _fields_ = [("d_v", C.c_void_p), ("n", C.c_uint32), ("device", C.c_int), ("stream", C.c_void_p),
                ("h_start", C.c_void_p), ("h_end", C.c_void_p), ("h_minus", C.c_void_p), ("nregions", C.c_uint32)]


def _regions_array(regions, nvecs):
    """regions: rows (vector index, start, end, strand +1 / -1), zero-based half-open -> int64[count, 4]"""
    a = np.asarray(regions, dtype=np.int64).reshape(-1, 4)
    assert np.all((a[:, 0] >= 0) & (a[:, 0] <= 0x7FFFFFFF)) and np.all((a[:, 1:3] >= 0) & (a[:, 1:3] <= 0xFFFFFFFF))
    assert np.all(np.abs(a[:, 3]) == 1)
    return a


def _regions_columns(body, upstream, downstream, bin):
    ok = bin >= 1 and body >= 1 and upstream >= 0 and downstream >= 0 and upstream % bin == 0 and downstream % bin == 0
    return upstream // bin + body + downstream // bin if ok else 0


def region_cell_bounds(n, start, end, strand, body, upstream=0, downstream=0, bin=1, column=0):
    """Host, no GPU: (lo, hi), the bases [lo, hi) of one column of the row of region [start, end) on a chromosome of n
    bases, cut to [0, n) (lo >= hi: an empty cell) -- gdsp_region_cell_bounds, the function the kernel itself uses."""
    lo, hi = C.c_int64(), C.c_int64()
    call("gdsp_region_cell_bounds", int(n), int(start), int(end), 1 if strand < 0 else 0, int(body), int(upstream),
         int(downstream), int(bin), int(column), C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def regions_set_launch_rows(rows):
    """Rows per launch of genome_regions (0: the library's own number).  For tests that force several launches."""
    call("gdsp_regions_set_launch_rows", int(rows))


def regions_rows(vecs, regions, body, upstream=0, downstream=0, bin=1, what="mean", lo=-DBL_MAX, hi=DBL_MAX, stream=None):
    """One gdsp_region_rows_batch: (rows, todo).  rows is np.float64[len(regions), ncols] as the device left it, todo the
    np.uint32 indices row * ncols + column of the cells it could not finish exactly (in no particular order), whose
    entries of rows mean nothing.  vecs: as xsum_sources, whole chromosomes; regions: rows (vector index, start, end,
    strand +1 / -1)."""
    body, upstream, downstream, bin = int(body), int(upstream), int(downstream), int(bin)
    _, items = _anchor_items(vecs, stream)
    a = _regions_array(regions, len(vecs))
    na = len(a)
    reg = DeviceBuffer(max(1, 3 * na) * 4)                              # the starts, the ends, the code words
    if na:
        reg.upload(np.concatenate([a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32),
                                   (a[:, 0] * 2 + (a[:, 3] < 0)).astype(np.uint32)]), stream=stream)
    ncols = _regions_columns(body, upstream, downstream, bin)
    cells = na * ncols
    out = DeviceBuffer(max(1, cells) * 8)
    todo = DeviceBuffer((max(1, cells) + 1) * 4)                        # the counter, then the list
    todo.upload(np.zeros(1, np.uint32), stream=stream)
    call("gdsp_region_rows_batch", items, len(vecs), C.c_void_p(reg.ptr), C.c_void_p(reg.ptr + 4 * na),
         C.c_void_p(reg.ptr + 8 * na), na, body, upstream, downstream, bin, _matrix_figure(what), float(lo), float(hi),
         C.c_void_p(out.ptr), C.c_void_p(todo.ptr + 4), C.c_void_p(todo.ptr), _sp(stream))
    ntodo = int(todo.download(np.uint32, 1, stream=stream)[0])
    assert ntodo <= cells
    rows = out.download(np.float64, cells, stream=stream).reshape(na, ncols) if cells else np.zeros((na, ncols))
    left = todo.download(np.uint32, 1 + ntodo, stream=stream)[1:].copy()
    return rows, left


def genome_regions(vecs, regions, body, upstream=0, downstream=0, bin=1, what="mean", lo=-DBL_MAX, hi=DBL_MAX, stream=None):
    """Every region scaled to the same columns (gdsp_genome_regions): np.float64[len(regions), upstream // bin + body +
    downstream // bin], row i the figure `what` ("mean", "sum", "count", "min" or "max") of region i over its upstream
    flank in columns of `bin` bases, its own bases in `body` columns, and its downstream flank, in the region's own
    direction; every value exact and rounded once, NaN where a mean, min or max has nothing to look at.  vecs: as
    xsum_sources, whole chromosomes; regions: rows (vector index, start, end, strand +1 / -1), zero-based half-open, and
    the rows come back in their order."""
    body, upstream, downstream, bin = int(body), int(upstream), int(downstream), int(bin)
    a = _regions_array(regions, len(vecs))
    ncols = _regions_columns(body, upstream, downstream, bin)
    src = xsum_sources(vecs, stream)
    tab = (RegionSource * max(1, len(vecs)))()
    keep = []
    for i in range(len(vecs)):
        where = np.flatnonzero(a[:, 0] == i)
        start = np.ascontiguousarray(a[where, 1], dtype=np.uint32)
        end = np.ascontiguousarray(a[where, 2], dtype=np.uint32)
        minus = np.ascontiguousarray(a[where, 3] < 0, dtype=np.uint32)
        mine = np.zeros((max(1, where.size), max(1, ncols)), np.float64)
        keep.append((where, start, end, minus, mine))
        tab[i].d_v, tab[i].n, tab[i].device, tab[i].stream = src[i].d_v, src[i].n, src[i].device, stream
        tab[i].h_start, tab[i].h_end, tab[i].h_minus, tab[i].nregions = start.ctypes.data, end.ctypes.data, minus.ctypes.data, where.size
    if len(a) and not np.all(a[:, 0] < len(vecs)):
        raise GdspError("genome_regions: a region names a vector the call does not have")
    rows = (C.c_void_p * max(1, len(keep)))(*[k[4].ctypes.data for k in keep])
    call("gdsp_genome_regions", tab, len(vecs), body, upstream, downstream, bin, _matrix_figure(what), float(lo), float(hi), rows)
    out = np.zeros((a.shape[0], ncols), np.float64)
    for where, _, _, _, mine in keep:
        out[where] = mine[:where.size, :ncols]
    return out


def genome_regions_last():
    """What the last genome_regions did: its rows, its cells, the cells the host finished, and the launches."""
    out = (C.c_uint64 * 4)()
    lib().gdsp_genome_regions_last(out)
    return dict(zip(("rows", "cells", "host cells", "launches"), [int(x) for x in out]))


# ------------------------------------------------------ histogram (not in the reference) ----

HISTOGRAM_MAX_BINS = 65536


def histogram_uniform_edges(lo=0.0, width=1.0, bins=256):
    """Host, no GPU: the uniform table e[k] = fma(k, width, lo), k = 0 .. bins, each edge rounded once
    (gdsp_histogram_uniform_edges).  ValueError for a table that is not strictly increasing and finite."""
    bins = int(bins)
    if not 1 <= bins <= HISTOGRAM_MAX_BINS:
        raise ValueError("bins must be 1 .. %d" % HISTOGRAM_MAX_BINS)
    e = np.empty(bins + 1, np.float64)
    if lib().gdsp_histogram_uniform_edges(float(lo), float(width), bins, e.ctypes.data_as(C.c_void_p)) != 0:
        raise ValueError("lo=%r width=%r bins=%d is not a strictly increasing finite table" % (lo, width, bins))
    return e


def _histogram_table(edges, lo, width, bins):
    """-> (np.float64 table, its number of bins, the uniform hint); ValueError for a table the library would refuse"""
    if edges is None:
        return histogram_uniform_edges(lo, width, bins), int(bins), 1
    e = np.ascontiguousarray(edges, dtype=np.float64)
    if e.ndim != 1 or not 2 <= e.size <= HISTOGRAM_MAX_BINS + 1:
        raise ValueError("edges must be a vector of 2 .. %d values" % (HISTOGRAM_MAX_BINS + 1))
    if not (np.all(np.isfinite(e)) and np.all(e[:-1] < e[1:])):
        raise ValueError("edges must be finite and strictly increasing")
    return e, e.size - 1, 0


def histogram_accumulate(vecs, counts, edges, window=1, lo=-DBL_MAX, hi=DBL_MAX, uniform=False, stream=None):
    """Add the sample of vecs (as xsum_sources) to `counts`, a DeviceBuffer of len(edges) + 2 u64 words
    (gdsp_histogram_accumulate_batch; zero it with gdsp_histogram_init).  uniform: the hint that edges are evenly spaced."""
    e, nbins, _ = _histogram_table(edges, 0.0, 1.0, 1)
    assert counts.nbytes >= (nbins + 3) * 8
    src = xsum_sources(vecs, stream)
    call("gdsp_histogram_accumulate_batch", src, len(vecs), int(window), float(lo), float(hi),
         e.ctypes.data_as(C.c_void_p), nbins, 1 if uniform else 0, C.c_void_p(counts.ptr), _sp(stream))


def histogram_words(vecs, edges, window=1, lo=-DBL_MAX, hi=DBL_MAX, uniform=False, stream=None):
    """The len(edges) + 2 words of one accumulate over vecs, as np.uint64: bins, below, above, n."""
    e, nbins, _ = _histogram_table(edges, 0.0, 1.0, 1)
    acc = DeviceBuffer((nbins + 3) * 8)
    call("gdsp_histogram_init", C.c_void_p(acc.ptr), nbins, _sp(stream))
    histogram_accumulate(vecs, acc, e, window, lo, hi, uniform, stream)
    return acc.download(np.uint64, nbins + 3, stream=stream)


def genome_histogram(vecs, edges=None, lo=0.0, width=1.0, bins=256, window=1, min=-DBL_MAX, max=DBL_MAX, allreduce=None,
                     stream=None, uniform=None):
    """(counts, below, above, n) of the sampled genome (gdsp_genome_histogram): counts[k] values v with
    e[k] <= v < e[k+1], below those under e[0], above those at or over e[-1], n all of them.  The table is `edges`, or
    the uniform one of histogram_uniform_edges(lo, width, bins).  The sample is genome_stats': every window-th value
    counted from each chromosome's first base with min <= v <= max (never NaN or +-inf).  vecs: as xsum_sources.
    allreduce(np.uint64 array, "sum") -> the array summed over ranks (None: one rank).  uniform: force the hint on or off
    (None: on for a uniform table, off for `edges`); the words do not depend on it."""
    e, nbins, hint = _histogram_table(edges, lo, width, bins)
    if uniform is not None:
        hint = 1 if uniform else 0
    src = xsum_sources(vecs, stream)
    out = np.zeros(nbins + 3, np.uint64)
    failure = []
    cb = _reduce_hook(allreduce, failure)
    with _hook_failure_first(failure):
        call("gdsp_genome_histogram", src, len(vecs), int(window), float(min), float(max), e.ctypes.data_as(C.c_void_p),
             nbins, hint, cb, None, out.ctypes.data_as(C.c_void_p))
    return out[:nbins].copy(), int(out[nbins]), int(out[nbins + 1]), int(out[nbins + 2])


# ------------------------------------------------------ statsover (not in the reference) ----

INTERVAL_STAT = np.dtype([("count", np.uint64), ("sum", np.float64), ("mean", np.float64), ("min", np.float64),
                          ("max", np.float64), ("maxpos", np.uint32), ("image", np.uint32)])       # gdsp_interval_stat
INTERVAL_PIECE = np.dtype([("a0", np.float64), ("a1", np.float64), ("min", np.float64), ("max", np.float64),
                           ("count", np.uint32), ("maxpos", np.uint32), ("flag", np.uint32), ("reserved", np.uint32)])   # gdsp_interval_piece


def interval_stats_tile():
    """The tile the kernel cuts intervals at (values of the 16-byte aligned frame a vector lies in)."""
    return int(lib().gdsp_interval_stats_tile())


def _interval_figures(rec):
    none = rec["count"] == 0
    maxpos = rec["maxpos"].astype(np.int64)
    maxpos[none] = -1
    return {"count": rec["count"].copy(), "sum": rec["sum"].copy(), "mean": rec["mean"].copy(), "min": rec["min"].copy(),
            "max": rec["max"].copy(), "maxpos": maxpos}


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _interval_call(v, start, end, vec):
    """interval_stats, interval_percentiles and interval_breadth open with it -> items, vectors, vec or None, start, end"""
    vecs = v if isinstance(v, list) else [v]
    items = _read_only_items(vecs)
    start = np.ascontiguousarray(start, dtype=np.uint32)
    end = np.ascontiguousarray(end, dtype=np.uint32)
    assert start.shape == end.shape and start.ndim == 1
    which = None if vec is None else np.ascontiguousarray(vec, dtype=np.uint32)
    assert which is None or which.shape == start.shape
    return items, len(vecs), which, start, end


def interval_stats_set_launch_pieces(pieces=0):
    """The most pieces of one launch; 0: the default.  For tests."""
    call("gdsp_interval_stats_set_launch_pieces", int(pieces))


def interval_stats(v, start, end, lo=-DBL_MAX, hi=DBL_MAX, stream=None, vec=None):
    """count, sum, mean, min, max and maxpos of v over the intervals [start[i], end[i]) (gdsp_interval_stats: stats'
    sample inside each interval, every figure exact and rounded once; NaN / -1 where the sample is empty).  -> dict of
    numpy arrays in the caller's order.  v: a DeviceVector or a (vector, first, count) stretch of one; or a LIST of
    them with vec[i] naming interval i's vector (gdsp_interval_stats_batch: one launch for all of them).  Waits."""
    items, nvec, which, start, end = _interval_call(v, start, end, vec)
    rec = np.zeros(start.size, INTERVAL_STAT)
    call("gdsp_interval_stats_batch", items, nvec, _vp(which), _vp(start), _vp(end), start.size, float(lo), float(hi),
         _vp(rec), _sp(stream))
    return _interval_figures(rec)


def interval_stats_combine(pieces, images=None):
    """Host, no GPU: an interval's figures from its pieces' records (np array of INTERVAL_PIECE; images: one
    XSUM_WORDS image per flagged piece, in order).  -> dict of scalars, as interval_stats gives arrays."""
    pieces = np.ascontiguousarray(pieces, dtype=INTERVAL_PIECE)
    img = None if images is None else np.ascontiguousarray(images, dtype=np.uint64)
    rec = np.zeros(1, INTERVAL_STAT)
    call("gdsp_interval_stats_combine", pieces.ctypes.data_as(C.c_void_p), pieces.size,
         None if img is None else img.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p))
    out = {k: a[0] for k, a in _interval_figures(rec).items()}
    out["image"] = int(rec["image"][0])
    return out


def interval_stats_last():
    """What the last interval_stats did: intervals, pieces, flagged pieces (summed again through the exact pass),
    intervals rounded from the integer image; and ms spent cutting, in the kernel, copying and waiting, combining."""
    out, ms = (C.c_uint64 * 4)(), (C.c_double * 4)()
    lib().gdsp_interval_stats_last(out)
    lib().gdsp_interval_stats_times(ms)
    d = dict(zip(("intervals", "pieces", "flagged", "imaged"), [int(x) for x in out]))
    d.update(zip(("ms_cut", "ms_kernel", "ms_copy", "ms_combine"), [float(x) for x in ms]))
    return d


# ------------------------------------------ percentilesover / medianover (not in the reference) ----

def interval_percentiles_short():
    """The longest interval the one-read (LDS sort) route takes; results never depend on it."""
    return int(lib().gdsp_interval_percentiles_short())


def interval_percentiles_piece():
    """The piece a longer interval is cut into for the radix select; results never depend on it."""
    return int(lib().gdsp_interval_percentiles_piece())


def interval_percentiles_set_batch(long_queries=0):
    """Long (interval, percentile) queries per batch of the radix select; 0: the default.  For tests."""
    call("gdsp_interval_percentiles_set_batch", int(long_queries))


def interval_percentiles(v, start, end, p_thousandths, lo=-DBL_MAX, hi=DBL_MAX, stream=None, vec=None):
    """The sample's size and, for every percentile of p_thousandths, the exact order statistic of v over the intervals
    [start[i], end[i]) (gdsp_interval_percentiles: statsover's sample, percentile's order and rank rule; NaN where the
    sample is empty).  -> {"count": uint32[n], "values": float64[n, len(p_thousandths)]} in the caller's order.
    v: a DeviceVector or a (vector, first, count) stretch of one; or a LIST of them with vec[i] naming interval i's
    vector (gdsp_interval_percentiles_batch).  Waits."""
    items, nvec, which, start, end = _interval_call(v, start, end, vec)
    pcts = np.ascontiguousarray(np.atleast_1d(p_thousandths), dtype=np.uint32)
    count = np.zeros(start.size, np.uint32)
    values = np.zeros((start.size, max(1, pcts.size)), np.float64)
    call("gdsp_interval_percentiles_batch", items, nvec, _vp(which), _vp(start), _vp(end), start.size, _vp(pcts), pcts.size,
         float(lo), float(hi), _vp(count), _vp(values), _sp(stream))
    return {"count": count, "values": values[:, :pcts.size]}


def interval_percentiles_last():
    """What the last interval_percentiles did: intervals, those of the short and of the long route, histogram passes,
    batches of long queries, long queries that ended before the last digit."""
    out = (C.c_uint64 * 6)()
    lib().gdsp_interval_percentiles_last(out)
    return dict(zip(("intervals", "short", "long", "passes", "batches", "ended_early"), [int(x) for x in out]))


# ------------------------------------------------------ breadthover (not in the reference) ----

def interval_breadth_tile():
    """The tile the kernel cuts intervals at (values of the 16-byte aligned frame a vector lies in)."""
    return int(lib().gdsp_interval_breadth_tile())


def interval_breadth_set_launch_pieces(pieces=0):
    """The most pieces of one launch; 0: the default.  For tests."""
    call("gdsp_interval_breadth_set_launch_pieces", int(pieces))


def interval_breadth(v, start, end, thresholds, strict=False, lo=-DBL_MAX, hi=DBL_MAX, stream=None, vec=None):
    """The sample's size and, for every threshold T, the number of sampled bases with v >= T (v > T when strict) over the
    intervals [start[i], end[i]) (gdsp_interval_breadth: statsover's sample, IEEE comparisons, integers throughout).
    -> {"count": uint32[n], "atleast": uint32[n, len(thresholds)]} in the caller's order.  v: a DeviceVector or a
    (vector, first, count) stretch of one; or a LIST of them with vec[i] naming interval i's vector
    (gdsp_interval_breadth_batch).  Waits."""
    items, nvec, which, start, end = _interval_call(v, start, end, vec)
    ts = np.ascontiguousarray(np.atleast_1d(thresholds), dtype=np.float64)
    count = np.zeros(start.size, np.uint32)
    atleast = np.zeros((start.size, max(1, ts.size)), np.uint32)
    call("gdsp_interval_breadth_batch", items, nvec, _vp(which), _vp(start), _vp(end), start.size, _vp(ts), ts.size,
         1 if strict else 0, float(lo), float(hi), _vp(count), _vp(atleast), _sp(stream))
    return {"count": count, "atleast": atleast[:, :ts.size]}


def interval_breadth_last():
    """What the last interval_breadth did: intervals, pieces, launches, workgroups."""
    out = (C.c_uint64 * 4)()
    lib().gdsp_interval_breadth_last(out)
    return dict(zip(("intervals", "pieces", "launches", "workgroups"), [int(x) for x in out]))


def interval_breadth_times():
    """Where the last interval_breadth's time went, in ms: cutting, the kernel (HIP events), copies and waiting, combining."""
    ms = (C.c_double * 4)()
    lib().gdsp_interval_breadth_times(ms)
    return dict(zip(("ms_cut", "ms_kernel", "ms_copy", "ms_combine"), [float(x) for x in ms]))


# ---------------------------------------------------- correlateover (not in the reference) ----

INTERVAL_CORR = np.dtype([("count", np.uint32), ("reserved", np.uint32), ("mean", np.float64), ("filemean", np.float64),
                          ("stddev", np.float64), ("filestddev", np.float64), ("covariance", np.float64),
                          ("correlation", np.float64), ("slope", np.float64), ("intercept", np.float64)])   # gdsp_interval_corr
INTERVAL_CORR_FIGURES = ("count", "mean", "filemean", "stddev", "filestddev", "covariance", "correlation", "slope", "intercept")


def interval_correlation_tile():
    """The tile the kernel cuts intervals at (values of the 16-byte aligned frame the signal lies in)."""
    return int(lib().gdsp_interval_correlation_tile())


def interval_correlation_set_launch_pieces(pieces=0):
    """The most pieces of one launch; 0: the default.  For tests."""
    call("gdsp_interval_correlation_set_launch_pieces", int(pieces))


def interval_correlation(x, y, start, end, lo=-DBL_MAX, hi=DBL_MAX, ylo=-DBL_MAX, yhi=DBL_MAX, stream=None, vec=None):
    """correlate's figures of x against y over the intervals [start[i], end[i]) (gdsp_interval_correlation: the pair sample
    inside each interval, lo <= x <= hi and ylo <= y <= yhi, never NaN or +-inf; every figure exact and rounded once or
    derived from such; NaN where it is not defined).  -> dict of numpy arrays (INTERVAL_CORR_FIGURES) in the caller's
    order.  x, y: a DeviceVector each, or a (vector, first, count) stretch of one; or LISTS of them of the same lengths
    with vec[i] naming interval i's pair (gdsp_interval_correlation_batch).  Neither is written.  Waits."""
    items, nvec, which, start, end = _interval_call(x, start, end, vec)
    tracks = _read_only_items(y if isinstance(y, list) else [y])
    assert nvec == (len(y) if isinstance(y, list) else 1)
    for k in range(nvec):
        assert items[k].n == tracks[k].n, "a track must be as long as its signal"
        items[k].d_out = tracks[k].d_in
    rec = np.zeros(start.size, INTERVAL_CORR)
    call("gdsp_interval_correlation_batch", items, nvec, _vp(which), _vp(start), _vp(end), start.size, float(lo), float(hi),
         float(ylo), float(yhi), _vp(rec), _sp(stream))
    return {k: rec[k].copy() for k in INTERVAL_CORR_FIGURES}


def interval_correlation_last():
    """What the last interval_correlation did: intervals, pieces, and the pieces summed again through correlate's exact
    pass after pass 1 and after pass 2."""
    out = (C.c_uint64 * 4)()
    lib().gdsp_interval_correlation_last(out)
    return dict(zip(("intervals", "pieces", "flagged1", "flagged2"), [int(x) for x in out]))


def interval_correlation_times():
    """Where the last interval_correlation's time went, in ms: cutting, the kernels of both passes (HIP events), copies,
    waiting and second sums, the means and combining."""
    ms = (C.c_double * 4)()
    lib().gdsp_interval_correlation_times(ms)
    return dict(zip(("ms_cut", "ms_kernel", "ms_copy", "ms_combine"), [float(x) for x in ms]))


# ------------------------------------------------------- segments (not in the reference) ----

RUN_PIECE = np.dtype([("vec", np.uint32), ("start", np.uint32), ("end", np.uint32), ("reserved", np.uint32),
                      ("piece", INTERVAL_PIECE)])                                                   # gdsp_run_piece
SEGMENT = np.dtype([("vec", np.uint32), ("start", np.uint32), ("end", np.uint32), ("reserved", np.uint32),
                    ("stat", INTERVAL_STAT)])                                                       # gdsp_segment
RUN_PIECES_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p)
SEGMENTS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint32)


def segments_tile():
    """The tile the piece kernel cuts runs at (values of the 16-byte aligned frame a vector lies in)."""
    return int(lib().gdsp_segments_tile())


def _read_only_items(vecs):
    items = (BatchItem * max(1, len(vecs)))()
    for k, item in enumerate(vecs):
        if isinstance(item, DeviceVector):
            items[k].d_in, items[k].n = item.ptr.value, item.n
        else:                                                       # a (vector, first, count) stretch of one
            assert 0 <= int(item[1]) and int(item[1]) + int(item[2]) <= item[0].n
            items[k].d_in, items[k].n = item[0].ptr.value + 8 * int(item[1]), int(item[2])
    return items


def _copy_records(ptr, count, dtype):
    if count == 0:
        return np.zeros(0, dtype)
    return np.frombuffer(C.string_at(ptr, count * dtype.itemsize), dtype=dtype).copy()


def _segment_collector(out, failure):
    def take(_ctx, segs, count):
        try:
            out.append(_copy_records(segs, count, SEGMENT))
            return 0
        except Exception as e:
            failure.append(e)
            return 1
    return SEGMENTS_FN(take)


def _segment_arrays(chunks):
    rec = np.concatenate(chunks) if chunks else np.zeros(0, SEGMENT)
    out = {"vec": rec["vec"].copy(), "start": rec["start"].copy(), "end": rec["end"].copy()}
    out.update(_interval_figures(rec["stat"]))
    return out


def run_pieces(vecs, T, ties_above=False, stream=None):
    """The device half of segments (gdsp_run_pieces_batch): every maximal stretch of members (v > T, or v >= T with
    ties_above) inside a tile of every vector, in (vector, position) order.  -> [(records, images), ...], one pair per
    call the library made: records an array of RUN_PIECE, images (flagged pieces, XSUM_WORDS) uint64 or None.  Waits."""
    vecs = vecs if isinstance(vecs, list) else [vecs]
    items = _read_only_items(vecs)
    chunks, failure = [], []

    def take(_ctx, recs, count, images):
        try:
            r = _copy_records(recs, count, RUN_PIECE)
            nflag = int(np.count_nonzero(r["piece"]["flag"]))
            img = None
            if nflag:
                img = np.frombuffer(C.string_at(images, nflag * XSUM_WORDS * 8), dtype=np.uint64).reshape(nflag, XSUM_WORDS).copy()
            chunks.append((r, img))
            return 0
        except Exception as e:
            failure.append(e)
            return 1

    cb = RUN_PIECES_FN(take)
    with _hook_failure_first(failure):
        call("gdsp_run_pieces_batch", items, len(vecs), float(T), 1 if ties_above else 0, cb, None, _sp(stream))
    return chunks


def segments_from_pieces(chunks, merge_gap=0, min_length=1, min_height=None):
    """The host half of segments, no GPU (gdsp_segments_feed / gdsp_segments_finish): chunks is a list of (records,
    images) pairs as run_pieces gives them, each fed on its own.  -> (dict of arrays: vec, start, end, count, sum, mean,
    min, max, maxpos; dict of counts: runs, pieces, flagged, kept)."""
    out, failure = [], []
    cb = _segment_collector(out, failure)
    b = C.c_void_p()
    call("gdsp_segments_create", C.byref(b), int(merge_gap), int(min_length), 0 if min_height is None else 1,
         0.0 if min_height is None else float(min_height), cb, None)
    try:
        with _hook_failure_first(failure):
            for recs, images in chunks:
                recs = np.ascontiguousarray(recs, dtype=RUN_PIECE)
                img = None if images is None else np.ascontiguousarray(images, dtype=np.uint64)
                call("gdsp_segments_feed", b, recs.ctypes.data_as(C.c_void_p), recs.size,
                     None if img is None else img.ctypes.data_as(C.c_void_p))
            call("gdsp_segments_finish", b)
        counts = (C.c_uint64 * 4)()
        lib().gdsp_segments_counts(b, counts)
    finally:
        lib().gdsp_segments_destroy(b)
    return _segment_arrays(out), dict(zip(("runs", "pieces", "flagged", "kept"), [int(x) for x in counts]))


def segments(vecs, T, ties_above=False, merge_gap=0, min_length=1, min_height=None, stream=None):
    """The thresholded regions of the vectors with statsover's figures (gdsp_segments_batch): runs of members joined
    across gaps of at most merge_gap bases, those shorter than min_length or (with min_height) lower than it dropped.
    -> dict of numpy arrays: vec, start, end, count, sum, mean, min, max, maxpos (-1 where the sample is empty), in
    (vector, position) order.  The vectors are only read.  Waits."""
    vecs = vecs if isinstance(vecs, list) else [vecs]
    items = _read_only_items(vecs)
    out, failure = [], []
    cb = _segment_collector(out, failure)
    with _hook_failure_first(failure):
        call("gdsp_segments_batch", items, len(vecs), float(T), 1 if ties_above else 0, int(merge_gap), int(min_length),
             0 if min_height is None else 1, 0.0 if min_height is None else float(min_height), cb, None, _sp(stream))
    return _segment_arrays(out)


def segments_last():
    """What the last segments call did: runs, pieces, flagged pieces (summed again), kept segments; and ms spent in the
    counting pass, in the piece kernel, copying and waiting, consuming the pieces."""
    out, ms = (C.c_uint64 * 4)(), (C.c_double * 4)()
    lib().gdsp_segments_last(out)
    lib().gdsp_segments_times(ms)
    d = dict(zip(("runs", "pieces", "flagged", "kept"), [int(x) for x in out]))
    d.update(zip(("ms_count", "ms_kernel", "ms_copy", "ms_consume"), [float(x) for x in ms]))
    return d


# --------------------------------------------------- keepsegments (not in the reference) ----

PAINT_SPAN = np.dtype([("vec", np.uint32), ("start", np.uint32), ("end", np.uint32), ("reserved", np.uint32),
                       ("value", np.float64)])                                                      # gdsp_paint_span
KEEP_MODES = ("one", "value", "count", "length", "sum", "mean", "min", "max")                       # GDSP_KEEP_*


def paint_tile():
    """The tile the paint kernel cuts an output at (values of the 16-byte aligned frame it lies in)."""
    return int(lib().gdsp_paint_tile())


def _in_out_items(vecs, outs):
    """vecs (None: nothing is read), outs: DeviceVectors or (vector, first, count) stretches, pairwise of equal length"""
    items = _read_only_items(outs)
    for k in range(len(outs)):
        items[k].d_out, items[k].d_in = items[k].d_in, None
    if vecs is not None:
        assert len(vecs) == len(outs)
        ins = _read_only_items(vecs)
        for k in range(len(outs)):
            assert ins[k].n == items[k].n
            items[k].d_in = ins[k].d_in
    return items


def paint_spans(vecs, outs, spans, mode="figure", outside=0.0, start=(0, 0), stop=None, stream=None):
    """Paint disjoint spans into the outputs (gdsp_paint_spans_batch).  spans: (vec, start, end, value) rows in
    (vector, position) order, or an array of PAINT_SPAN.  Every base from `start` = (vector, position) up to `stop`
    (None: the end of the last vector) is written once: the span's value inside a span -- with mode "value" the base of
    vecs itself -- and `outside` elsewhere.  vecs may be None unless mode is "value".  -> dict: bases painted inside and
    outside, ms in the launches and around them.  Waits."""
    outs = outs if isinstance(outs, list) else [outs]
    vecs = vecs if (vecs is None or isinstance(vecs, list)) else [vecs]
    assert mode in ("figure", "value")
    items = _in_out_items(vecs, outs)
    if isinstance(spans, np.ndarray) and spans.dtype == PAINT_SPAN:
        rec = np.ascontiguousarray(spans)
    else:
        rec = np.zeros(len(spans), PAINT_SPAN)
        for k, (v, s, e, x) in enumerate(spans):
            rec[k] = (v, s, e, 0, x)
    stop = (len(outs), 0) if stop is None else stop
    call("gdsp_paint_spans_batch", items, len(outs), rec.ctypes.data_as(C.c_void_p), rec.size, 1 if mode == "value" else 0,
         float(outside), int(start[0]), int(start[1]), int(stop[0]), int(stop[1]), _sp(stream))
    painted, ms = (C.c_uint64 * 2)(), (C.c_double * 2)()
    lib().gdsp_paint_spans_last(painted, ms)
    return {"inside": int(painted[0]), "outside": int(painted[1]), "ms_paint": float(ms[0]), "ms_around": float(ms[1])}


def keep_segments(vecs, outs, T, ties_above=False, merge_gap=0, min_length=1, min_height=None, as_="one", one=1.0, zero=0.0,
                  stream=None):
    """The kept segments of segments(vecs, T, ...) written into outs (gdsp_keep_segments_batch): `zero` outside every
    kept segment; inside one -- its whole span, joined gaps included -- by as_: `one`, the signal's own "value", or the
    segment's "count", "length", "sum", "mean", "min" or "max".  outs are other buffers than vecs, which are only read.
    -> the dict of arrays segments() returns.  Waits."""
    vecs = vecs if isinstance(vecs, list) else [vecs]
    outs = outs if isinstance(outs, list) else [outs]
    items = _in_out_items(vecs, outs)
    out, failure = [], []
    cb = _segment_collector(out, failure)
    with _hook_failure_first(failure):
        call("gdsp_keep_segments_batch", items, len(vecs), float(T), 1 if ties_above else 0, int(merge_gap), int(min_length),
             0 if min_height is None else 1, 0.0 if min_height is None else float(min_height), KEEP_MODES.index(as_),
             float(one), float(zero), cb, None, _sp(stream))
    return _segment_arrays(out)


def keep_segments_last():
    """What the last keep_segments did: segments_last's counts, the bases painted inside and outside kept segments, and
    ms spent in the paint launches and around them."""
    out, ms = (C.c_uint64 * 6)(), (C.c_double * 2)()
    lib().gdsp_keep_segments_last(out)
    lib().gdsp_keep_segments_times(ms)
    d = dict(zip(("runs", "pieces", "flagged", "kept", "inside", "outside"), [int(x) for x in out]))
    d.update(zip(("ms_paint", "ms_around"), [float(x) for x in ms]))
    return d


def _each(name, vecs, *params, stream=None):
    if isinstance(vecs, DeviceVector):
        call(name, vecs.ptr, vecs.n, *params, _sp(stream))
        return vecs
    return _batch(name + "_batch", vecs, None, *params, stream=stream, in_place=True)


def multiply_constant(vecs, c, stream=None):
    """v = fl(v * c) in place, for one DeviceVector or a list of them (one launch per 32)."""
    return _each("gdsp_multiply_constant", vecs, float(c), stream=stream)


def divide_constant(vecs, c, stream=None):
    """v = fl(v / c) in place; c == 0 is refused."""
    return _each("gdsp_divide_constant", vecs, float(c), stream=stream)


def standardize(vecs, center, scale, stream=None):
    """v = fl(fl(v - center) / scale) in place; scale == 0 is refused."""
    return _each("gdsp_standardize", vecs, float(center), float(scale), stream=stream)


def normalize(vecs, to="mean", window=1, lo=-DBL_MAX, hi=DBL_MAX, allreduce=None, stream=None):
    """The driver's `normalize`: the genome's figures (genome_stats over the sample), then every base of every vector
    rewritten -- to="mean": fl(v / mean); to="zscore": fl(fl(v - mean) / stddev).  Refused (ValueError, nothing
    written) when the sample is empty or the divisor is 0 or not finite.  vecs: DeviceVectors.  Returns the figures."""
    if to not in ("mean", "zscore"):
        raise ValueError("normalize: unknown --to=%s (mean or zscore)" % to)
    st = genome_stats(vecs, window, lo, hi, allreduce, stream)
    if st["count"] == 0:
        raise ValueError("normalize: no values meet the criteria")
    div = st["mean"] if to == "mean" else st["stddev"]
    if not (div != 0 and abs(div) <= DBL_MAX):
        raise ValueError("normalize: the %s is %r" % ("mean" if to == "mean" else "standard deviation", div))
    if to == "mean":
        divide_constant(list(vecs), div, stream=stream)
    else:
        standardize(list(vecs), st["mean"], div, stream=stream)
    return st


class Comm:
    """RCCL communicator over devices of this process (gdsp_comm_create: ncclCommInitAll)."""

    def __init__(self, devices):
        h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices)
        call("gdsp_comm_create", C.byref(h), arr, len(devices))
        self.handle = h.value
        self.devices = list(devices)

    def allreduce(self, bufs, count, op, dtype="u64", streams=None):
        """bufs: one device address per rank, reduced in place; op 'sum' | 'min' | 'max'."""
        ptrs = (C.c_void_p * len(bufs))(*bufs)
        st = (C.c_void_p * len(bufs))(*(streams or [None] * len(bufs)))
        call("gdsp_comm_allreduce_" + dtype, C.c_void_p(self.handle), ptrs, int(count), ("sum", "min", "max").index(op), st)

    def close(self):
        if self.handle:
            call("gdsp_comm_destroy", C.c_void_p(self.handle))
            self.handle = None


def rccl_version():
    v = C.c_int(0)
    call("gdsp_comm_rccl_version", C.byref(v))
    return v.value


def percentile_stats():
    """What the last percentile() did: route (SELECT_RADIX / SELECT_BRACKET), population, subsample size,
    candidates kept on this rank, percentiles that fell back, histogram passes over the population, whether a fused
    binarize was settled in the counting pass, whether the call was decided on the device (one read-back)."""
    out = (C.c_uint64 * 8)()
    lib().gdsp_percentiles_stats(out)
    keys = ("route", "population", "sample", "candidates", "fallbacks", "population_passes", "binarize_in_one_pass", "resident")
    return dict(zip(keys, [int(x) for x in out]))


class PercentileBinarize(C.Structure):
    _fields_ = [("which", C.c_int), ("tiesAbove", C.c_int), ("one", C.c_double), ("zero", C.c_double), ("d_out", C.c_void_p)]


def percentile_binarize(vecs, p_thousandths, which=0, outs=None, ties_above=False, one=1.0, zero=0.0, window=1, lo=-DBL_MAX,
                        hi=DBL_MAX, stream=None, strategy=SELECT_AUTO, sample_target=0, device_allreduce=None):
    """`= percentile P = binarize --threshold=percentileP` in one read of the signal (gdsp_percentiles_binarize):
    -> (count, [values], outs, one_pass); outs[i] = binarize(vecs[i], values[which]), the vectors are left intact."""
    device = current_device()
    outs = outs if outs is not None else [v.like() for v in vecs]
    src = (SelectSource * max(1, len(vecs)))()
    for i, v in enumerate(vecs):
        src[i].d_v, src[i].n, src[i].device, src[i].stream = v.ptr, v.n, device, stream
    optrs = (C.c_void_p * max(1, len(vecs)))(*[o.ptr.value for o in outs])
    fuse = PercentileBinarize(int(which), int(ties_above), float(one), float(zero), C.cast(optrs, C.c_void_p))
    pts = (C.c_uint32 * len(p_thousandths))(*[int(p) for p in p_thousandths])
    vals = (C.c_double * len(p_thousandths))()
    count, one_pass = C.c_uint64(0), C.c_int(0)
    failure = []

    def device_reduce(_ctx, d_words, n, op, s):
        try:
            device_allreduce(d_words, n, ("sum", "min", "max")[op], s)
            return 0
        except Exception as e:
            failure.append(e)
            return 1

    dcb = DEVICE_REDUCE_FN(device_reduce) if device_allreduce is not None else None
    _PERCENTILE_HOOK.acquire()
    try:
        with _hook_failure_first(failure):
            if dcb is not None:
                call("gdsp_percentiles_use_device_reduce", dcb, None)
            call("gdsp_percentiles_binarize", src, len(vecs), int(window), float(lo), float(hi), pts, len(p_thousandths),
                 int(strategy), int(sample_target), C.cast(None, REDUCE_FN), None, vals, C.byref(count), C.byref(fuse), C.byref(one_pass))
    finally:
        if dcb is not None:
            call("gdsp_percentiles_use_device_reduce", None, None)
        _PERCENTILE_HOOK.release()
    if count.value == 0:
        return 0, [], outs, False
    return int(count.value), [float(x) for x in vals], outs, bool(one_pass.value)


def percentile_by_passes(vecs, p_thousandths, window=1, lo=-DBL_MAX, hi=DBL_MAX, allreduce=None, stream=None):
    """The same result through the pass-level entry points (gdsp_select_histogram + host walk), kept for
    callers that drive the passes themselves."""
    def histogram(shift, bits, prefix):
        nb = 1 << bits
        dh = DeviceBuffer((nb + 2) * 8)
        call("gdsp_select_hist_init", C.c_void_p(dh.ptr), bits, _sp(stream))
        for v in vecs:
            call("gdsp_select_histogram", v.ptr, v.n, window, float(lo), float(hi), shift, bits,
                 C.c_uint64(prefix), C.c_void_p(dh.ptr), _sp(stream))
        return dh.download(np.uint64, nb + 2, stream=stream)

    return radix_select(histogram, p_thousandths, allreduce)


def lpt_shards(lengths, nranks):
    """Deal chromosomes longest-first onto the least loaded rank (what genodsp_hip --gpus=N and
    bench.py do); returns a list of chromosome-index lists, one per rank."""
    order = sorted(range(len(lengths)), key=lambda i: -lengths[i])
    load = [0] * nranks
    shards = [[] for _ in range(nranks)]
    for i in order:
        r = min(range(nranks), key=lambda k: load[k])
        shards[r].append(i)
        load[r] += lengths[i]
    return shards


# ------------------------------------- genodsp.c / add.c / multiply.c ------

class BinnedIntervals:
    """Intervals of one chromosome, staged on the device with their tile CSR."""

    def __init__(self, n, start, end, val):
        start = np.ascontiguousarray(start, np.uint32)
        end = np.ascontiguousarray(end, np.uint32)
        val = np.ascontiguousarray(val, np.float64)
        tile = lib().gdsp_interval_tile()
        ntiles = (n + tile - 1) // tile
        offsets = np.zeros(ntiles + 1, np.uint32)
        length = C.c_uint64()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        call("gdsp_bin_intervals", n, vp(start), vp(end), start.size, vp(offsets), None, C.byref(length))
        tlist = np.zeros(max(length.value, 1), np.uint32)
        call("gdsp_bin_intervals", n, vp(start), vp(end), start.size, vp(offsets), vp(tlist), C.byref(length))
        self.n = n
        self.d_start = _dev_array(start, np.uint32)
        self.d_end = _dev_array(end, np.uint32)
        self.d_val = _dev_array(val, np.float64)
        self.d_offsets = _dev_array(offsets, np.uint32)
        self.d_list = _dev_array(tlist, np.uint32)

    def _args(self):
        return [C.c_void_p(b.ptr) for b in (self.d_start, self.d_end, self.d_val, self.d_offsets, self.d_list)]


def apply_intervals(v, start, end, val, overlap=OVERLAP_SUM, clear=False, missing=0.0, stream=None):
    b = BinnedIntervals(v.n, start, end, val)
    call("gdsp_apply_intervals", v.ptr, v.n, *b._args(), overlap, 3 if clear else 0, float(missing), _sp(stream))
    sync(stream)
    return v


def scale_intervals(v, start, end, val, divide=False, infinity=DBL_MAX, stream=None):
    b = BinnedIntervals(v.n, start, end, val)
    call("gdsp_scale_intervals", v.ptr, v.n, *b._args(), int(divide), float(infinity), _sp(stream))
    sync(stream)
    return v


def mask_intervals(v, start, end, val, inside=True, outside_val=0.0, binarize_first=False, stream=None):
    """mask / or (inside=True) and masknot / and (inside=False); see gdsp_mask_intervals."""
    b = BinnedIntervals(v.n, start, end, val)
    call("gdsp_mask_intervals", v.ptr, v.n, *b._args(), int(inside), float(outside_val), int(binarize_first), _sp(stream))
    sync(stream)
    return v


def extreme_in_intervals(v, start, end, want_max, fill, stream=None):
    """minover / maxover over sorted, non-overlapping intervals."""
    b = BinnedIntervals(v.n, start, end, np.ones(len(start)))
    count = len(start)
    work = DeviceBuffer(lib().gdsp_extreme_in_intervals_work(count))
    call("gdsp_extreme_in_intervals", v.ptr, v.n, C.c_void_p(b.d_start.ptr), C.c_void_p(b.d_end.ptr), count,
         C.c_void_p(b.d_offsets.ptr), C.c_void_p(b.d_list.ptr), int(want_max), float(fill), C.c_void_p(work.ptr), _sp(stream))
    sync(stream)
    return v


def report_runs(v, collapse=True, uncovered=0, stream=None):
    """(start, end, value) arrays of the runs report_intervals would print."""
    work = DeviceBuffer(lib().gdsp_report_runs_work(v.n))
    cnt = DeviceBuffer(16)
    call("gdsp_report_runs", v.ptr, v.n, int(collapse), uncovered, None, None, None, 0,
         C.c_void_p(cnt.ptr), C.c_void_p(work.ptr), _sp(stream))
    n = int(cnt.download(np.uint32, 1, stream=stream)[0])
    if n == 0:
        return np.empty(0, np.uint32), np.empty(0, np.uint32), np.empty(0, np.float64)
    s, e, x = DeviceBuffer(n * 4), DeviceBuffer(n * 4), DeviceBuffer(n * 8)
    call("gdsp_report_runs", v.ptr, v.n, int(collapse), uncovered, C.c_void_p(s.ptr), C.c_void_p(e.ptr),
         C.c_void_p(x.ptr), n, C.c_void_p(cnt.ptr), C.c_void_p(work.ptr), _sp(stream))
    return (s.download(np.uint32, n, stream=stream), e.download(np.uint32, n, stream=stream),
            x.download(np.float64, n, stream=stream))


# ------------------------- one launch per operator per device (gdsp_*_batch) ------

class BatchItem(C.Structure):
    _fields_ = [("d_in", C.c_void_p), ("d_out", C.c_void_p), ("n", C.c_uint32)]


def batch_items(ins, outs):
    """Table for the gdsp_*_batch calls: vector i is read from ins[i] and written to outs[i] (in-place operators use
    outs only; pass ins=None)."""
    items = (BatchItem * max(len(outs), 1))()
    for i, o in enumerate(outs):
        items[i].d_in = ins[i].ptr.value if ins is not None else None
        items[i].d_out = o.ptr.value
        items[i].n = o.n
    return items


def _batch(name, vecs, outs, *params, stream=None, in_place=False):
    outs = outs if outs is not None else ([v for v in vecs] if in_place else [v.like() for v in vecs])
    items = batch_items(None if in_place else vecs, outs)
    call(name, items, len(outs), *params, _sp(stream))
    return outs


def smooth_batch(vecs, W=101, outs=None, mode=FIR_EXACT, stream=None):
    return _batch("gdsp_smooth_batch", vecs, outs, int(W), int(mode), stream=stream)


def smooth_local_extrema_batch(vecs, W, N, want_max, fill, outs=None, mode=FIR_EXACT, stream=None):
    return _batch("gdsp_smooth_local_extrema_batch", vecs, outs, int(W), int(mode), int(N), int(want_max), float(fill),
                  stream=stream)


def local_extrema_batch(vecs, N, want_max, fill, outs=None, stream=None):
    return _batch("gdsp_local_extrema_batch", vecs, outs, int(N), int(want_max), float(fill), stream=stream)


def best_extrema_batch(vecs, W, want_max, outs=None, stream=None):
    return _batch("gdsp_best_extrema_batch", vecs, outs, int(W), int(want_max), stream=stream)


def sliding_percentile_batch(vecs, W, p_thousandths, outs=None, stream=None):
    return _batch("gdsp_sliding_percentile_batch", vecs, outs, int(W), int(p_thousandths), stream=stream)


def prominence_batch(vecs, W, as_="prominence", outs=None, stream=None):
    return _batch("gdsp_prominence_batch", vecs, outs, int(W), _prominence_what(as_), stream=stream)


def local_stats_batch(vecs, W, as_="zscore", floor=None, minsd=None, outs=None, stream=None):
    return _batch("gdsp_localstats_batch", vecs, outs, *_localstats_params(W, as_, floor, minsd), stream=stream)


def local_mad_batch(vecs, W, as_="zscore", scale=1.4826, threshold=3.0, minmad=None, outs=None, stream=None):
    return _batch("gdsp_localmad_batch", vecs, outs, *_localmad_params(W, as_, scale, threshold, minmad), stream=stream)


def local_correlation_batch(xs, ys, W, as_="correlation", stream=None):
    """local_correlation for every pair in one launch sequence; ys are overwritten and returned"""
    what = _localcorr_what(as_)
    if len(xs) != len(ys) or any(x.n != y.n for x, y in zip(xs, ys)):
        raise ValueError("xs and ys must pair up, vector by vector and length by length")
    return _batch("gdsp_localcorr_batch", xs, list(ys), int(W), what, stream=stream)


def distance_batch(vecs, T=0.0, ties_above=False, to="nearest", signed=False, cap=None, stream=None):
    return _batch("gdsp_distance_batch", vecs, None, *_distance_params(T, ties_above, to, signed, cap), stream=stream,
                  in_place=True)


def fill_gaps_batch(vecs, T=0.0, ties_above=False, known="above", how="linear", ends="extend", maxgap=None, stream=None):
    return _batch("gdsp_fillgaps_batch", vecs, None, *_fill_params(T, ties_above, known, how, ends, maxgap), stream=stream,
                  in_place=True)


def dilate_batch(vecs, left, right, T=0.0, one=1.0, zero=0.0, outs=None, stream=None):
    return _batch("gdsp_dilate_batch", vecs, outs, left, right, float(T), float(one), float(zero), stream=stream)


def erode_batch(vecs, left, right, T=0.0, one=1.0, zero=0.0, outs=None, stream=None):
    return _batch("gdsp_erode_batch", vecs, outs, left, right, float(T), float(one), float(zero), stream=stream)


def dilate_erode_batch(vecs, d_left, d_right, e_left, e_right, d_T=0.0, d_one=1.0, d_zero=0.0, e_T=0.0, e_one=1.0,
                       e_zero=0.0, binarize=None, outs=None, stream=None):
    b = binarize if binarize is not None else (0.0, False, 1.0, 0.0)
    return _batch("gdsp_dilate_erode_batch", vecs, outs, d_left, d_right, float(d_T), float(d_one), float(d_zero),
                  e_left, e_right, float(e_T), float(e_one), float(e_zero), int(binarize is not None),
                  float(b[0]), int(b[1]), float(b[2]), float(b[3]), stream=stream)


def binarize_batch(vecs, T=0.0, ties_above=False, one=1.0, zero=0.0, stream=None):
    return _batch("gdsp_binarize_batch", vecs, None, float(T), int(ties_above), float(one), float(zero), stream=stream,
                  in_place=True)


def clip_batch(vecs, lo=None, hi=None, stream=None):
    return _batch("gdsp_clip_batch", vecs, None, int(lo is not None), float(lo or 0.0), int(hi is not None), float(hi or 0.0),
                  stream=stream, in_place=True)


def erase_batch(vecs, lo=None, hi=None, keep_inside=False, zero=0.0, stream=None):
    return _batch("gdsp_erase_batch", vecs, None, int(lo is not None), float(lo or 0.0), int(hi is not None), float(hi or 0.0),
                  int(keep_inside), float(zero), stream=stream, in_place=True)


def add_constant_batch(vecs, c, stream=None):
    return _batch("gdsp_add_constant_batch", vecs, None, float(c), stream=stream, in_place=True)


def abs_batch(vecs, stream=None):
    return _batch("gdsp_abs_batch", vecs, None, stream=stream, in_place=True)


def synth_coverage(seed, chrom_index, start, count, mode=0, out=None, stream=None):
    out = out if out is not None else DeviceVector(count)
    call("gdsp_synth_coverage", out.ptr, C.c_uint64(seed), chrom_index, start, count, mode, _sp(stream))
    return out
