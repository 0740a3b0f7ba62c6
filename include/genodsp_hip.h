/* genodsp_hip.h -- C ABI of libgenodsp_hip.so, the MI355X (gfx950) device side
 * of the genodsp hot path.
 *
 * Every entry point is what a genodsp operator's `apply` (genodsp_interface.h:76-93
 * in the reference) would call once its chromosome vector lives in HBM: plain
 * pointers and sizes, no C++ or torch types.  `d_` pointers are device memory
 * (hipMalloc, or any allocation a HIP stream can address, 16-byte aligned);
 * `h_` pointers are host memory.  `stream` is a hipStream_t passed as void*
 * (NULL = the default stream).  Calls only enqueue work unless stated
 * otherwise.  Lengths are u32 like the reference's (genodsp_interface.h:45).
 *
 * Return value: 0 on success, a GDSP_E* code otherwise; gdsp_last_error()
 * gives the message.  The library never falls back to a CPU path.
 */
#ifndef GENODSP_HIP_H
#define GENODSP_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDSP_OK        0
#define GDSP_EINVAL    1   /* bad argument                         */
#define GDSP_EHIP      2   /* a HIP runtime call or launch failed  */
#define GDSP_ENOMEM    3

/* FIR arithmetic: EXACT rounds the product and the sum separately, ascending tap
 * order, and is bit-identical to the reference's loop (sum.c:659-662);
 * FMA fuses them (one rounding per tap instead of two). */
#define GDSP_FIR_EXACT 0
#define GDSP_FIR_FMA   1
/* HANN (gdsp_smooth only) uses what the window is -- tap k = c*(1 - cos(w(k+1))) -- and builds
 * each output from block sums of x and of x*exp(jwe): ~45 operations per base for any tap
 * count, additions only (no differences of running sums).  Within W * 2^-52 * sum|w_k v_k| of
 * the reference, like FMA, and no further from the exact value than the reference is.
 * Unlike EXACT and FMA it is not shift invariant (a flat input gives outputs that differ in
 * their last bits), so gdsp_smooth_local_extrema evaluates HANN as FMA.
 * Odd windows of 81..50001 taps have such a kernel (W=101 a dedicated one; beyond 4001 taps the block totals go through HBM,
 * gdsp_hann_far.hip); shorter ones are evaluated as FMA.  A tile that holds inf / NaN / a magnitude >= 2^1017 is evaluated tap by
 * tap (FMA's bits there), so the mode differs from the reference by rounding only on any input. */
#define GDSP_FIR_HANN  2

/* interval overlap operators, values as genodsp_interface.h:157-159 */
#define GDSP_OVERLAP_SUM 0
#define GDSP_OVERLAP_MIN 1
#define GDSP_OVERLAP_MAX 2

const char* gdsp_last_error (void);
const char* gdsp_version    (void);
/* debugging aid: 1 and *value = the pattern when the environment holds GDSP_POISON=<double|nan>, else 0.  Every gdsp_malloc
 * is then filled with it, and the driver refills a vector's partner after every flip: a kernel that reads memory nobody
 * wrote changes the output (tests/test_cli_hip.py::test_no_operator_reads_memory_nobody_wrote). */
int gdsp_poison (double* value);

/* ---- runtime plumbing (what genodsp.c:865-878 / :1890-2037 do with calloc) ---- */
int gdsp_device_count   (int* count);
int gdsp_set_device     (int device);
int gdsp_get_device     (int* device);
int gdsp_malloc         (void** d_ptr, size_t bytes);      /* (filled with GDSP_POISON when that is set, see gdsp_poison) */
int gdsp_free           (void* d_ptr);
int gdsp_host_alloc     (void** h_ptr, size_t bytes);          /* pinned staging  */
int gdsp_host_free      (void* h_ptr);
int gdsp_memcpy_h2d     (void* d_dst, const void* h_src, size_t bytes, void* stream);
int gdsp_memcpy_d2h     (void* h_dst, const void* d_src, size_t bytes, void* stream);
int gdsp_memcpy_d2d     (void* d_dst, const void* d_src, size_t bytes, void* stream);
int gdsp_memcpy_peer    (void* d_dst, int dstDevice, const void* d_src, int srcDevice, size_t bytes, void* stream); /* GPU to GPU (xGMI) */
int gdsp_memset         (void* d_dst, int byte, size_t bytes, void* stream);
int gdsp_stream_create  (void** stream);
int gdsp_stream_destroy (void* stream);
int gdsp_stream_sync    (void* stream);
int gdsp_device_sync    (void);                                /* every stream of the current device */
int gdsp_event_create   (void** event);
int gdsp_event_destroy  (void* event);
int gdsp_event_record   (void* event, void* stream);
int gdsp_stream_wait_event (void* stream, void* event);         /* work queued on stream from now on starts after the event (independent
                                                                 * chromosomes on alternating streams hide the drain between kernels: +3..5 %) */
int gdsp_event_elapsed_ms (void* start, void* stop, float* ms); /* syncs on stop   */
int gdsp_fill           (double* d_v, uint32_t n, double val, void* stream);

/* ---- sum.c ---------------------------------------------------------------------- */

/* Host: the reference's Hann taps (sum.c:632-645), W odd >= 3. */
int gdsp_hann_taps (uint32_t W, double* h_taps);

/* op_smooth_apply (sum.c:616-676): zero-padded W-tap FIR, out-of-place.  A plan takes any odd number W >= 1 of
 * arbitrary finite taps and applies them as out[i] = sum_k w[k] v[i-h+k], h = (W-1)/2, k ascending from a sum of +0.0,
 * inputs outside [0,n) skipped: correlation order, the taps are NOT flipped (a convolution kernel is passed reversed).
 * GDSP_FIR_EXACT rounds every product and every sum, GDSP_FIR_FMA fuses each tap's two into one rounding.
 * gdsp_fir_plan_create refuses a NaN or infinite tap (GDSP_EINVAL): the kernels pad with zeros instead of skipping,
 * which is the same only while tap * (+0.0) is a zero, and inf * 0 is NaN. */
typedef struct gdsp_fir_plan gdsp_fir_plan;
int gdsp_fir_plan_create  (gdsp_fir_plan** plan, const double* h_taps, uint32_t W);
int gdsp_fir_plan_destroy (gdsp_fir_plan* plan);
int gdsp_fir_apply        (const gdsp_fir_plan* plan, const double* d_in, double* d_out,
                           uint32_t n, int mode, void* stream);
/* convenience: Hann plan for W cached inside the library (per device) */
int gdsp_smooth           (const double* d_in, double* d_out, uint32_t n, uint32_t W,
                           int mode, void* stream);

/* `= smooth W = localmax|localmin N` in one pass (sum.c:616-676 feeding minmax.c:1183-1227 /
 * :981-1022): the smoothed tile is tested in LDS and only the peaks track is written.
 * Bit-identical to gdsp_smooth followed by gdsp_local_extrema.  Fusable for W=101, N<=129.
 * Synchronisation: for W=101 and N<=15 the call takes the filtered route (gdsp_peaks.hip), which reads a probe's counts
 * back to choose each vector's form: it WAITS for the stream once per table of <= 32 vectors (everything queued on the
 * stream before it included) and cannot be captured into a graph.  GDSP_PEAKS_FLAT=0 keeps the decision on the device
 * (no wait; vectors of flat stretches then take the direct kernel), GDSP_PEAKS_FILTER=0 the direct kernel throughout. */
int gdsp_smooth_local_extrema_fusable (uint32_t W, uint32_t N);
int gdsp_smooth_local_extrema (const double* d_in, double* d_out, uint32_t n, uint32_t W, int mode,
                               uint32_t N, int wantMax, double fill, void* stream);

/* op_sliding_sum_apply (sum.c:420-463): centred window sum / denom, out-of-place.
 * Bit-identical to the reference whenever every partial sum is exact (integer
 * or dyadic signals); otherwise within the running-sum rounding bound. */
int gdsp_sliding_sum      (const double* d_in, double* d_out, uint32_t n, uint32_t W,
                           double denom, void* stream);
/* op_window_sum_apply (sum.c:211-252), in place. */
int gdsp_window_sum       (double* d_v, uint32_t n, uint32_t W, double denom, int useActual,
                           double zeroVal, void* stream);
/* op_cumulative_sum_apply (sum.c:776-792), in place; d_work >= gdsp_cumulative_sum_work(n) bytes. */
size_t gdsp_cumulative_sum_work (uint32_t n);
int gdsp_cumulative_sum   (double* d_v, uint32_t n, void* d_work, void* stream);

/* ---- minmax.c ------------------------------------------------------------------- */

/* op_local_maxima_apply / op_local_minima_apply (minmax.c:1183-1227, :981-1022) */
int gdsp_local_extrema (const double* d_in, double* d_out, uint32_t n, uint32_t N,
                        int wantMax, double fill, void* stream);
/* op_best_local_max_apply / _min_ (minmax.c:1616-1721, :1369-1474): sliding max/min */
int gdsp_best_extrema  (const double* d_in, double* d_out, uint32_t n, uint32_t W,
                        int wantMax, void* stream);

/* Any window length (the tiled kernels above stop at what one LDS tile holds and return
 * GDSP_EINVAL beyond): the *_any forms use the tiled kernel when it applies and otherwise
 * whole-vector passes through d_work (>= gdsp_long_window_work(n) bytes of device memory). */
size_t gdsp_long_window_work (uint32_t n);
int gdsp_best_extrema_any  (const double* d_in, double* d_out, uint32_t n, uint32_t W, int wantMax,
                            void* d_work, size_t workBytes, void* stream);
int gdsp_local_extrema_any (const double* d_in, double* d_out, uint32_t n, uint32_t N, int wantMax, double fill,
                            void* d_work, size_t workBytes, void* stream);
int gdsp_sliding_sum_any   (const double* d_in, double* d_out, uint32_t n, uint32_t W, double denom,
                            void* d_work, size_t workBytes, void* stream);

/* ---- morphology.c --------------------------------------------------------------- */

/* All four binarise with v > T and write only one/zero.  Out-of-place
 * (d_out may not alias d_in). */
int gdsp_dilate (const double* d_in, double* d_out, uint32_t n, uint32_t left, uint32_t right,
                 double T, double one, double zero, void* stream);   /* :882-1072  */
int gdsp_erode  (const double* d_in, double* d_out, uint32_t n, uint32_t left, uint32_t right,
                 double T, double one, double zero, void* stream);   /* :1331-1454 */
/* `= dilate = erode [= binarize]` in one pass (morphology.c:882-1072 -> :1331-1454 ->
 * logical.c:216-268): the dilated set stays in LDS as a bit mask.  Bit-identical to the
 * three calls in sequence; each stage keeps its own threshold and output values. */
int gdsp_dilate_erode_fusable (uint32_t dLeft, uint32_t dRight, uint32_t eLeft, uint32_t eRight);   /* 1: fused for any vector length */
int gdsp_dilate_erode (const double* d_in, double* d_out, uint32_t n,
                       uint32_t dLeft, uint32_t dRight, double dT, double dOne, double dZero,
                       uint32_t eLeft, uint32_t eRight, double eT, double eOne, double eZero,
                       int binarize, double bT, int bTiesAbove, double bOne, double bZero, void* stream);
int gdsp_close  (const double* d_in, double* d_out, uint32_t n, double closingLength,
                 double T, double one, double zero, void* stream);   /* :231-319   */
int gdsp_open   (const double* d_in, double* d_out, uint32_t n, double openingLength,
                 double T, double one, double zero, void* stream);   /* :529-605   */

/* Any length (the reference accepts any, morphology.c:696-866, :1163-1315; the tiled kernels above return GDSP_EINVAL
 * once a window reaches beyond the 262 k bases one LDS tile can stage): the tiled kernel when it applies, otherwise
 * the set as bits plus per-word next / previous-member tables in d_work (>= gdsp_long_window_work(n) bytes). */
int gdsp_dilate_any (const double* d_in, double* d_out, uint32_t n, uint32_t left, uint32_t right,
                     double T, double one, double zero, void* d_work, size_t workBytes, void* stream);
int gdsp_erode_any  (const double* d_in, double* d_out, uint32_t n, uint32_t left, uint32_t right,
                     double T, double one, double zero, void* d_work, size_t workBytes, void* stream);
int gdsp_close_any  (const double* d_in, double* d_out, uint32_t n, double closingLength,
                     double T, double one, double zero, void* d_work, size_t workBytes, void* stream);
int gdsp_open_any   (const double* d_in, double* d_out, uint32_t n, double openingLength,
                     double T, double one, double zero, void* d_work, size_t workBytes, void* stream);

/* ---- one launch per operator per device (replaces the chromosome loop of genodsp.c:909-921) ----------------------
 * The reference applies an operator to one chromosome after the other.  On the GPU every launch ramps up and drains
 * (10-15 % of a short kernel's time), so a device that holds several chromosomes -- or several stretches of them --
 * is given ONE grid that covers all of its vectors: items[i] = (input, output, length) of vector i, all on the current
 * device, all 16-byte aligned, outputs distinct from inputs for the out-of-place operators (in-place operators use
 * d_out only).  Results are those of the single-vector calls bit for bit (the same kernels; only the block-to-tile
 * map differs).  Any number of items; tables of 32 vectors travel in the kernel arguments. */
typedef struct gdsp_batch_item { const double* d_in;  double* d_out;  uint32_t n; } gdsp_batch_item;
int gdsp_smooth_batch               (const gdsp_batch_item* items, int nitems, uint32_t W, int mode, void* stream);
int gdsp_smooth_local_extrema_batch (const gdsp_batch_item* items, int nitems, uint32_t W, int mode,
                                     uint32_t N, int wantMax, double fill, void* stream);
int gdsp_local_extrema_batch        (const gdsp_batch_item* items, int nitems, uint32_t N, int wantMax, double fill, void* stream);
int gdsp_best_extrema_batch         (const gdsp_batch_item* items, int nitems, uint32_t W, int wantMax, void* stream);
int gdsp_dilate_batch               (const gdsp_batch_item* items, int nitems, uint32_t left, uint32_t right,
                                     double T, double one, double zero, void* stream);
int gdsp_erode_batch                (const gdsp_batch_item* items, int nitems, uint32_t left, uint32_t right,
                                     double T, double one, double zero, void* stream);
int gdsp_dilate_erode_batch         (const gdsp_batch_item* items, int nitems,
                                     uint32_t dLeft, uint32_t dRight, double dT, double dOne, double dZero,
                                     uint32_t eLeft, uint32_t eRight, double eT, double eOne, double eZero,
                                     int binarize, double bT, int bTiesAbove, double bOne, double bZero, void* stream);
int gdsp_binarize_batch             (const gdsp_batch_item* items, int nitems, double T, int tiesAbove, double one, double zero, void* stream);
int gdsp_clip_batch                 (const gdsp_batch_item* items, int nitems, int haveMin, double minVal, int haveMax, double maxVal, void* stream);
int gdsp_erase_batch                (const gdsp_batch_item* items, int nitems, int haveMin, double minVal, int haveMax, double maxVal,
                                     int keepInside, double zero, void* stream);
int gdsp_add_constant_batch         (const gdsp_batch_item* items, int nitems, double c, void* stream);
int gdsp_abs_batch                  (const gdsp_batch_item* items, int nitems, void* stream);
/* GDSP_EINVAL from a *_batch call whose parameters the single-vector call would also refuse, or for which no tiled
 * kernel exists (the caller then loops over the vectors with the single-vector / *_any forms). */

/* ---- slidingpercentile / median (not in the reference): exact order statistics over a sliding window ------------
 * For a vector v of n values, a window W (1 <= W <= GDSP_SLIDING_PERCENTILE_MAX_WINDOW) and P in thousandths of a
 * percent (0..100000): wL = (W-1)/2, wR = W-1-wL (bestmax's centring: for even W the extra base is on the right).
 * The window of base i is [max(0, i-wL), min(n-1, i+wR)]: bases beyond the ends are not considered, as in bestmax;
 * n_i is the number of bases in it and k_i = gdsp_percentile_rank(n_i, P).  out[i] is gdsp_key_to_double of the
 * k_i-th smallest (from 0) of the keys gdsp_double_to_key(v[j]) over the window: the order `percentile` uses, -0.0
 * folded onto +0.0 (printed as 0), NaNs ordered by their bits (positive NaNs above +inf, negative ones below -inf).
 * The result is an input value, bit exact.  P = 0 and P = 100000 are bestmin and bestmax (on data without -0.0 and
 * NaN).  Out-of-place; GDSP_EINVAL for d_in == d_out, W == 0, W above the maximum or P > 100000; n == 0 is a no-op.
 * One kernel launch covers every vector of a batch (gdsp_rankfilt.hip: per tile a sort and a wavelet matrix in LDS,
 * then one range-quantile query per base; the cost per base does not grow with W). */
#define GDSP_SLIDING_PERCENTILE_MAX_WINDOW 4095
/* Host: outputs per workgroup tile of the kernel for window W (0 outside 1..the maximum); results never depend on it */
uint32_t gdsp_sliding_percentile_tile (uint32_t W);
int gdsp_sliding_percentile       (const double* d_in, double* d_out, uint32_t n, uint32_t W, uint32_t pThousandths, void* stream);
int gdsp_sliding_percentile_batch (const gdsp_batch_item* items, int nitems, uint32_t W, uint32_t pThousandths, void* stream);

/* ---- prominence (not in the reference): how far each base stands above its surroundings -------------------------
 * Take a vector v of n values and a window W with 1 <= W <= GDSP_PROMINENCE_MAX_WINDOW.  Let wL = (W-1)/2 and
 * wR = W-1-wL, which is bestmax's centring: for even W the extra base is on the right.
 * For base i, with x = v[i] and plain IEEE comparisons on doubles:
 *   Left walk:  j = i-1, i-2, ... while j >= max(0, i-wL) and not v[j] > x.
 *   mL starts as x and is replaced by v[j] whenever v[j] < mL (strictly).
 *   Right walk: the same over j = i+1 ... min(n-1, i+wR), giving mR.
 *   base = mL if mL >= mR, else mR.
 *   prominence = +0.0 if x == base, else x - base.  That is one rounded subtraction.
 * So the result is never negative and never -0.0; no NaN arises from NaN-free input (inf - inf cannot happen because
 * of the x == base rule); a base with a strictly higher neighbour gets 0; every base of a plateau gets the plateau's
 * prominence; a base at a chromosome end gets 0, because the missing side contributes x.  For odd W this is the
 * prominence with window length W of scipy.signal.peak_prominences, evaluated at every base.
 * If the window [i-wL, i+wR] of a base contains a NaN, the result at that base is unspecified (some double); every
 * other base gets the defined result.
 * what: GDSP_PROMINENCE_VALUE writes prominence, GDSP_PROMINENCE_BASE writes base (an input value; the sign of a zero
 * is whichever of the equal candidates was met).  Out-of-place; GDSP_EINVAL for d_in == d_out, W == 0, W above the
 * maximum or an unknown `what`; n == 0 is a no-op.  One kernel launch covers every vector of a batch
 * (gdsp_prominence.hip: per tile a max / min summary of every aligned block of 8, 64 and 512 staged positions in LDS;
 * the bases without a higher neighbour walk outwards over single values, then blocks of 8, 64 and 512, and down again
 * towards the end of the window: under 50 LDS reads per side whatever the data). */
#define GDSP_PROMINENCE_MAX_WINDOW 4095
#define GDSP_PROMINENCE_VALUE 0
#define GDSP_PROMINENCE_BASE  1
/* Host: outputs per workgroup tile of the kernel for window W (0 outside 1..the maximum); results never depend on it */
uint32_t gdsp_prominence_tile  (uint32_t W);
int gdsp_prominence       (const double* d_in, double* d_out, uint32_t n, uint32_t W, int what, void* stream);
int gdsp_prominence_batch (const gdsp_batch_item* items, int nitems, uint32_t W, int what, void* stream);

/* ---- localstats (not in the reference): each base against the mean and variance of the window centred on it -----
 * Take a vector v of n values and a window W with 1 <= W <= GDSP_LOCALSTATS_MAX_WINDOW.  The window is slidingsum's
 * (sum.c:436-455), cut off at the ends of the vector: with rgt = (W-1)/2 and lft = W-1-rgt (an even W reaches one
 * base further to the left), base c has lo = max(0, c-lft), hi = min(n-1, c+rgt) and m = hi-lo+1 bases in its window.
 *   S1 = the sum of v[k], S2 = the sum of fl(v[k] v[k]) over k = lo .. hi (one rounded product per term).
 * From these, every step one rounded IEEE operation on doubles, in this order and never fused:
 *   mean     = fl(S1 / m)
 *   N        = fl(fl(m S2) - fl(S1 S1))
 *   variance = +0.0 if N <= 0, else fl(N / fl(m m))          (the population variance, as in gdsp_genome_stats)
 *   stddev   = sqrt(variance), correctly rounded
 *   bg       = floor if haveFloor and floor > mean, else mean       (MACS's max(local, genome-wide))
 *   sd       = minSd if haveMinSd and minSd > stddev, else stddev
 * what:  GDSP_LOCALSTATS_MEAN       writes bg
 *        GDSP_LOCALSTATS_VARIANCE   writes variance
 *        GDSP_LOCALSTATS_STDDEV     writes sd
 *        GDSP_LOCALSTATS_DIFFERENCE writes fl(v[c] - bg)
 *        GDSP_LOCALSTATS_RATIO      writes fl(v[c] / bg), +0.0 where bg == 0
 *        GDSP_LOCALSTATS_ZSCORE     writes fl(fl(v[c] - mean) / sd), +0.0 where sd == 0
 * so the floor touches mean, difference and ratio only, and minSd stddev and zscore only.
 * The two sums may be formed in any order or tree, inside the tile a workgroup stages: no further than
 * gdsp_localstats_tile(W) bases beyond the window on either side.  A result therefore lies within what
 * S1 +- gamma_M A1 and S2 +- gamma_M A2 allow, M = 2 (W + tile) + 4, A the sum of the magnitudes over the window
 * widened by the tile (tests/localstats_ref.py pushes those intervals through the steps above).  Where no sum of those
 * terms can round, every figure is the definition's, bit for bit, however the implementation sums: for read depth N is
 * exact while m S2 < 2^53 (depth up to about 9000 at W = 10001) and variance is then the exact population variance of
 * the window, rounded once.  Non-finite values inside a window give that base whatever the arithmetic above gives.
 * Out-of-place; GDSP_EINVAL for d_in == d_out, W == 0, W above the maximum or an unknown `what`; n == 0 is a no-op.
 * One kernel launch covers every vector of a batch, and the single-vector call runs the same kernel over a table of
 * one (gdsp_localstats.hip: per tile the staged values in LDS, running sums over blocks of 16 of them for v and for
 * fl(v v), each window's two sums as differences, and the staged v for the last step). */
#define GDSP_LOCALSTATS_MAX_WINDOW 12287       /* what leaves a workgroup's 16384 staged values a tile of 4096 */
#define GDSP_LOCALSTATS_ZSCORE     0
#define GDSP_LOCALSTATS_MEAN       1
#define GDSP_LOCALSTATS_VARIANCE   2
#define GDSP_LOCALSTATS_STDDEV     3
#define GDSP_LOCALSTATS_DIFFERENCE 4
#define GDSP_LOCALSTATS_RATIO      5
/* Host: outputs per workgroup tile of the kernel for window W (0 outside 1..the maximum) */
uint32_t gdsp_localstats_tile  (uint32_t W);
int gdsp_localstats       (const double* d_in, double* d_out, uint32_t n, uint32_t W, int what,
                           int haveFloor, double floor, int haveMinSd, double minSd, void* stream);
int gdsp_localstats_batch (const gdsp_batch_item* items, int nitems, uint32_t W, int what,
                           int haveFloor, double floor, int haveMinSd, double minSd, void* stream);

/* ---- localmad / hampel (not in the reference): each base against the median and the MAD of the window around it ---
 * Take a vector v of n values and a window W with 1 <= W <= GDSP_LOCALMAD_MAX_WINDOW.  Window, centring and rank are
 * slidingpercentile's: wL = (W-1)/2, wR = W-1-wL; the window of base i is [max(0, i-wL), min(n-1, i+wR)] with m bases
 * in it, and k = gdsp_percentile_rank(m, 50000) = m/2 counted from 0: the upper median for even m.
 *   med   = what gdsp_sliding_percentile at P = 50000 writes for base i: the k-th smallest key of the window, -0.0
 *           folded onto +0.0
 *   d_j   = |fl(v_j - med)| for every base j of the window: one rounded subtraction, then the sign cleared
 *   mad   = the k-th smallest d_j, counted from 0, with the same k (the median absolute deviation)
 *   madf  = minMad if haveMinMad and minMad > mad, else mad
 *   sigma = fl(scale madf)                      (scale 1.4826 makes sigma estimate a normal distribution's stddev)
 *   diff  = +0.0 where v_i == med, else fl(v_i - med)
 *   limit = fl(threshold sigma)
 *   base i is an outlier where |diff| > limit; with sigma == 0 every base that differs from its median is one, which
 *   is Hampel's own behaviour (minMad is there to temper it).
 * Every step is one rounded IEEE operation on doubles, in this order and never fused.
 * what:  GDSP_LOCALMAD_ZSCORE     writes fl(diff / sigma), +0.0 where sigma == 0 (localstats' rule)
 *        GDSP_LOCALMAD_MEDIAN     writes med
 *        GDSP_LOCALMAD_MAD        writes madf
 *        GDSP_LOCALMAD_DIFFERENCE writes diff
 *        GDSP_LOCALMAD_CLEAN      writes med where the base is an outlier, else v_i bit for bit (the Hampel filter)
 *        GDSP_LOCALMAD_OUTLIER    writes 1.0 where the base is an outlier, else 0.0
 * The definition holds where every value of the window is finite (a deviation may overflow to +inf: that is still
 * ordered).  Where a window holds a NaN or an infinity the figure at that base is unspecified (some double); the call
 * still ends, and every base whose window holds none gets the definition's figure.  At W = 1 mad is 0, CLEAN is the
 * input and OUTLIER is 0.
 * Out-of-place; GDSP_EINVAL for d_in == d_out, W == 0, W above the maximum, an unknown `what`, a scale that is not
 * finite and positive, or a threshold or minMad that is NaN or negative; n == 0 is a no-op.  One kernel launch covers
 * every vector of a batch (gdsp_localmad.hip: slidingpercentile's tile -- one sort and one wavelet matrix in LDS --
 * then per base the median's range-quantile query and a binary search for the block of the k+1 smallest deviations,
 * two such queries per probe: at most 2 + 2 ceil(log2(k+1)) queries, whatever the values). */
#define GDSP_LOCALMAD_MAX_WINDOW 4095          /* GDSP_SLIDING_PERCENTILE_MAX_WINDOW: the same tile */
#define GDSP_LOCALMAD_ZSCORE     0
#define GDSP_LOCALMAD_MEDIAN     1
#define GDSP_LOCALMAD_MAD        2
#define GDSP_LOCALMAD_DIFFERENCE 3
#define GDSP_LOCALMAD_CLEAN      4
#define GDSP_LOCALMAD_OUTLIER    5
/* Host: outputs per workgroup tile of the kernel for window W (0 outside 1..the maximum); results never depend on it */
uint32_t gdsp_localmad_tile  (uint32_t W);
int gdsp_localmad       (const double* d_in, double* d_out, uint32_t n, uint32_t W, int what,
                         double scale, double threshold, int haveMinMad, double minMad, void* stream);
int gdsp_localmad_batch (const gdsp_batch_item* items, int nitems, uint32_t W, int what,
                         double scale, double threshold, int haveMinMad, double minMad, void* stream);

/* ---- localcorrelate (not in the reference): the signal against a second track over the window centred on each base -
 * Take x (the signal) and y (the track) of n values each and a window W with 1 <= W <= GDSP_LOCALCORR_MAX_WINDOW.
 * The window is localstats' and slidingsum's: with rgt = (W-1)/2 and lft = W-1-rgt, base c has lo = max(0, c-lft),
 * hi = min(n-1, c+rgt) and m = hi-lo+1 bases in its window.  Over k = lo .. hi, each term one rounded product:
 *   Sx = sum x[k]   Sy = sum y[k]   Sxx = sum fl(x[k] x[k])   Syy = sum fl(y[k] y[k])   Sxy = sum fl(x[k] y[k])
 * From these, every step one rounded IEEE operation on doubles, in this order and never fused:
 *   md  = (double) m                 mm  = fl(md md)
 *   Nxx = fl(fl(md Sxx) - fl(Sx Sx))
 *   Nyy = fl(fl(md Syy) - fl(Sy Sy))
 *   Nxy = fl(fl(md Sxy) - fl(Sx Sy))
 *   covariance  = +0.0 if Nxy == 0, else fl(Nxy / mm)               (the population covariance, as in gdsp_genome_correlation)
 *   correlation = +0.0 if Nxx <= 0 or Nyy <= 0;
 *                 else D = fl(sqrt(Nxx) * sqrt(Nyy)), each sqrt correctly rounded;
 *                      +0.0 if D == 0, else fl(Nxy / D), clamped into [-1, 1]
 *   slope       = +0.0 if Nxx <= 0, else fl(Nxy / Nxx)              (the track regressed on the signal: correlate's direction)
 *   intercept   = fl(fl(Sy / md) - fl(slope * fl(Sx / md)))
 * what:  GDSP_LOCALCORR_CORRELATION, _COVARIANCE, _SLOPE or _INTERCEPT writes that figure.
 * The five sums may be formed in any order or tree, inside the tile a workgroup stages: no further than
 * gdsp_localcorr_tile(W) bases beyond the window on either side -- the allowance localstats states.  A result therefore
 * lies within what S +- gamma_M A allows for each of the five, M = 2 (W + tile) + 4, A the sum of the magnitudes of that
 * sum's terms over the window widened by the tile (tests/localcorr_ref.py pushes those intervals through the steps
 * above).  Where no sum of those terms can round, every figure is the definition's, bit for bit, however the
 * implementation sums: for read depth while m Sxx, m Syy and m |Sxy| stay below 2^53.  Non-finite values inside a window
 * give that base whatever the arithmetic above gives.
 * d_x (items[].d_in) is the signal and is only read.  d_y (items[].d_out) holds the track on entry and the result on
 * return: the caller then treats d_y as the new signal, exactly as after any out-of-place operator, and the old signal
 * is nobody's data any more.  GDSP_EINVAL for d_x == d_y, a NULL or misaligned (16 bytes) pointer, W == 0, W above the
 * maximum or an unknown `what`; n == 0 is a no-op.
 * Two launches in stream order cover every vector of a batch, 32 vectors at a time, and the single-vector call runs
 * the same over a table of one (gdsp_localcorr.hip).  A tile's halo bases of the track are its neighbours' own bases,
 * which they overwrite, so a small kernel first copies, for every tile, the HL track values before it and the HR behind
 * it (0.0 outside the vector) into a record of HL + HR doubles in workspace of the library's own (per device, grown on
 * demand and kept; calls on several streams of a device take it in turn).  The main kernel then stages x from d_x, its
 * own T track values from d_y and the halos from its record, forms the five sums as localstats forms its two, and
 * writes its T results over d_y only after every thread of the workgroup has finished reading.  No workgroup reads a
 * live base that another one writes; nothing is polled and nothing waits on another workgroup.
 * The workspace is (HL + HR) / T of the track: about 1 % of it at W = 101, 14 % at W = 1001 and 100 % at W = 4097.
 * gdsp_localcorr_times: with GDSP_LOCALCORR_TIMES=1 in the environment, the milliseconds of the last call's two
 * launches, from events (the call then waits for them); zeros otherwise. */
#define GDSP_LOCALCORR_MAX_WINDOW  4097        /* what leaves a workgroup's 8192 staged positions a tile of 4096 */
#define GDSP_LOCALCORR_CORRELATION 0
#define GDSP_LOCALCORR_COVARIANCE  1
#define GDSP_LOCALCORR_SLOPE       2
#define GDSP_LOCALCORR_INTERCEPT   3
/* Host: outputs per workgroup tile of the kernel for window W (0 outside 1..the maximum) */
uint32_t gdsp_localcorr_tile  (uint32_t W);
int gdsp_localcorr       (const double* d_x, double* d_y, uint32_t n, uint32_t W, int what, void* stream);
int gdsp_localcorr_batch (const gdsp_batch_item* items, int nitems, uint32_t W, int what, void* stream);
void gdsp_localcorr_times (double ms[2]);

/* ---- distance (not in the reference): every base to the nearest base above a threshold ----------------------------
 * Take a vector v of n values, a threshold T with tiesAbove, a side `to`, a flag isSigned and a cap R (0: none).
 * Base i is a member iff v[i] > T, or v[i] >= T with tiesAbove: the test of gdsp_segments_batch; a NaN is never a member.
 * For base i let L(i) be the largest member j <= i and Rt(i) the smallest member j >= i; either may not exist.
 *   dl = i - L(i), dr = Rt(i) - i
 *   to:  GDSP_DISTANCE_NEAREST  d = the smaller of those that exist
 *        GDSP_DISTANCE_LEFT     d = dl  (towards lower coordinates)
 *        GDSP_DISTANCE_RIGHT    d = dr
 *   and d = n where nothing exists on the asked side(s): no distance reaches it (the largest is n-1).
 * Unsigned: out[i] = d, so a member gets +0.0.
 * Signed: a non-member gets d; a member gets -e, where e is the same figure for the complement set with positions -1
 * and n counted as non-members (erode's convention: outside the vector is not in S).  So e >= 1 always exists, nothing
 * is 0, the edge bases of a run are -1 and the base next to a run is +1; with LEFT / RIGHT e looks that way only.
 * Cap R >= 1: out[i] = min(d, R), respectively max(-e, -R); a base with nothing on the asked side gets R, not n.  With
 * a cap, out[i] depends on v[i-R .. i+R] only and not on where i lies in the vector.
 * Every output is an integer held exactly by a double (n <= 2^32-1); the values enter through the membership test
 * alone, so the result is the definition's bit for bit on any input.
 * In place.  gdsp_distance_batch uses d_out only, as the other in-place batch calls.  GDSP_EINVAL for an unknown `to` or
 * a NaN T; n == 0 is a no-op.  Three launches in stream order cover every vector of the batch, 32 vectors at a time
 * (gdsp_distance.hip: membership bits and tile extents; a join of the extents per vector; the write), in workspace of
 * the library's own (n/8 bytes and 32 per tile, per device, kept); calls on several streams of a device take it in turn.
 * gdsp_distance_times: with GDSP_DISTANCE_TIMES=1 in the environment, the milliseconds of the last call's three
 * launches, from events (the call then waits for them); zeros otherwise. */
#define GDSP_DISTANCE_NEAREST 0
#define GDSP_DISTANCE_LEFT    1
#define GDSP_DISTANCE_RIGHT   2
/* Host: bases per workgroup tile; results never depend on it */
uint32_t gdsp_distance_tile  (void);
int gdsp_distance       (double* d_v, uint32_t n, double T, int tiesAbove, int to, int isSigned, uint32_t cap, void* stream);
int gdsp_distance_batch (const gdsp_batch_item* items, int nitems, double T, int tiesAbove, int to, int isSigned,
                         uint32_t cap, void* stream);
void gdsp_distance_times (double ms[3]);

/* ---- fillgaps (not in the reference): the signal interpolated across its uncovered bases ------------------------------
 * Take a vector v of n values, a test `known` with its threshold T and tiesAbove, a way to fill `how`, a treatment of the
 * ends `ends` and a longest gap G (maxgap; 0: no limit).
 * Known bases.  GDSP_FILL_KNOWN_ABOVE: base i is known iff v[i] > T, or v[i] >= T with tiesAbove (the test of
 * gdsp_segments_batch).  GDSP_FILL_KNOWN_NONZERO: iff v[i] != 0 and v[i] == v[i]; negative values count, both zeros do
 * not, and T and tiesAbove are not used.  A NaN is never known under either test.  A known base keeps its value bit for
 * bit, infinities included.
 * Gaps.  A gap is a maximal run of unknown bases.  An interior gap has a known base l just before it and a known base r
 * just behind it; for its base i let a = v[l], b = v[r], d = r - l, k = i - l.  An end gap touches the vector's start or
 * its end and has one known neighbour.  A vector without a known base is left untouched, bit for bit.
 *   how:  GDSP_FILL_LINEAR   interior: a where a == b (bit for bit); otherwise x = fl(a + fl(fl(fl(b - a) * k) / d)),
 *                            every step rounded once and none fused, k and d exact doubles, and then clamped:
 *                            x < lo ? lo : (x > hi ? hi : x) with lo = min(a, b), hi = max(a, b).  A NaN (from
 *                            inf - inf) passes through the clamp as NaN.
 *         GDSP_FILL_NEAREST  interior: a where k <= d - k, else b; a tie goes to the lower coordinate
 *         GDSP_FILL_LEFT     a: forward fill
 *         GDSP_FILL_RIGHT    b
 *   ends: GDSP_FILL_ENDS_EXTEND  a base whose mode needs a side that does not exist takes the value of the side that
 *                            does: the end gaps under every mode; under LEFT the bases before the first known base,
 *                            under RIGHT those behind the last
 *         GDSP_FILL_ENDS_KEEP    such a base keeps its own value, bit for bit
 *   G >= 1: a gap of more than G bases is left as it is, bit for bit, interior gaps and end gaps alike.  With G, out[i]
 *   depends on v[i-G-1 .. i+G+1] only (ops_fillgaps.c has the argument).
 * Only the four operations above touch values, so the result is the definition's bit for bit on any input.
 * In place.  gdsp_fillgaps_batch uses d_out only, as the other in-place batch calls.  GDSP_EINVAL for an unknown `known`,
 * `how` or `ends`, or a NaN T under GDSP_FILL_KNOWN_ABOVE; n == 0 is a no-op.  Three launches in stream order cover every
 * vector of the batch, 32 vectors at a time (gdsp_fillgaps.hip: the known bases as bits, and tile extents; a join of the
 * extents per vector; the write, which skips every tile that has nothing to fill), in the workspace that gdsp_distance
 * uses (one per device, kept); calls on several streams of a device take it in turn.
 * gdsp_fillgaps_times: with GDSP_FILLGAPS_TIMES=1 in the environment, the milliseconds of the last call's three
 * launches, from events (the call then waits for them); zeros otherwise. */
#define GDSP_FILL_KNOWN_ABOVE   0
#define GDSP_FILL_KNOWN_NONZERO 1
#define GDSP_FILL_LINEAR        0
#define GDSP_FILL_NEAREST       1
#define GDSP_FILL_LEFT          2
#define GDSP_FILL_RIGHT         3
#define GDSP_FILL_ENDS_EXTEND   0
#define GDSP_FILL_ENDS_KEEP     1
/* Host: bases per workgroup tile; results never depend on it */
uint32_t gdsp_fillgaps_tile  (void);
int gdsp_fillgaps       (double* d_v, uint32_t n, double T, int tiesAbove, int known, int how, int ends, uint32_t maxgap,
                         void* stream);
int gdsp_fillgaps_batch (const gdsp_batch_item* items, int nitems, double T, int tiesAbove, int known, int how, int ends,
                         uint32_t maxgap, void* stream);
void gdsp_fillgaps_times (double ms[3]);

/* ---- logical.c, mask.c, add.c (in place) ---------------------------------------- */
int gdsp_binarize     (double* d_v, uint32_t n, double T, int tiesAbove, double one, double zero,
                       void* stream);                                 /* logical.c:216-268 */
int gdsp_clip         (double* d_v, uint32_t n, int haveMin, double minVal, int haveMax,
                       double maxVal, void* stream);                  /* mask.c:850-924    */
int gdsp_erase        (double* d_v, uint32_t n, int haveMin, double minVal, int haveMax,
                       double maxVal, int keepInside, double zero, void* stream); /* mask.c:1147-1243 */
int gdsp_add_constant (double* d_v, uint32_t n, double c, void* stream);   /* add.c:726-741   */
int gdsp_abs          (double* d_v, uint32_t n, void* stream);             /* add.c:1038-1049 */
int gdsp_invert       (double* d_v, uint32_t n, double mid, void* stream); /* add.c:927-937   */
/* op_map_apply (map.c:194-381): piecewise-linear mapping through nknots (in,out) knots sorted by
 * `in` (device arrays).  Bit-identical to the reference for strictly increasing knots. */
int gdsp_map          (double* d_v, uint32_t n, const double* d_knotIn, const double* d_knotOut,
                       uint32_t nknots, void* stream);
/* clump_search (clump.c:494-736), op_clump_apply (above != 0) / op_skimp_apply: bases in stretches
 * of at least minLength whose average is >= (<=) `average` become `one`, the rest `zero`; each
 * merged run is trimmed to its first and last base on the right side of the threshold.  In place;
 * d_work >= gdsp_clump_work(n) bytes.  Whole-vector scans; bit-identical to the reference whenever
 * the running sum of (v - average) is exactly representable (depth against a dyadic threshold). */
size_t gdsp_clump_work (uint32_t n);
int gdsp_clump        (double* d_v, uint32_t n, double average, uint32_t minLength, int above,
                       double one, double zero, void* d_work, void* stream);
/* add.c:909-923 / percentile.c:434-530: d_minmax[0]=min(d_minmax[0], min over sample),
 * d_minmax[1]=max(...), d_minmax[2]+=count (as double); sample = every window-th value
 * with lo <= v <= hi.  Initialise with gdsp_minmax_init. */
int gdsp_minmax_init   (double* d_minmax, void* stream);
int gdsp_minmax_update (const double* d_v, uint32_t n, uint32_t window, double lo, double hi,
                        double* d_minmax, void* stream);

/* ---- percentile.c:392-751 -------------------------------------------------------- */

/* Exact order statistic by radix select on the order-preserving 64-bit image of
 * the doubles (-0.0 folded onto +0.0: the reference's comparator, genodsp.c:2262-2270,
 * cannot tell them apart).  The signal is left untouched (the reference scrambles
 * it, percentile.c:34-36).  One pass = gdsp_select_hist_init, then one
 * gdsp_select_histogram per chromosome on each GPU, then a SUM of the bins over
 * GPUs (min/max of the two trailing words) -- the only collective on the whole
 * path -- then gdsp_select_pick on the host to find the bucket holding rank k.
 *   sample  : every window-th value with !(v < lo) && !(v > hi)   (percentile.c:559-561)
 *   digit   : key bits [shift, shift+bits), bits <= GDSP_SELECT_MAX_BITS
 *   prefix  : only keys whose bits above the digit equal prefix's are counted
 *   d_hist  : (1<<bits) u64 counts, then the smallest and the largest matching key
 *             (when those two are equal every remaining candidate is that value). */
#define GDSP_SELECT_MAX_BITS 13
int gdsp_select_hist_init (uint64_t* d_hist, int bits, void* stream);
int gdsp_select_histogram (const double* d_v, uint32_t n, uint32_t window, double lo, double hi,
                           int shift, int bits, uint64_t prefix, uint64_t* d_hist, void* stream);
/* Host: bucket holding 0-based rank k among the counted keys, and the rank inside it. */
int gdsp_select_pick      (const uint64_t* h_hist, int bits, uint64_t k, uint32_t* bucket, uint64_t* kWithin);
/* Host: key image <-> double */
double   gdsp_key_to_double (uint64_t key);
uint64_t gdsp_double_to_key (double v);
/* Host: the reference's rank formula, percentile.c:587-589 and :688-710 */
uint32_t gdsp_percentile_rank (uint32_t numValues, uint32_t pThousandths);

/* op_percentile_apply (percentile.c:392-751) end to end: the exact percentiles of the sampled
 * genome -- every window-th value v with !(v < lo) && !(v > hi) of every source vector --
 * non-destructive.  values[i] = the order statistic of rank gdsp_percentile_rank(count, p[i]);
 * *count = the population size (0: nothing qualifies, values untouched).
 * Sources may sit on several devices of this process (the counts are added on the host); with
 * one process per GPU pass `reduce`, which must replace words[0..count) by their sum (op 0),
 * minimum (op 1) or maximum (op 2) over all ranks and return 0 -- every rank then takes the same
 * decisions and gets the same values.  That reduction (a few KiB per step) is the path's only
 * collective.
 * strategy: AUTO brackets the ranks with pivots from a strided subsample of `sampleTarget`
 * values (0 = one value in 1024, between 2^16 and 2^20) and settles all percentiles in one counting pass over the
 * population when it is larger than 2^20 (or than an explicit sampleTarget), RADIX is five histogram passes per percentile (the fallback of AUTO
 * whenever a bracket misses), BRACKET forces the first route (tests). */
typedef struct gdsp_select_source { const double* d_v; uint32_t n; int device; void* stream; } gdsp_select_source;
typedef int (*gdsp_reduce_fn) (void* ctx, uint64_t* words, size_t count, int op);
#define GDSP_SELECT_AUTO    0
#define GDSP_SELECT_RADIX   1
#define GDSP_SELECT_BRACKET 2
int gdsp_percentiles (const gdsp_select_source* sources, int nsources, uint32_t window, double lo, double hi,
                      const uint32_t* pThousandths, int npercentiles, int strategy, uint32_t sampleTarget,
                      gdsp_reduce_fn reduce, void* reduceCtx, double* values, uint64_t* count);
/* The path's only collective (gdsp_comm.hip): all-reduce of the counters across the GPUs of one node, RCCL over
 * xGMI.  One process drives several devices: gdsp_comm_create makes one RCCL communicator per device
 * (ncclCommInitAll; RCCL is dlopen'ed on first use, a one-GPU run never loads it) and the all-reduces run in place
 * on d_bufs[rank] -- rank r is devices[r] -- on streams[rank] (NULL: that device's default stream).  op: 0 sum,
 * 1 min, 2 max.  Replaces, for chromosomes dealt over GPUs, what the reference's single thread sees at once:
 * percentile.c:547-683 (the sort of the sampled genome), add.c:909-923 (invert's global min / max). */
typedef struct gdsp_comm gdsp_comm;
int gdsp_comm_create        (gdsp_comm** comm, const int* devices, int ndevices);
int gdsp_comm_destroy       (gdsp_comm* comm);
int gdsp_comm_size          (const gdsp_comm* comm);
int gdsp_comm_device        (const gdsp_comm* comm, int rank);
int gdsp_comm_rccl_version  (int* version);
int gdsp_comm_allreduce_u64 (gdsp_comm* comm, uint64_t* const* d_bufs, size_t count, int op, void* const* streams);
int gdsp_comm_allreduce_f64 (gdsp_comm* comm, double* const* d_bufs, size_t count, int op, void* const* streams);
/* gdsp_percentiles over the devices of THIS process: all-reduce its histograms and counters in HBM through `comm`
 * (whose devices must be the sources' devices) instead of adding host copies; NULL switches back. */
int gdsp_percentiles_use_comm (gdsp_comm* comm);
/* gdsp_percentiles with one process per GPU: hand every buffer to be reduced to the caller as DEVICE words on the
 * stream the counts were produced on (the caller runs its collective there, e.g. torch.distributed over RCCL, and
 * returns 0); NULL switches back to the host hook of gdsp_percentiles.  op as above. */
typedef int (*gdsp_device_reduce_fn) (void* ctx, uint64_t* d_words, size_t count, int op, void* stream);
int gdsp_percentiles_use_device_reduce (gdsp_device_reduce_fn fn, void* ctx);

/* `= percentile P = binarize --threshold=percentileP` (percentile.c:392-751 feeding logical.c:216-268) in ONE read of the
 * signal: the counting pass knows the bracket the percentile lies in before it knows the percentile, so it writes
 * one / zero for every base outside that bracket as it counts and queues the positions inside it (0.1 % of real-valued
 * coverage) for a fix-up once the value is known -- 16 B/base for the pair instead of 24.  d_out[i] receives
 * binarize(source i) against values[which] (out of place: the sources are left intact); *onePass = 1 when every source
 * went that way, 0 when some (or all) were binarized by a pass of their own -- strided sampling (window > 1), the radix
 * route, a percentile that fell outside its bracket, more than n/16 bases inside the bracket.  Same values, same
 * outputs either way.  *count = 0 (nothing qualifies): no output is written. */
typedef struct gdsp_percentile_binarize { int which;  int tiesAbove;  double one, zero;  double* const* d_out; } gdsp_percentile_binarize;
int gdsp_percentiles_binarize (const gdsp_select_source* sources, int nsources, uint32_t window, double lo, double hi,
                               const uint32_t* pThousandths, int npercentiles, int strategy, uint32_t sampleTarget,
                               gdsp_reduce_fn reduce, void* reduceCtx, double* values, uint64_t* count,
                               const gdsp_percentile_binarize* fuse, int* onePass);

/* what the last gdsp_percentiles call of this process did: [0] route taken (GDSP_SELECT_RADIX or
 * _BRACKET), [1] population, [2] subsample size, [3] candidates kept on this rank, [4] percentiles
 * that fell back to the radix route, [5] histogram passes over the population, [6] 1 when a fused binarize
 * was settled in the counting pass for every source, [7] 1 when the call was decided on the device with one read-back
 * (one device, nothing to reduce with; GDSP_PERCENTILE_RESIDENT_OFF forbids it) */
void gdsp_percentiles_stats (uint64_t out[8]);

/* ---- stats / normalize (not in the reference): genome-wide sum, mean and variance, exact and rounded once --------
 * The sample is percentile's: every window-th value counted from each chromosome's first base whose value v satisfies
 * !(v < lo) && !(v > hi), non-finite values never; n is its size.  sum = the exact sum rounded once to nearest-even (it
 * may round to +-inf; an exact zero is +0.0).  mean = the exact sum / n rounded once (not sum / n: always finite).
 * variance = the exact (sum over the sample of q) / n rounded once, q = fl(fl(v - mean)^2) without fma; +inf when some
 * q is.  stddev = sqrt(variance).  None of them depends on how the genome is cut into vectors, stretches, devices or
 * ranks, nor on tiles, grid or dispatch order (gdsp_xsum.hip).
 *
 * The accumulator: GDSP_XSUM_WORDS u64 words.  Word k < GDSP_XSUM_DIGITS is a signed (two's complement) multiple of
 * 2^(32k - 1074); the value is the sum of them all (2^-1074 .. 2^1102).  GDSP_XSUM_WORD_COUNT counts the sampled values,
 * GDSP_XSUM_WORD_INF the q that are +inf (pass 2), GDSP_XSUM_WORD_FLUSHES the times a lane's register expansion handed
 * a residual to the workgroup's integer image (a diagnostic: it depends on the cut).  Images add as plain u64 SUMs
 * (all-reduce them with op 0); each accumulate call grows a word by less than 2^43.
 * A source is d_v[0 .. n) (8-byte aligned, on the current device for the *_batch calls); `first` is the chromosome
 * position of d_v[0], so that the window counts from the chromosome's first base whatever stretch the source is. */
#define GDSP_XSUM_DIGITS       68
#define GDSP_XSUM_WORD_COUNT   68
#define GDSP_XSUM_WORD_INF     69
#define GDSP_XSUM_WORD_FLUSHES 70
#define GDSP_XSUM_WORDS        72
typedef struct gdsp_xsum_source { const double* d_v; uint32_t n; uint32_t first; int device; void* stream; } gdsp_xsum_source;
int gdsp_xsum_init (uint64_t* d_acc, void* stream);                                  /* zero an accumulator */
/* pass 1: add every sampled v of every source to d_acc (one launch per 32 sources) */
int gdsp_xsum_accumulate_batch    (const gdsp_xsum_source* sources, int nsources, uint32_t window, double lo, double hi,
                                   uint64_t* d_acc, void* stream);
/* pass 2: add fl(fl(v - mean)^2) of every sampled v (mean finite) */
int gdsp_xsum_accumulate_sq_batch (const gdsp_xsum_source* sources, int nsources, uint32_t window, double lo, double hi,
                                   double mean, uint64_t* d_acc, void* stream);
/* carry the digits into canonical form (0 <= digit < 2^32 below the top one, which keeps the sign): equal values give
 * equal words, and up to 2^31 canonical images add without overflow */
int gdsp_xsum_fold (uint64_t* d_acc, void* stream);
/* Host, no GPU: add a finite x to a host image (and 1 to its count; non-finite x are ignored); the image's value rounded
 * once (+inf when the INF word is set); the value / n rounded once (NaN for n == 0, +inf when the INF word is set).
 * The image may be canonical or not. */
void   gdsp_xsum_add_host  (uint64_t* h_acc, double x);
double gdsp_xsum_round     (const uint64_t* h_acc);
double gdsp_xsum_div_round (const uint64_t* h_acc, uint64_t n);
/* end to end: out[0..4] = count, sum, mean, variance, stddev (count 0: sum 0 and the rest NaN).  Sources may sit on
 * several devices of this process (each device's work is queued on the stream of its first source; the images are
 * added on the host, or all-reduced in HBM through the communicator given to gdsp_genome_stats_use_comm, whose devices
 * must then be the sources' devices); with one process per GPU pass `reduce` (op 0 = sum of the u64 words over all
 * ranks), as for gdsp_percentiles.  Two passes over the signal; waits for them. */
int gdsp_genome_stats (const gdsp_xsum_source* sources, int nsources, uint32_t window, double lo, double hi,
                       gdsp_reduce_fn reduce, void* reduceCtx, double* out);
int gdsp_genome_stats_use_comm (gdsp_comm* comm);     /* NULL switches back to host sums */
/* what the last gdsp_genome_stats did: [0] n, [1] lane flushes of pass 1, [2] of pass 2, [3] q that were +inf */
void gdsp_genome_stats_last (uint64_t out[4]);

/* ---- correlate (not in the reference): the signal against a second track -- covariance, Pearson r, regression ------
 * A pair source is x = d_x[0 .. n) and y = d_y[0 .. n), with `first`, `device` and `stream` as in gdsp_xsum_source.  Both
 * pointers are 8-byte aligned; their 16-byte alignment may differ (a y that is congruent to x modulo 16 bytes is read
 * with the same 16-byte loads; any other y is read value by value: as exact, slower).
 * The pair sample is every window-th position, counted from the chromosome's first base as for stats, that passes all of
 *   !(x < lo) && !(x > hi), x finite, !(y < ylo) && !(y > yhi), y finite;          n is its size.
 * Pass 1: the exact sums Sx, Sy over the pair sample.  sumx, sumy are those sums rounded once; meanx = Sx / n and
 *   meany = Sy / n, each rounded once (gdsp_xsum_div_round).
 * Pass 2: per pair dx = fl(x - meanx), dy = fl(y - meany), qxx = fl(dx dx), qyy = fl(dy dy), qxy = fl(dx dy), without
 *   fma (the rule of stats' q), each of the three summed exactly.  A q that is not finite (qxx, qyy = +inf; qxy = +-inf,
 *   or NaN from inf * 0) is counted in its image's GDSP_XSUM_WORD_INF and not added.
 *   varx = (sum of qxx) / n rounded once, +inf when some qxx was not finite; vary likewise;
 *   cov  = (sum of qxy) / n rounded once, NaN when some qxy was not finite;  sdx = sqrt (varx), sdy = sqrt (vary).
 *   (The three overflow separately: x alternating +-DBL_MAX against y = 1, 2, 1, 2, ... has every qxx = +inf but every
 *   qxy = fl(+-DBL_MAX * -+0.5) finite, so varx is +inf and cov is -DBL_MAX/2, not NaN; against y = 1, 5, 1, 5, ...
 *   every qxy is -inf and cov is NaN.)
 * The rest is derived on the host, in plain IEEE double, from those once-rounded figures, so it too is a function of
 * the pair sample alone -- not of the cut into pairs, devices or ranks, of tiles, grid or dispatch order:
 *   correlation: (mx, ex) = frexp (sdx), (my, ey) = frexp (sdy), r = ldexp (cov, -(ex + ey)) / fl(mx my), clamped to
 *     [-1, 1]: symmetric in x and y, no spurious overflow or underflow.  NaN when n = 0, when varx or vary is 0 or not
 *     finite, or when cov is NaN.
 *   slope = fl(cov / varx), intercept = fl(meany - fl(slope meanx)): y regressed on x.  NaN when varx is 0 or not
 *     finite, or when cov is NaN.
 *   n = 0: both sums are +0.0 and everything else is NaN.
 * Agreement with stats: when every sampled y is admitted (finite and within ylo, yhi), count, sumx, meanx, varx and sdx
 *   are bit for bit what gdsp_genome_stats gives for x with the same window, lo and hi.
 * Symmetry: swapping x and y, and their limits, swaps the x and y figures; cov and correlation keep the same bits.
 *
 * The accumulators are GDSP_XSUM_WORDS images side by side: 2 for pass 1 (Sx, Sy), 3 for pass 2 (qxx, qyy, qxy).  Each
 * image's count word holds n, and each has its own INF and FLUSHES words.  gdsp_xsum_init and gdsp_xsum_fold act on
 * one image: call them per image (d_acc + k * GDSP_XSUM_WORDS). */
typedef struct gdsp_xsum_pair { const double* d_x; const double* d_y; uint32_t n; uint32_t first; int device; void* stream; } gdsp_xsum_pair;
uint32_t gdsp_xsum_pair_tile (void);                  /* pairs per tile of the kernel's walk (what tests size their shapes by) */
/* pass 1 into 2 images, pass 2 (means finite) into 3; one launch per 32 pairs, all on the current device */
int gdsp_xsum_pair_accumulate_batch     (const gdsp_xsum_pair* pairs, int npairs, uint32_t window, double lo, double hi,
                                         double ylo, double yhi, uint64_t* d_acc, void* stream);
int gdsp_xsum_pair_accumulate_dev_batch (const gdsp_xsum_pair* pairs, int npairs, uint32_t window, double lo, double hi,
                                         double ylo, double yhi, double meanx, double meany, uint64_t* d_acc, void* stream);
/* end to end, like gdsp_genome_stats (several devices, the communicator of gdsp_genome_correlation_use_comm, or the
 * `reduce` hook, called once per pass over the images side by side: 144 words, then 216).  The figure order: */
enum { GDSP_CORR_COUNT = 0, GDSP_CORR_SUMX, GDSP_CORR_SUMY, GDSP_CORR_MEANX, GDSP_CORR_MEANY, GDSP_CORR_VARX, GDSP_CORR_VARY,
       GDSP_CORR_SDX, GDSP_CORR_SDY, GDSP_CORR_COV, GDSP_CORR_CORRELATION, GDSP_CORR_SLOPE, GDSP_CORR_INTERCEPT,
       GDSP_CORR_FIGURES };                           /* out[13]: count, sumx, sumy, meanx, meany, varx, vary, sdx, sdy,
                                                         covariance, correlation, slope, intercept */
int gdsp_genome_correlation (const gdsp_xsum_pair* pairs, int npairs, uint32_t window, double lo, double hi,
                             double ylo, double yhi, gdsp_reduce_fn reduce, void* reduceCtx, double* out);
int gdsp_genome_correlation_use_comm (gdsp_comm* comm);   /* NULL switches back to host sums */
/* what the last gdsp_genome_correlation did: [0] n, [1] lane flushes of pass 1 (both images), [2] of pass 2 (all three),
 * [3] qxx, [4] qyy, [5] qxy that were not finite, [6] and [7] zero */
void gdsp_genome_correlation_last (uint64_t out[8]);

/* ---- crosscorrelate / autocorrelate (not in the reference): the covariance and correlation at every lag of a range ---
 * A genome is a list of pairs (x_c, y_c) of WHOLE chromosome vectors of length L_c (gdsp_xsum_pair; `first` is ignored).
 * Lagged pairs never cross a chromosome's end or join two chromosomes.
 * N, meanx, meany, varx, vary, sdx, sdy are exactly gdsp_genome_correlation's figures for these pairs with window 1 and
 *   no limits: the sample is the bases where x and y are both finite.
 * For an integer lag d, with dx = fl(x - meanx) and dy = fl(y - meany):
 *   Q(d) = sum over c, and over the i with 0 <= i < L_c, 0 <= i+d < L_c, x_c[i] and y_c[i+d] both finite, of
 *          fl(dx_c[i] * dy_c[i+d]):  each product one rounding, never contracted; the sum exact.
 *   A product that is not finite is counted in that lag's GDSP_XSUM_WORD_INF word and not added.  The count word of lag
 *   d's image holds the number of products taken, n(d) (those that were not finite included).
 *   covariance(d) = Q(d) / N rounded once (gdsp_xsum_div_round); NaN when some product of that lag was not finite.  The
 *     division is by N, not by n(d): the estimator of time-series software (R's acf / ccf), which needs no per-lag means,
 *     and whose curve is a positive semi-definite sequence for y = x.  A lag no chromosome is long enough for gives +0.0.
 *   correlation(d): from covariance(d), sdx, sdy by the frexp / ldexp rule of correlate, clamped to [-1, 1]; NaN when
 *     varx or vary is 0 or not finite, or when covariance(d) is NaN.
 *   N = 0: every count is 0 and every covariance and correlation is NaN.
 * Consequences, bit for bit: lag 0 gives correlate's covariance and correlation; swapping x and y maps lag d to -d; with
 *   y = x the curve is symmetric in d, and lag 0 is the variance and 1 (or NaN).  Nothing depends on chromosome order, on
 *   which device holds which chromosome, on grid, tile, lag block or dispatch order.
 *
 * gdsp_lag_products_batch adds every pair's products into nlags images of GDSP_XSUM_WORDS words side by side, lag
 * lagLo + k in image k, and leaves the images in canonical digits (they add as plain u64 sums).  nlags is 1 .. 4096, the
 * lags any int32; the means are finite; the pairs are on the current device, one launch per 32 of them.  d_acc is zeroed
 * by the caller.  gdsp_lag_tile () positions by gdsp_lag_block () lags are staged at a time (what tests size their shapes
 * by).  The cost is N * nlags products of 13 rounded operations each: a genome at a few hundred lags takes on the order
 * of a second. */
uint32_t gdsp_lag_tile  (void);
uint32_t gdsp_lag_block (void);
int gdsp_lag_products_batch (const gdsp_xsum_pair* pairs, int npairs, int32_t lagLo, uint32_t nlags, double meanx, double meany,
                             uint64_t* d_acc, void* stream);
/* end to end: fig[GDSP_CORR_FIGURES] by gdsp_genome_correlation (its hook calls, then one more over the nlags * 72 words
 * of the lag images), then count[k] = n(lagLo + k), cov[k], corr[k].  Devices, communicator and hook as for
 * gdsp_genome_correlation. */
int gdsp_genome_lag_correlation (const gdsp_xsum_pair* pairs, int npairs, int32_t lagLo, uint32_t nlags, gdsp_reduce_fn reduce,
                                 void* reduceCtx, double* fig, uint64_t* count, double* cov, double* corr);
int gdsp_genome_lag_correlation_use_comm (gdsp_comm* comm);   /* NULL switches back to host sums */
/* what the last gdsp_genome_lag_correlation did: [0] N, [1] products taken (all lags), [2] lane flushes into the device
 * images, [3] products that were not finite, [4] .. [7] zero */
void gdsp_genome_lag_correlation_last (uint64_t out[8]);

/* ---- profileover (not in the reference): the signal's figures at every offset from a list of anchors, exact ----------
 * A genome is a list of WHOLE chromosome vectors.  An anchor is (vector, position p, strand s) with 0 <= p < n of its
 * vector and s = +1 or -1.  For an integer offset k the anchor looks at base g = p + s k of its vector; the pair
 * (anchor, k) is sampled iff 0 <= g < n and v[g] passes stats' test: finite, and !(v < lo) && !(v > hi).  An anchor whose
 * window leaves its chromosome contributes the offsets that stay inside; a duplicated anchor contributes twice; nothing
 * crosses a chromosome's end or joins two chromosomes.
 * The offsets are the range offLo .. offLo + noffsets - 1: noffsets is 1 .. GDSP_PROFILE_MAX_OFFSETS, offLo any int32 for
 * which the range stays in int32.  A bin width b >= 1 divides noffsets; column j is the sample of all the pairs
 * (anchor, k) with offLo + j b <= k < offLo + (j+1) b.  Per column, exactly what gdsp_genome_stats defines for that sample:
 *   count     the number of pairs sampled;
 *   sum       the exact sum rounded once (an exact zero is +0.0);
 *   mean      the exact sum divided by count, rounded once;
 *   variance  the exact (sum of q) / count rounded once, q = fl(fl(v - mean)^2) without fma against the column's own mean;
 *             +inf when some q is;   stddev = sqrt (variance).
 *   count == 0: sum is +0.0 and the rest is NaN.
 *   (stderr = fl(stddev / sqrt ((double) count)) is the caller's to derive.)
 * Every figure is a function of the column's sample alone: nothing depends on the order of the anchors or of the
 * chromosomes, on which device holds which chromosome, on grid, offset block, launch chunking or dispatch order.
 *
 * gdsp_profile_accumulate_batch adds the sampled values of every anchor into noffsets images of GDSP_XSUM_WORDS words side
 * by side, offset offLo + k in image k -- always at base resolution: a column's image is the plain u64 sum of its b
 * offsets' images -- and leaves the images in canonical digits.  The vectors are items[i] (d_in and n are read) on the
 * current device, 8-byte aligned; anchor i is position d_pos[i] of vector d_code[i] >> 1, minus strand when d_code[i] & 1:
 * DEVICE arrays of `count` entries, any order.  d_mean == NULL is pass 1 (the values themselves); otherwise pass 2, which
 * adds fl(fl(v - d_mean[k])^2) for offset offLo + k (a DEVICE array of noffsets means: a column's mean at each of its
 * offsets; the mean of an offset that samples nothing is not used) and counts a q that is not finite in the image's
 * GDSP_XSUM_WORD_INF instead of adding it.  d_acc is zeroed by the caller.  One launch sequence per 32 vectors; within
 * it the anchors go in launches short enough that no image word can overflow before it is carried
 * (gdsp_profile_set_launch_anchors lowers that number so that tests can force several launches; 0 restores it).
 * GDSP_EINVAL for a bad range or an anchor outside its vector (decided on the device: the call waits for the stream once).
 * gdsp_profile_block () offsets belong to one workgroup (what tests size their shapes by). */
#define GDSP_PROFILE_MAX_OFFSETS 16384
uint32_t gdsp_profile_block (void);
int gdsp_profile_set_launch_anchors (uint32_t anchors);
int gdsp_profile_accumulate_batch (const gdsp_batch_item* items, int nitems, const uint32_t* d_pos, const uint32_t* d_code,
                                   uint32_t count, int32_t offLo, uint32_t noffsets, double lo, double hi, const double* d_mean,
                                   uint64_t* d_acc, void* stream);
/* end to end, like gdsp_genome_lag_correlation: a source is a whole chromosome d_v[0 .. n) on `device` with its anchors as
 * HOST arrays (h_pos[i] < n; h_minus[i] != 0 is the minus strand, h_minus == NULL all plus).  Sources may sit on several
 * devices of this process (communicator and hook as for gdsp_genome_stats; the `reduce` hook is called once per pass
 * over the noffsets * 72 words, and not for pass 2 when no column sampled anything).  count, sum, mean, variance, stddev:
 * HOST arrays of noffsets / bin columns. */
typedef struct gdsp_profile_source { const double* d_v; uint32_t n; int device; void* stream;
                                     const uint32_t* h_pos; const uint32_t* h_minus; uint32_t nanchors; } gdsp_profile_source;
int gdsp_genome_profile (const gdsp_profile_source* sources, int nsources, int32_t offLo, uint32_t noffsets, uint32_t bin,
                         double lo, double hi, gdsp_reduce_fn reduce, void* reduceCtx, uint64_t* count, double* sum,
                         double* mean, double* variance, double* stddev);
int gdsp_genome_profile_use_comm (gdsp_comm* comm);   /* NULL switches back to host sums */
/* what the last gdsp_genome_profile did: [0] anchors, [1] samples taken (all offsets), [2] lane flushes into the device
 * images (both passes), [3] q that were not finite */
void gdsp_genome_profile_last (uint64_t out[4]);

/* ---- matrixover (not in the reference): the signal around each anchor of a list, one row per anchor, exact -----------
 * Anchors, offsets and bins are profileover's: an anchor is (vector, position p, strand s) with 0 <= p < n of its WHOLE
 * chromosome vector; the offsets are offLo .. offLo + noffsets - 1 (1 .. GDSP_PROFILE_MAX_OFFSETS of them, the range inside
 * int32); a bin b >= 1 divides noffsets and ncols = noffsets / b; offset k of an anchor looks at base p + s k.  Nothing is
 * added up over the anchors here: the CELL (anchor, column j) is the set of bases p + s k, offLo + j b <= k <
 * offLo + (j+1) b, that lie in [0, n) -- one interval of the chromosome, possibly empty; for a minus anchor column 0 holds
 * the highest bases.  A cell's figures are exactly what the statsover section below defines for that interval and the
 * limits lo, hi: count; sum (the exact sum rounded once, an exact zero +0.0); mean (the exact sum over count, rounded
 * once); min and max (a zero result is +0.0); an empty sample has count 0, sum +0.0 and mean, min, max NaN.  One call
 * computes ONE figure, `what`, as one double per cell (a count is exact in a double).  Each value is a function of its
 * cell's sample alone: nothing depends on the launch split, grid, dispatch order or devices, on chromosome order or on
 * the order of the anchors; a duplicated anchor gives two equal rows; nothing crosses a chromosome's end.
 *
 * gdsp_matrix_rows_batch writes the rows of `count` anchors -- items, d_pos and d_code as gdsp_profile_accumulate_batch
 * takes them -- into d_out, count x ncols doubles, row-major, in the anchors' order (at most 2^32 - 1 cells).  A cell the
 * device cannot finish exactly (a lane's two-term expansion was flagged or overflowed; a mean it cannot prove to be
 * rounded once) is left to the caller: its index row * ncols + column is appended to d_todo (room for count x ncols entries)
 * and counted in *d_ntodo, which the caller zeroes; what d_out holds there means nothing.  count, min and max are always
 * finished, and so is every figure of integer read depth whose sums stay below 2^53.  One launch sequence per 32 vectors.
 * GDSP_EINVAL for a bad range, a bin that does not divide noffsets, a figure that is none of the five, or an anchor
 * outside its vector (decided on the device: the call waits for the stream once).
 * gdsp_genome_matrix is the host half over profileover's source table: per device it uploads the anchors, launches
 * bounded pieces (at most 2^25 cells of device output per launch; gdsp_matrix_set_launch_rows lowers the rows of a
 * piece so that tests can force several, 0 restores the library's own number), reads the rows back into h_rows[i]
 * (a HOST array of sources[i].nanchors x ncols doubles, in that source's anchor order) and computes the to-do cells with
 * gdsp_interval_stats_batch over their intervals, which is exact on any input.  Nothing is reduced across devices. */
#define GDSP_MATRIX_MEAN  0
#define GDSP_MATRIX_SUM   1
#define GDSP_MATRIX_COUNT 2
#define GDSP_MATRIX_MIN   3
#define GDSP_MATRIX_MAX   4
int gdsp_matrix_rows_batch (const gdsp_batch_item* items, int nitems, const uint32_t* d_pos, const uint32_t* d_code, uint32_t count,
                            int32_t offLo, uint32_t noffsets, uint32_t bin, int what, double lo, double hi, double* d_out,
                            uint32_t* d_todo, uint32_t* d_ntodo, void* stream);
int gdsp_genome_matrix (const gdsp_profile_source* sources, int nsources, int32_t offLo, uint32_t noffsets, uint32_t bin, int what,
                        double lo, double hi, double* const* h_rows);
int gdsp_matrix_set_launch_rows (uint32_t rows);
/* what the last gdsp_genome_matrix did: [0] rows, [1] cells, [2] cells the host finished, [3] launches */
void gdsp_genome_matrix_last (uint64_t out[4]);

/* ---- regionsover (not in the reference): every region of a list scaled to the same columns, one row per region, exact --
 * The other half of matrixover (deepTools' computeMatrix scale-regions).  A region is (vector, [s, e), strand) with
 * 0 <= s < e <= n of its WHOLE chromosome vector and L = e - s.  A row has U / b + B + D / b columns in the region's own
 * direction: the upstream flank of U bases in columns of b, the body in B columns, the downstream flank of D bases in
 * columns of b.  1 <= B <= GDSP_REGIONS_MAX_COLUMNS; U, D <= GDSP_REGIONS_MAX_COLUMNS; b >= 1 divides both; at most
 * GDSP_REGIONS_MAX_COLUMNS columns.  In integers, on the plus strand:
 *   body column k        the bases [s + floor (k L / B), s + floor ((k+1) L / B)): the B cells partition [s, e), each of
 *                        floor (L / B) or ceil (L / B) bases, and with L < B some are empty;
 *   upstream column j    [s - U + j b, s - U + (j+1) b);     downstream column j    [e + j b, e + (j+1) b);
 *   a flank cell is cut to [0, n) (a region itself is never cut: one that leaves its vector is refused).
 * The minus strand is the mirror image about the region: body column k is [e - floor ((k+1) L / B), e - floor (k L / B)),
 * upstream lies above e and downstream below s.  A CELL is thus one interval of the chromosome, possibly empty, and its
 * figures are matrixover's, that is statsover's for that interval under the limits lo, hi; one call computes one figure
 * GDSP_MATRIX_*; an empty cell has count 0, sum +0.0 and mean, min, max NaN.  Each value is a function of its cell's
 * sample alone: nothing depends on the launch split, grid, dispatch order, devices or the order of the regions.
 *
 * gdsp_region_cell_bounds is that definition on the host, without a device: [*lo, *hi) of one column, cut to [0, n)
 * (*lo >= *hi: empty) -- the same function the kernel and the host half use.
 * gdsp_region_rows_batch writes the rows of `count` regions that are on the device already -- d_start, d_end and d_code
 * (vector * 2 + minus, as an anchor's) DEVICE arrays, items as gdsp_matrix_rows_batch takes them -- into d_out, count x
 * ncols doubles, row-major; d_todo and d_ntodo as there.  GDSP_EINVAL for a bad shape or a region that is not
 * s < e <= n of one of the items (decided on the device: the call waits for the stream once; no kernel follows).
 * gdsp_genome_regions is the host half: a source is a whole chromosome on `device` with its regions as HOST arrays; per
 * device it uploads them, launches bounded pieces (at most 2^25 cells each; gdsp_regions_set_launch_rows lowers the rows
 * of a piece for tests, 0 restores), reads the rows back into h_rows[i] (sources[i].nregions x ncols doubles) and
 * computes the to-do cells with gdsp_interval_stats_batch. */
#define GDSP_REGIONS_MAX_COLUMNS 16384
typedef struct gdsp_region_source { const double* d_v; uint32_t n; int device; void* stream;
                                    const uint32_t* h_start; const uint32_t* h_end; const uint32_t* h_minus;
                                    uint32_t nregions; } gdsp_region_source;
int gdsp_region_cell_bounds (uint32_t n, uint32_t start, uint32_t end, int minus, uint32_t B, uint32_t U, uint32_t D, uint32_t b,
                             uint32_t column, int64_t* lo, int64_t* hi);
int gdsp_region_rows_batch (const gdsp_batch_item* items, int nitems, const uint32_t* d_start, const uint32_t* d_end,
                            const uint32_t* d_code, uint32_t count, uint32_t B, uint32_t U, uint32_t D, uint32_t b, int what,
                            double lo, double hi, double* d_out, uint32_t* d_todo, uint32_t* d_ntodo, void* stream);
int gdsp_genome_regions (const gdsp_region_source* sources, int nsources, uint32_t B, uint32_t U, uint32_t D, uint32_t b, int what,
                         double lo, double hi, double* const* h_rows);
int gdsp_regions_set_launch_rows (uint32_t rows);
/* what the last gdsp_genome_regions did: [0] rows, [1] cells, [2] cells the host finished, [3] launches */
void gdsp_genome_regions_last (uint64_t out[4]);

/* ---- statsover (not in the reference): one signal quantified over many intervals, exact ---------------------------
 * For a vector v of n doubles, an interval [s, e) with 0 <= s < e <= n, and limits lo, hi:
 *   the sample of the interval is stats' sample restricted to it: the bases i in [s, e) with !(v[i] < lo) &&
 *     !(v[i] > hi) and v[i] finite (never NaN, never +-inf).  There is no window here.
 *   count   the number of sampled bases;
 *   sum     the exact sum of the sample, rounded once (+-inf only when the rounded value is beyond DBL_MAX);
 *   mean    the exact sum divided by count, rounded once -- the two figures gdsp_genome_stats gives for that sample;
 *   min, max  the least and greatest sampled value as IEEE compares them; a result that is a zero is +0.0;
 *   maxpos  the lowest i in the sample with v[i] == max (the summit);
 *   count == 0: sum is +0.0, and mean, min, max are NaN and maxpos is UINT32_MAX.
 * Every figure is a function of the sample alone: nothing depends on tiles, grid, dispatch order, the order of the
 * intervals or how they overlap.  (No variance per interval: it would take a second pass against each interval's mean.)
 *
 * The calls take the intervals as HOST arrays (any order, overlapping and duplicate intervals allowed; start < end <= n
 * or GDSP_EINVAL), read the signal on the current device without modifying it, wait for the device, and fill a HOST
 * array of records in the caller's order.  The batch form covers every vector of a device in one launch: interval i
 * lies on vector items[h_vec[i]] (d_in and n of an item are read; h_vec == NULL: all on items[0]).  Vectors must be
 * 8-byte aligned.  The device reduces pieces -- an interval cut at multiples of gdsp_interval_stats_tile() values of
 * the 16-byte aligned frame its vector lies in -- to records (a0 + a1 is the piece's exact sum unless `flag` says a
 * lane's two-term expansion could not hold it; such a piece is summed again through gdsp_xsum_accumulate_batch), and
 * gdsp_interval_stats_combine, host code that needs no GPU, turns an interval's pieces into its figures: `images` holds
 * one GDSP_XSUM_WORDS image per flagged piece, in the pieces' order (NULL when none is flagged).  A record's `image` is 1
 * when its sum and mean were rounded from the integer image and not from two doubles (a diagnostic). */
typedef struct gdsp_interval_stat  { uint64_t count;  double sum, mean, min, max;  uint32_t maxpos, image; } gdsp_interval_stat;
typedef struct gdsp_interval_piece { double a0, a1, min, max;  uint32_t count, maxpos, flag, reserved; } gdsp_interval_piece;
uint32_t gdsp_interval_stats_tile (void);
int gdsp_interval_stats_set_launch_pieces (uint32_t pieces);       /* for tests: the most pieces of one launch (0: the default) */
int gdsp_interval_stats       (const double* d_v, uint32_t n, const uint32_t* h_start, const uint32_t* h_end, uint32_t count,
                               double lo, double hi, gdsp_interval_stat* h_out, void* stream);
int gdsp_interval_stats_batch (const gdsp_batch_item* items, int nitems, const uint32_t* h_vec, const uint32_t* h_start,
                               const uint32_t* h_end, uint32_t count, double lo, double hi, gdsp_interval_stat* h_out, void* stream);
int gdsp_interval_stats_combine (const gdsp_interval_piece* pieces, uint32_t npieces, const uint64_t* images, gdsp_interval_stat* out);
/* what the last gdsp_interval_stats[_batch] did: [0] intervals, [1] pieces, [2] flagged pieces (summed again), [3] intervals
 * whose sum went through the integer image; and where its time went, in ms: [0] cutting the intervals into pieces (host),
 * [1] the kernel (HIP events), [2] copies, waiting and flagged pieces, [3] combining the pieces (host) */
void gdsp_interval_stats_last  (uint64_t out[4]);
void gdsp_interval_stats_times (double ms[4]);

/* ---- percentilesover / medianover (not in the reference): exact order statistics of every interval ----------------
 * What statsover leaves out: the figures of an interval that take more than one reduction.  For a vector v of n doubles,
 * an interval [s, e) with 0 <= s < e <= n, limits lo, hi and percentiles P_0 .. P_{q-1} in thousandths of a percent
 * (0..100000, 1 <= q <= GDSP_INTERVAL_PERCENTILES_MAX):
 *   the sample is statsover's: the bases i in [s, e) with !(v[i] < lo) && !(v[i] > hi) and v[i] finite;
 *   count    m, the number of sampled bases;
 *   value_j  for each P_j, with k_j = gdsp_percentile_rank(m, P_j): gdsp_key_to_double of the k_j-th smallest (from 0)
 *            of the keys gdsp_double_to_key(v[i]) over the sample -- the order `percentile` and `slidingpercentile`
 *            use.  The value is an input value bit for bit, -0.0 folded onto +0.0.  For even m, P = 50000 is the upper
 *            median, as in `median` and `localmad`;
 *   m == 0:  every value_j is NaN.
 * Duplicate P_j are allowed and answered in the order given.  Intervals may overlap, repeat and come in any order.
 * Every figure is a function of the interval's sample alone, chosen by integer comparisons: nothing depends on the
 * route an interval takes, the grid, the dispatch order, the order of the intervals or how they are batched.
 *
 * The conventions are gdsp_interval_stats[_batch]'s: HOST arrays in (GDSP_EINVAL for start >= end or end > n, for np
 * outside 1..16 and for a P above 100000; count == 0 is a no-op), HOST arrays out in the caller's order -- h_count[i],
 * and h_values[i*np + j] for P_j --, vectors 8-byte aligned, the signal read on the current device and never written,
 * and the call waits for the device.  Intervals of at most gdsp_interval_percentiles_short() bases are sorted in LDS
 * after one read of the signal; longer ones are cut into pieces of gdsp_interval_percentiles_piece() bases and take a
 * radix select over HBM for all their (interval, percentile) queries at once, a query ending as soon as every key it
 * still considers is one value (gdsp_intervalpct.hip).  The histograms of that select are bounded workspace: a call
 * with more long queries than fit runs them in batches of whole intervals, and gdsp_interval_percentiles_set_batch
 * sets that number of queries (0: the default) so that a test can force many small batches. */
#define GDSP_INTERVAL_PERCENTILES_MAX 16
/* Host: the longest interval the one-read route takes, and the piece of the other; results never depend on them */
uint32_t gdsp_interval_percentiles_short (void);
uint32_t gdsp_interval_percentiles_piece (void);
int gdsp_interval_percentiles       (const double* d_v, uint32_t n, const uint32_t* h_start, const uint32_t* h_end, uint32_t count,
                                     const uint32_t* pThousandths, int np, double lo, double hi,
                                     uint32_t* h_count, double* h_values, void* stream);
int gdsp_interval_percentiles_batch (const gdsp_batch_item* items, int nitems, const uint32_t* h_vec, const uint32_t* h_start,
                                     const uint32_t* h_end, uint32_t count, const uint32_t* pThousandths, int np,
                                     double lo, double hi, uint32_t* h_count, double* h_values, void* stream);
int  gdsp_interval_percentiles_set_batch (uint32_t longQueries);
/* what the last gdsp_interval_percentiles[_batch] did: [0] intervals, [1] those of the short route, [2] of the long
 * route, [3] histogram passes (per batch, those of the query that took most), [4] batches, [5] long queries that ended
 * before the last digit */
void gdsp_interval_percentiles_last (uint64_t out[6]);

/* ---- breadthover (not in the reference): bases at or above each depth threshold, per interval -----------------------
 * The inverse of percentilesover's question: rank from value.  For a vector v of n doubles, an interval [s, e) with
 * 0 <= s < e <= n, limits lo, hi, thresholds T_0 .. T_{q-1} (1 <= q <= GDSP_INTERVAL_THRESHOLDS_MAX) and a flag `strict`:
 *   the sample is statsover's: the bases i in [s, e) with !(v[i] < lo) && !(v[i] > hi) and v[i] finite;
 *   count      m, the number of sampled bases;
 *   atleast_j  the number of sampled bases with v[i] >= T_j as IEEE compares them, or with v[i] > T_j when strict != 0;
 *              -0.0 and +0.0 are equal.
 * A threshold is any double that is not NaN, infinities included (T = -inf counts the whole sample, T = +inf nothing).
 * Duplicate T_j are allowed, in any order, and answered in the order given.  Intervals may overlap, repeat and come in
 * any order.  Every figure is an integer and a function of the interval's sample alone: nothing depends on tiles, grid,
 * the split into launches, dispatch order, the order of the intervals or how they overlap, or devices.
 *
 * The conventions are gdsp_interval_percentiles[_batch]'s: HOST arrays in (GDSP_EINVAL, before the device is touched, for
 * nt outside 1..16, a NaN threshold, start >= end, end > n, a vector index beyond the table, a misaligned vector and NULL
 * arrays; count == 0 is a no-op), HOST arrays out in the caller's order -- h_count[i], and h_atleast[i*nt + j] for T_j --,
 * vectors 8-byte aligned, the signal read on the current device and never written, and the call waits for the device.
 * The device reduces statsover's pieces -- an interval cut at multiples of gdsp_interval_breadth_tile() values of the
 * 16-byte aligned frame its vector lies in -- to integer records and the host adds an interval's records in 64 bits
 * (gdsp_intervalbreadth.hip).  gdsp_interval_breadth_set_launch_pieces sets the most pieces of one launch (0: the
 * default) so that a test can force several launches. */
#define GDSP_INTERVAL_THRESHOLDS_MAX 16
uint32_t gdsp_interval_breadth_tile (void);
int gdsp_interval_breadth       (const double* d_v, uint32_t n, const uint32_t* h_start, const uint32_t* h_end, uint32_t count,
                                 const double* thresholds, int nt, int strict, double lo, double hi,
                                 uint32_t* h_count, uint32_t* h_atleast, void* stream);
int gdsp_interval_breadth_batch (const gdsp_batch_item* items, int nitems, const uint32_t* h_vec, const uint32_t* h_start,
                                 const uint32_t* h_end, uint32_t count, const double* thresholds, int nt, int strict,
                                 double lo, double hi, uint32_t* h_count, uint32_t* h_atleast, void* stream);
int  gdsp_interval_breadth_set_launch_pieces (uint32_t pieces);
/* what the last gdsp_interval_breadth[_batch] did: [0] intervals, [1] pieces, [2] launches, [3] workgroups; and where its
 * time went, in ms: [0] cutting the intervals into pieces (host), [1] the kernel (HIP events), [2] copies and waiting,
 * [3] combining the pieces (host) */
void gdsp_interval_breadth_last  (uint64_t out[4]);
void gdsp_interval_breadth_times (double ms[4]);

/* ---- correlateover (not in the reference): correlate's figures of the signal against a second track, per interval ----
 * For a vector x of n doubles, a second track y of the same length, an interval [s, e) with 0 <= s < e <= n and limits
 * lo, hi, ylo, yhi, the interval's pair sample is correlate's, without a window: the bases i in [s, e) with
 *   !(x[i] < lo) && !(x[i] > hi), x[i] finite, !(y[i] < ylo) && !(y[i] > yhi), y[i] finite.
 * The interval's record is what gdsp_genome_correlation gives for that sample (the definitions are there and are not
 * reworded): count; mean and filemean, the exact sums of x and of y over the count, each rounded once; then with
 * dx = fl(x - mean), dy = fl(y - filemean) the products fl(dx dx), fl(dy dy), fl(dx dy), each summed exactly and divided
 * once by the count -- a product that is not finite makes its variance +inf, the covariance NaN --; stddev and filestddev
 * the square roots of the two variances; covariance; correlation, slope and intercept derived operation by operation as
 * correlate derives them.  An empty sample has count 0 and NaN in every other figure; a figure that is not defined is
 * NaN.  An interval [0, n) has, bit for bit, gdsp_genome_correlation's figures of the one pair (x, y) with window 1.
 * Intervals may overlap, repeat and come in any order.  Every figure is a function of the interval's sample alone: nothing
 * depends on tiles, grid, the split into launches, dispatch order, the order of the intervals or how they overlap, or
 * devices.
 *
 * The conventions are gdsp_interval_breadth[_batch]'s: HOST arrays in, h_out[i] for interval i in the caller's order, the
 * vectors read on the current device and never written, the call waits for the device.  items[k].d_in is the signal and
 * items[k].d_out the second track of the same length, READ ONLY here (gdsp_localcorr_batch's way of naming two vectors).
 * Both are 8-byte aligned and the track's 16-byte alignment may differ from the signal's.  GDSP_EINVAL before the device
 * is touched for what gdsp_interval_breadth_batch refuses and for a track that is NULL or not 8-byte aligned; count == 0
 * is a no-op.  The device reduces statsover's pieces in two passes, sums and then products around the interval's means,
 * to two-term expansions that the host combines exactly; a piece whose expansion did not hold its sum is summed again
 * through correlate's exact pass (gdsp_intervalcorr.hip).  gdsp_interval_correlation_set_launch_pieces sets the most
 * pieces of one launch (0: the default) so that a test can force several launches. */
typedef struct gdsp_interval_corr
	{ uint32_t count, reserved;  double mean, filemean, stddev, filestddev, covariance, correlation, slope, intercept; } gdsp_interval_corr;
uint32_t gdsp_interval_correlation_tile (void);
int gdsp_interval_correlation       (const double* d_x, const double* d_y, uint32_t n, const uint32_t* h_start, const uint32_t* h_end,
                                     uint32_t count, double lo, double hi, double ylo, double yhi, gdsp_interval_corr* h_out, void* stream);
int gdsp_interval_correlation_batch (const gdsp_batch_item* items, int nitems, const uint32_t* h_vec, const uint32_t* h_start,
                                     const uint32_t* h_end, uint32_t count, double lo, double hi, double ylo, double yhi,
                                     gdsp_interval_corr* h_out, void* stream);
int  gdsp_interval_correlation_set_launch_pieces (uint32_t pieces);
/* what the last gdsp_interval_correlation[_batch] did: [0] intervals, [1] pieces, [2] pieces summed again after pass 1,
 * [3] after pass 2; and where its time went, in ms: [0] cutting the intervals into pieces (host), [1] the kernels of both
 * passes (HIP events), [2] copies, waiting and the second sums, [3] the means and combining the pieces (host) */
void gdsp_interval_correlation_last  (uint64_t out[4]);
void gdsp_interval_correlation_times (double ms[4]);

/* ---- segments (not in the reference): the signal's own thresholded regions, each with statsover's figures, exact ------
 * For a vector v of n doubles, a threshold T and tiesAbove:
 *   member   base i is a member iff v[i] > T, or v[i] >= T with ties above: binarize's test.  A NaN is never a member
 *            and splits a run; +inf (and -inf against T = -inf with ties above) is a member when the test says so.
 *   run      a maximal stretch [s, e) of consecutive members.
 *   segment  the runs of one vector, in position order, joined while next.s - prev.e <= mergeGap (0: nothing is joined);
 *            it spans [first.s, last.e).  Its sample is statsover's sample restricted to its member bases: the finite
 *            members.  The bases of the gaps are not sampled.
 *   filters  applied after joining: a segment is dropped when end - start < minLength (1: none is), and, when a minimum
 *            height is given, when its sample is empty or its max < minHeight.
 *   figures  of a kept segment: count, sum and mean (exact, rounded once), min, max, maxpos (the lowest position of the
 *            maximum) exactly as statsover defines them: a zero result is +0.0, and an empty sample (a segment of +inf
 *            only) has sum +0.0, NaN for mean, min and max, and maxpos UINT32_MAX.
 * The set of segments and every figure are functions of the signal and the five parameters alone: nothing depends on
 * tiles, grid, dispatch order, how many records a launch may hold, devices or the order of the vectors.
 *
 * Device half, gdsp_run_pieces_batch: every vector of the table (d_in and n of an item are read; 8-byte aligned; on the
 * current device) is cut at multiples of gdsp_segments_tile() values of the 16-byte aligned frame it lies in, and every
 * maximal stretch of members inside a tile becomes one record: where it lies, and a gdsp_interval_piece for its sample
 * (a0 + a1 is the exact sum unless `flag`).  Pieces of neighbouring tiles that touch are one run.  The records reach
 * `emit` as HOST arrays in (vector, position) order, at most a bounded number per call -- 2^21, or what the environment
 * variable GDSP_SEGMENTS_RECORDS says when that is less, down to the gdsp_segments_tile() / 2 a single tile can give --
 * together with one GDSP_XSUM_WORDS image per flagged piece, in order (NULL when none is flagged).  The arrays are the
 * library's and valid during the call; a nonzero return from `emit` ends the pass with GDSP_EINVAL.  The signal is only
 * read.  Waits for the device.
 *
 * Host half, no GPU: a builder takes such records in (vector, position) order in any number of feeds, joins touching
 * pieces and runs within mergeGap, carries the open segment from one feed to the next, applies the filters, and hands
 * the kept segments to its callback in order (gdsp_interval_stats_combine gives the figures).  gdsp_segments_finish
 * closes the open segment; the builder can then be fed again or destroyed.  Its memory does not grow with the length of
 * a segment. */
typedef struct gdsp_run_piece { uint32_t vec, start, end, reserved;  gdsp_interval_piece piece; } gdsp_run_piece;   /* [start, end) of items[vec] */
typedef struct gdsp_segment   { uint32_t vec, start, end, reserved;  gdsp_interval_stat  stat;  } gdsp_segment;
typedef int (*gdsp_run_pieces_fn) (void* ctx, const gdsp_run_piece* pieces, uint32_t count, const uint64_t* images);
typedef int (*gdsp_segments_fn)   (void* ctx, const gdsp_segment* segments, uint32_t count);
typedef struct gdsp_segments_builder gdsp_segments_builder;
uint32_t gdsp_segments_tile (void);
int gdsp_run_pieces_batch (const gdsp_batch_item* items, int nitems, double T, int tiesAbove, gdsp_run_pieces_fn emit, void* ctx,
                           void* stream);
int gdsp_segments_create  (gdsp_segments_builder** builder, uint32_t mergeGap, uint32_t minLength, int haveMinHeight,
                           double minHeight, gdsp_segments_fn emit, void* ctx);
int gdsp_segments_feed    (gdsp_segments_builder* builder, const gdsp_run_piece* pieces, uint32_t count, const uint64_t* images);
int gdsp_segments_finish  (gdsp_segments_builder* builder);
/* what the builder has seen so far: [0] runs, [1] pieces, [2] flagged pieces, [3] kept segments */
void gdsp_segments_counts (const gdsp_segments_builder* builder, uint64_t out[4]);
void gdsp_segments_destroy (gdsp_segments_builder* builder);
/* end to end on the current device: the device half feeding a builder; waits for the pass */
int gdsp_segments_batch (const gdsp_batch_item* items, int nitems, double T, int tiesAbove, uint32_t mergeGap, uint32_t minLength,
                         int haveMinHeight, double minHeight, gdsp_segments_fn emit, void* ctx, void* stream);
/* what the last gdsp_segments_batch did: [0] runs, [1] pieces, [2] flagged pieces (summed again), [3] kept segments; and
 * where the last gdsp_run_pieces_batch spent its time, in ms: [0] the counting pass, [1] the piece kernel (HIP events),
 * [2] copies, waiting and flagged pieces, [3] inside `emit` */
void gdsp_segments_last  (uint64_t out[4]);
void gdsp_segments_times (double ms[4]);

/* ---- keepsegments (not in the reference): the kept segments of `segments` written back into the signal ---------------
 * For vectors v (d_in) and outputs w (d_out, another buffer: an output never overlaps its input), the selection
 * parameters of `segments`, a mode and two values `one` and `zero`:
 *   every base of w outside every kept segment becomes `zero`;
 *   a kept segment is its whole span [start, end), the gap bases that mergeGap joined included (as after a `close`), and
 *   every base of it becomes, by mode:
 *     GDSP_KEEP_ONE     `one`;
 *     GDSP_KEEP_VALUE   v's own base, bit for bit (a gap base keeps whatever it holds, a NaN and its payload included);
 *     GDSP_KEEP_COUNT, _LENGTH, _SUM, _MEAN, _MIN, _MAX   that figure of the segment: the very double of its
 *                       gdsp_interval_stat (count and end - start converted, both exact), so a segment with an empty
 *                       sample writes NaN for mean, min and max and +0.0 for sum.
 * `one` and `zero` are stored as given (a -0.0 stays -0.0).  Every base of every w is written exactly once; v is only
 * read.  The result is a function of the signal and the parameters alone, as the segments are.
 *
 * Device half, gdsp_paint_spans_batch: `spans` is a HOST array of disjoint spans in (vector, position) order (start < end
 * <= n of items[vec], a span may begin where the one before ends; anything else is GDSP_EINVAL).  Every base (vector,
 * position) with (fromVec, fromPos) <= it < (toVec, toPos) -- (nitems, 0) is the end of the last vector -- is written
 * once: a base inside a span gets the span's value, or with `copy` d_in's own base; any other base gets `outside`.  Spans
 * or parts of spans outside that range are passed over, so a cursor or a limit may lie inside a span, and two calls that
 * split the range anywhere write what one call writes.  Figure painting (copy == 0) reads nothing of d_in (it may be
 * NULL).  Vectors are 8-byte aligned; the outputs are cut at multiples of gdsp_paint_tile() values of the 16-byte aligned
 * frame each lies in; all vectors of the current device go into one launch per 32 of them, and at most 2^21 spans are
 * staged at a time.  Waits for the device.
 *
 * End to end, gdsp_keep_segments_batch: gdsp_segments_batch's pass over d_in; each time kept segments arrive (a bounded
 * number at a time, see GDSP_SEGMENTS_RECORDS) their spans are painted into d_out from where the last paint ended to the
 * end of the last segment received, and the rest is painted after the pass: neither host nor device memory grows with
 * the number of segments.  `emit` (may be NULL) then receives the same segments gdsp_segments_batch would hand it.  Waits. */
enum { GDSP_KEEP_ONE = 0, GDSP_KEEP_VALUE = 1, GDSP_KEEP_COUNT = 2, GDSP_KEEP_LENGTH = 3, GDSP_KEEP_SUM = 4, GDSP_KEEP_MEAN = 5,
       GDSP_KEEP_MIN = 6, GDSP_KEEP_MAX = 7 };
typedef struct gdsp_paint_span { uint32_t vec, start, end, reserved;  double value; } gdsp_paint_span;   /* [start, end) of items[vec] */
uint32_t gdsp_paint_tile (void);
int gdsp_paint_spans_batch (const gdsp_batch_item* items, int nitems, const gdsp_paint_span* spans, uint32_t nspans, int copy,
                            double outside, uint32_t fromVec, uint32_t fromPos, uint32_t toVec, uint32_t toPos, void* stream);
/* what the last gdsp_paint_spans_batch did (either may be NULL): bases painted [0] inside spans, [1] outside; ms spent
 * [0] in the paint launches (HIP events), [1] around them (the tiles' index, copies, waiting) */
void gdsp_paint_spans_last (uint64_t painted[2], double ms[2]);
int gdsp_keep_segments_batch (const gdsp_batch_item* items, int nitems, double T, int tiesAbove, uint32_t mergeGap, uint32_t minLength,
                              int haveMinHeight, double minHeight, int mode, double one, double zero, gdsp_segments_fn emit, void* ctx,
                              void* stream);
/* what the last gdsp_keep_segments_batch did: [0] .. [3] as gdsp_segments_last, [4] bases painted inside kept segments,
 * [5] bases painted outside; and the time of its paints as gdsp_paint_spans_last gives it, summed.  (gdsp_segments_last
 * and gdsp_segments_times describe its pass.) */
void gdsp_keep_segments_last  (uint64_t out[6]);
void gdsp_keep_segments_times (double ms[2]);

/* ---- histogram (not in the reference): the genome-wide distribution of the values, exact, in one pass ---------------
 * The sample is stats': every window-th value counted from each chromosome's first base (a source carries `first`) whose
 * value v satisfies !(v < lo) && !(v > hi), finite values only (never NaN, never +-inf); n is its size.
 * The bins are an edge table e[0] < e[1] < ... < e[B] of finite doubles, 1 <= B <= 65536: a sampled v belongs to bin k
 * iff e[k] <= v < e[k+1] as IEEE compares them (-0.0 falls where +0.0 falls), is `below` when v < e[0] and `above` when
 * v >= e[B].  Uniform bins are the table e[k] = fma (k, width, lo), each edge rounded once: gdsp_histogram_uniform_edges,
 * host code that needs no GPU, fills h_edges[0 .. nbins] and refuses (GDSP_EINVAL) a lo / width / nbins whose table is not
 * strictly increasing and finite.
 * The result is nbins + 3 u64 words: counts[0 .. B) the bins, counts[B] below, counts[B+1] above, counts[B+2] = n, the sum
 * of all the others.  It is a function of the sample and the table alone: it does not depend on tiles, grid, dispatch
 * order, the cut of the genome, devices or ranks, and the words of two samples add to the words of their union
 * (all-reduce them with op 0).
 * `uniform` != 0 is a hint that the table is (close to) evenly spaced: the bin is guessed by one multiplication and then
 * corrected by comparing against the table, which alone decides; any table gives the same words with and without it.
 * The signal is only read.  Sources as for the xsum calls (8-byte aligned, on the current device for the _batch call). */
int gdsp_histogram_uniform_edges (double lo, double width, uint32_t nbins, double* h_edges);
int gdsp_histogram_init (uint64_t* d_counts, uint32_t nbins, void* stream);          /* zero nbins + 3 words */
/* add the sample of every source to d_counts (one launch per 32 sources; h_edges is a HOST table of nbins + 1 values) */
int gdsp_histogram_accumulate_batch (const gdsp_xsum_source* sources, int nsources, uint32_t window, double lo, double hi,
                                     const double* h_edges, uint32_t nbins, int uniform, uint64_t* d_counts, void* stream);
/* end to end, like gdsp_genome_stats: sources may sit on several devices of this process (each device's work is queued on
 * the stream of its first source; the words are added on the host, or all-reduced in HBM through the communicator given
 * to gdsp_genome_histogram_use_comm); with one process per GPU pass `reduce` (op 0).  h_counts: nbins + 3 HOST words; no
 * sources, or an empty sample: all zeros.  Waits for the pass. */
int gdsp_genome_histogram (const gdsp_xsum_source* sources, int nsources, uint32_t window, double lo, double hi,
                           const double* h_edges, uint32_t nbins, int uniform,
                           gdsp_reduce_fn reduce, void* reduceCtx, uint64_t* h_counts);
int gdsp_genome_histogram_use_comm (gdsp_comm* comm);  /* NULL switches back to host sums */

/* multiplyconst / divideconst / normalize (in place, one pointwise launch per table of 32 vectors): v = fl(v * c),
 * fl(v / c) (c == 0 is refused), fl(fl(v - center) / scale) (scale == 0 is refused) */
int gdsp_multiply_constant       (double* d_v, uint32_t n, double c, void* stream);
int gdsp_divide_constant         (double* d_v, uint32_t n, double c, void* stream);
int gdsp_standardize             (double* d_v, uint32_t n, double center, double scale, void* stream);
int gdsp_multiply_constant_batch (const gdsp_batch_item* items, int nitems, double c, void* stream);
int gdsp_divide_constant_batch   (const gdsp_batch_item* items, int nitems, double c, void* stream);
int gdsp_standardize_batch       (const gdsp_batch_item* items, int nitems, double center, double scale, void* stream);

/* ---- genodsp.c read_intervals / add.c / multiply.c ------------------------------ */

/* Interval-driven writes.  The host routes intervals to this chromosome, applies
 * origin and clipping rules, and bins their indices (file order kept) into tiles of
 * gdsp_interval_tile() bases with gdsp_bin_intervals; the device then applies, to
 * every base, the intervals covering it IN FILE ORDER -- bit-identical to the
 * reference's `for ix in [start,end)` loops for any values.
 *   gdsp_apply_intervals: read_intervals genodsp.c:1305-1331 (sum/min/max, and the
 *     first-touch rule when `clear`), op_add/op_subtract add.c:282-283, :575-576
 *     (pass negated values for subtract).
 *   gdsp_scale_intervals: op_multiply multiply.c:326-345, op_divide :706-740; bases
 *     under no interval become 0 (multiply) or +-infinityVal (divide). */
#define GDSP_CLEAR_FIRST_TOUCH 1   /* a base still equal to missingVal is assigned (genodsp.c:1311) */
#define GDSP_CLEAR_FILL        2   /* every base starts from missingVal (genodsp.c:1225-1240)       */
#define GDSP_CLEAR_BOTH        3   /* what read_intervals(clear=true) does                          */
#define GDSP_MASK_BINARIZE_FIRST 4 /* internal flag of gdsp_mask_intervals                            */
uint32_t gdsp_interval_tile (void);
int gdsp_bin_intervals   (uint32_t n, const uint32_t* h_start, const uint32_t* h_end, uint32_t count,
                          uint32_t* h_tileOffsets, uint32_t* h_tileList, uint64_t* listLen);
int gdsp_apply_intervals (double* d_v, uint32_t n, const uint32_t* d_start, const uint32_t* d_end,
                          const double* d_val, const uint32_t* d_tileOffsets, const uint32_t* d_tileList,
                          int overlapOp, int clear, double missingVal, void* stream);
int gdsp_scale_intervals (double* d_v, uint32_t n, const uint32_t* d_start, const uint32_t* d_end,
                          const double* d_val, const uint32_t* d_tileOffsets, const uint32_t* d_tileList,
                          int divide, double infinityVal, void* stream);

/* mask / masknot (mask.c:187-300, :483-640) and or / and (logical.c:439-560, :737-880):
 *   inside=1: bases under an interval become d_val[i]; inside=0: bases under NO interval become
 *   outsideVal (intervals sorted and non-overlapping, as for multiply);
 *   binarizeFirst: every nonzero base becomes 1.0 first (or, and).
 * minwith / maxwith (minmax.c:1893-2010, :2179-2294) are gdsp_apply_intervals with
 * GDSP_OVERLAP_MIN / GDSP_OVERLAP_MAX and clear=0. */
int gdsp_mask_intervals (double* d_v, uint32_t n, const uint32_t* d_start, const uint32_t* d_end,
                         const double* d_val, const uint32_t* d_tileOffsets, const uint32_t* d_tileList,
                         int inside, double outsideVal, int binarizeFirst, void* stream);

/* minover / maxover (minmax.c:193-390, :596-793): inside each sorted, non-overlapping interval only
 * the extreme survives, at the tied position nearest the interval's centre; everything else becomes
 * `fill`.  d_work >= gdsp_extreme_in_intervals_work(count) bytes. */
size_t gdsp_extreme_in_intervals_work (uint32_t count);
int gdsp_extreme_in_intervals (double* d_v, uint32_t n, const uint32_t* d_start, const uint32_t* d_end, uint32_t count,
                               const uint32_t* d_tileOffsets, const uint32_t* d_tileList,
                               int wantMax, double fill, void* d_work, void* stream);

/* ---- genodsp.c report_intervals:1561-1691 --------------------------------------- */

/* Run-length encode one chromosome on the device.  d_runs receives up to cap
 * (start,end) u32 pairs and d_vals the run values; *d_count the number of runs
 * found (may exceed cap: call again with more room).  uncovered: 0 hide, 1 show, -1 NA. */
size_t gdsp_report_runs_work (uint32_t n);
int gdsp_report_runs (const double* d_v, uint32_t n, int collapse, int uncovered,
                      uint32_t* d_runStart, uint32_t* d_runEnd, double* d_runVal, uint32_t cap,
                      uint32_t* d_count, void* d_work, void* stream);

/* ---- synthetic coverage signal for benchmarks and parity tests (not in the reference) */
int gdsp_synth_coverage (double* d_out, uint64_t seed, uint32_t chromIndex, uint32_t start,
                         uint32_t count, int mode, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GENODSP_HIP_H */
