// gdsp_localmad.hip -- localmad / hampel: each base against the median and the median absolute deviation (MAD) of the
// window centred on it.
//
// Not an operator of the reference.  Definition (include/genodsp_hip.h): slidingpercentile's window, centring and rank;
// med the window's median as gdsp_sliding_percentile writes it, d_j = |fl(v_j - med)| over the window, mad the k-th
// smallest d_j with the median's own k, and from these sigma = fl(scale max(mad, minmad)), diff, limit and the six
// figures, every step one rounded IEEE operation.  Comparisons and single roundings only: bit exact.
//
// One workgroup owns T outputs and builds rankfilt's tile over the NS = 2^LOG_N inputs they read (gdsp_rank_tile.h):
// ONE sort and ONE wavelet matrix per tile, whatever is asked of it afterwards.  Per output:
//   1. the median: one range-quantile query, rank k of the window;
//   2. the MAD without forming a single deviation of the window.  With s_0 <= ... <= s_{m-1} the sorted window and
//      med = s_k, fl(x - med) is monotone in x, so the k+1 smallest deviations are those of one contiguous block
//      s_a .. s_{a+k} and mad = min over a of max(L(a), R(a)), L(a) = |fl(med - s_a)| falling and
//      R(a) = |fl(s_{a+k} - med)| rising with a.  A binary search over a = 0 .. k for the first a with L(a) <= R(a):
//      ceil(log2(k+1)) probes, each two range-quantile queries (ranks a and a+k of the same window) and two values.
//      The answer is min(R(a*), L(a*-1)); both were formed by the probes that last moved the two ends of the search,
//      so they are kept and not asked for again -- except R(k) where no probe held and m is odd, one more query (for
//      even m rank 2k lies outside the window and L(k-1) alone is the answer).  A probe with L(a) == R(a) ends the
//      search at once: every block to its left has L no smaller, every block to its right R no smaller (exact; on read
//      depth, where deviations are small integers, most searches end this way);
//   3. the figure, from med, mad and v_i.
// So a base costs at most 1 + 2 ceil(log2(k+1)) + 1 queries where slidingpercentile asks one: 8 at W = 11, 14 at
// W = 101, 20 at W = 1001, 24 at W = 4095.
//
// Where the probes get their values.  The sort destroys the staged keys (they share a union with the levels), and a
// probe needs s_a and s_{a+k} themselves.  They are read from the input again, through the sorted local index, as
// rankfilt's last line reads its result: the tile's 64 KiB were loaded by this workgroup a moment ago and sit in L2.
// The other way -- a sorted copy of the values in LDS -- takes 64 KiB more at NS = 8192: 144 KiB, one workgroup per CU
// in place of two, and with it the overlap of one tile's sort barriers with the other tile's queries, which is what
// keeps the CU busy during the build; the queries themselves are chains of dependent LDS reads (two per level), which
// a second workgroup's waves hide as well.  A probe's two loads are independent of each other and issued together, so
// a probe pays one L2 latency on top of its 2 x LOG_N LDS round trips.
//
// Measured (profiles/localmad.txt, one MI355X, 3.1 Gbp in one call, W = 101 / 1001 / 4095): 2.1-3.0 x slidingpercentile's
// time on read depth, 2.7-3.3 x on a smoothed signal, 1.2-1.3 x on an all-zero genome -- about a seventh of the query
// count, because most of slidingpercentile's time is the tile, which is built once either way.  A full search adds
// 25-43 ms per probe over the genome: 4 x LOG_N gathered 16-byte LDS reads per lane, which at the LDS's rate for such reads
// accounts for the time; the two value reads do not (reckoned from the rates, not profiled).
//
// No scratch (profiles/localmad_resources.txt), no workgroup waits on another, and every loop is bounded by the window
// whatever the values are: a NaN or an infinity spoils the figures of the windows that hold it and nothing else.

#include "gdsp_rank_tile.h"

static_assert (GDSP_LOCALMAD_MAX_WINDOW == GDSP_SLIDING_PERCENTILE_MAX_WINDOW, "the tile rule is slidingpercentile's");
static_assert (2 * (GDSP_LOCALMAD_MAX_WINDOW - 1) < (1 << RF_MAX_LOG), "the largest window must leave half a tile of outputs");

struct LmParams { double scale, threshold, minMad;  int what, haveMinMad; };

// the figure of one base: v its value (bit for bit), med its window's median (-0.0 folded), mad its window's MAD
__device__ __forceinline__ double lm_figure (double v, double med, double mad, const LmParams& P)
	{
	const double madf    = (P.haveMinMad && (P.minMad > mad))? P.minMad : mad;
	const double sigma   = P.scale * madf;
	const double diff    = (v == med)? 0.0 : v - med;
	const double limit   = P.threshold * sigma;
	const bool   outlier = fabs (diff) > limit;
	switch (P.what)
		{
		case GDSP_LOCALMAD_MEDIAN:     return med;
		case GDSP_LOCALMAD_MAD:        return madf;
		case GDSP_LOCALMAD_DIFFERENCE: return diff;
		case GDSP_LOCALMAD_CLEAN:      return outlier? med : v;
		case GDSP_LOCALMAD_OUTLIER:    return outlier? 1.0 : 0.0;
		default:                       return (sigma == 0.0)? 0.0 : diff / sigma;      // GDSP_LOCALMAD_ZSCORE
		}
	}

template <int LOG_N>
__device__ __forceinline__
void localmad_tile (const double* __restrict__ in, double* __restrict__ out, uint32_t n, uint32_t tile,
                    uint32_t wL, uint32_t wR, const LmParams& P)
	{
	constexpr int NS      = 1 << LOG_N;
	constexpr int THREADS = NS / 8;                                         // eight positions per thread
	__shared__ RfLds<LOG_N> S;
	const int      tid   = threadIdx.x;
	const int64_t  T     = NS - (int64_t) (wL + wR);                       // outputs per tile
	const int64_t  o0    = (int64_t) tile * T;                              // first output of the tile
	const int64_t  s0    = (o0 > (int64_t) wL)? o0 - wL : 0;                // first staged base
	const int64_t  send  = (o0 + T + wR < (int64_t) n)? o0 + T + wR : (int64_t) n;
	const int      nloc  = (int) (send - s0);                               // staged bases (<= NS)
	const double* __restrict__ staged = in + s0;

	rf_tile_build<LOG_N> (S, in, s0, nloc);                                 // stage, sort, matrix: once per tile

	for (int64_t o=tid ; o<T ; o+=THREADS)
		{
		const int64_t i = o0 + o;
		if (i >= (int64_t) n) break;
		const int64_t first = (i > (int64_t) wL)? i - wL : 0;
		const int64_t last  = (i + wR < (int64_t) n)? i + wR : (int64_t) n - 1;
		const uint32_t lo = (uint32_t) (first - s0), hi = (uint32_t) (last + 1 - s0);
		const uint32_t m  = hi - lo;
		const uint32_t k  = gdsp_rank_of (m, 50000);
		const double   v  = in[i];
		const double   med = gdsp_value_of (gdsp_key_of (staged[S.idx[rf_tile_query<LOG_N> (S, lo, hi, k)]]));

		// the first a of 0 .. k with L(a) <= R(a); every rank asked for is below m: a <= k-1 in a probe, and k-1+k <= m-1
		const double inf = __builtin_inf ();
		double   bestR = inf, bestL = inf;                                  // R(a_hi) once a probe held, L(a_lo - 1) once one did not
		uint32_t alo = 0, ahi = k;
		bool     heldOnce = false;
		while (alo < ahi)
			{
			const uint32_t a  = (alo + ahi) >> 1;
			const uint32_t ra = rf_tile_query<LOG_N> (S, lo, hi, a), rb = rf_tile_query<LOG_N> (S, lo, hi, a + k);
			const double   sa = staged[S.idx[ra]], sb = staged[S.idx[rb]];   // (both loads in flight together)
			const double   L  = fabs (med - sa), R = fabs (sb - med);
			if (L == R) { bestR = R;  heldOnce = true;  break; }            // no block has a smaller larger end
			if (L < R) { ahi = a;      bestR = R;  heldOnce = true; }
			else       { alo = a + 1;  bestL = L; }
			}
		if (!heldOnce && (2*k < m))                                         // a* = k with m odd: the block s_k .. s_2k, L(k) = 0
			bestR = fabs (staged[S.idx[rf_tile_query<LOG_N> (S, lo, hi, 2*k)]] - med);
		const double mad = (bestL < bestR)? bestL : bestR;

		out[i] = lm_figure (v, med, mad, P);
		}
	}

template <int LOG_N>
__global__ __launch_bounds__((1 << LOG_N) / 8) __attribute__((amdgpu_waves_per_eu ((LOG_N == 13)? 8 : 1)))   // (13: <= 64 VGPRs, two tiles per CU)
void localmad_kernel (const double* __restrict__ in, double* __restrict__ out, uint32_t n, uint32_t ntiles,
                      uint32_t wL, uint32_t wR, LmParams P)
	{ localmad_tile<LOG_N> (in, out, n, gdsp_xcd_tile (blockIdx.x, ntiles), wL, wR, P); }

template <int LOG_N>                                                        // one grid over every vector of the table (gdsp_common.h)
__global__ __launch_bounds__((1 << LOG_N) / 8) __attribute__((amdgpu_waves_per_eu ((LOG_N == 13)? 8 : 1)))
void localmad_batch_kernel (GdspBatch B, uint32_t wL, uint32_t wR, LmParams P)
	{
	const double* in;  double* out;  uint32_t n;
	const uint32_t tile = gdsp_batch_tile (B, in, out, n);
	localmad_tile<LOG_N> (in, out, n, tile, wL, wR, P);
	}

template <int LOG_N>
static void localmad_launch (const gdsp_batch_item* items, int nitems, uint32_t wL, uint32_t wR, const LmParams& P, hipStream_t s)
	{
	const uint64_t T = (1u << LOG_N) - (uint64_t) (wL + wR);
	if (nitems == 1)
		{
		if (items[0].n == 0) return;
		const uint32_t ntiles = (uint32_t) (((uint64_t) items[0].n + T - 1) / T);
		hipLaunchKernelGGL ((localmad_kernel<LOG_N>), dim3(ntiles), dim3((1 << LOG_N) / 8), 0, s,
		                    items[0].d_in, items[0].d_out, items[0].n, ntiles, wL, wR, P);
		return;
		}
	gdsp_batch_run (items, nitems, [=] (uint32_t n) { return ((uint64_t) n + T - 1) / T; },
		[&] (const GdspBatch& B, uint32_t tiles)
			{
			hipLaunchKernelGGL ((localmad_batch_kernel<LOG_N>), dim3(tiles), dim3((1 << LOG_N) / 8), 0, s, B, wL, wR, P);
			});
	}

static int localmad_run (const gdsp_batch_item* items, int nitems, uint32_t W, const LmParams& P, void* stream)
	{
	const uint32_t wL = (W - 1) / 2, wR = (W - 1) - wL;
	hipStream_t s = gdsp_stream (stream);
	switch (rf_tile_log (W))
		{
		case 10: localmad_launch<10> (items, nitems, wL, wR, P, s);  break;
		case 11: localmad_launch<11> (items, nitems, wL, wR, P, s);  break;
		case 12: localmad_launch<12> (items, nitems, wL, wR, P, s);  break;
		default: localmad_launch<13> (items, nitems, wL, wR, P, s);  break;
		}
	GDSP_LAUNCH_CHECK ();
	return GDSP_OK;
	}

// the checks the two calls share (-> GDSP_OK with P filled in)
static int localmad_params (LmParams& P, uint32_t W, int what, double scale, double threshold, int haveMinMad, double minMad)
	{
	GDSP_REQUIRE (W >= 1, "window must be >= 1");
	GDSP_REQUIRE (W <= GDSP_LOCALMAD_MAX_WINDOW, "window above GDSP_LOCALMAD_MAX_WINDOW");
	GDSP_REQUIRE ((what >= GDSP_LOCALMAD_ZSCORE) && (what <= GDSP_LOCALMAD_OUTLIER), "unknown figure (what)");
	GDSP_REQUIRE ((scale > 0.0) && (scale < __builtin_huge_val ()), "scale must be finite and positive");
	GDSP_REQUIRE (threshold >= 0.0, "threshold must be a number that is not negative");
	GDSP_REQUIRE (!haveMinMad || (minMad >= 0.0), "minMad must be a number that is not negative");
	P.scale = scale;  P.threshold = threshold;  P.minMad = haveMinMad? minMad : 0.0;
	P.what = what;  P.haveMinMad = haveMinMad? 1 : 0;
	return GDSP_OK;
	}

extern "C" {

uint32_t gdsp_localmad_tile (uint32_t W)
	{
	if ((W < 1) || (W > GDSP_LOCALMAD_MAX_WINDOW)) return 0;
	return (1u << rf_tile_log (W)) - (W - 1);
	}

int gdsp_localmad (const double* d_in, double* d_out, uint32_t n, uint32_t W, int what,
                   double scale, double threshold, int haveMinMad, double minMad, void* stream)
	{
	LmParams P;
	int rc = localmad_params (P, W, what, scale, threshold, haveMinMad, minMad);
	if (rc != GDSP_OK) return rc;
	if (n == 0) return GDSP_OK;
	GDSP_REQUIRE ((d_in != NULL) && (d_out != NULL), "NULL vector");
	GDSP_REQUIRE (d_in != d_out, "out-of-place operator: d_out must not alias d_in");
	gdsp_batch_item item = { d_in, d_out, n };
	return localmad_run (&item, 1, W, P, stream);
	}

int gdsp_localmad_batch (const gdsp_batch_item* items, int nitems, uint32_t W, int what,
                         double scale, double threshold, int haveMinMad, double minMad, void* stream)
	{
	LmParams P;
	int rc = localmad_params (P, W, what, scale, threshold, haveMinMad, minMad);
	if (rc != GDSP_OK) return rc;
	rc = gdsp_batch_check (items, nitems, false);
	if (rc != GDSP_OK) return rc;
	if (nitems == 0) return GDSP_OK;
	return localmad_run (items, nitems, W, P, stream);
	}

} // extern "C"
