// gdsp_rankfilt.hip -- slidingpercentile / median: the exact p-th percentile over a sliding window.
//
// Not an operator of the reference.  Definition (include/genodsp_hip.h): for base i of a vector of n values the
// window is [max(0, i-wL), min(n-1, i+wR)] with wL = (W-1)/2, wR = W-1-wL (bestmax's centring and edge rule,
// minmax.c:1634-1640 in the reference: bases beyond the ends are not considered); with n_i bases in it,
// out[i] is the value of the k_i-th smallest key, k_i = gdsp_percentile_rank(n_i, P), keys as gdsp_key_of (the
// order `percentile` uses: -0.0 folded onto +0.0, NaNs ordered by their bits).  Only comparisons: bit exact.
//
// One workgroup owns T outputs and stages the NS = 2^LOG_N inputs they read (T = NS - (W-1); positions past the
// vector are padding that sorts last).  Per tile the sort and the wavelet matrix of gdsp_rank_tile.h (which
// gdsp_localmad.hip builds too), then one range-quantile query per output over its local range [l, r) with rank k.
// The rank found indexes the sorted local indices, and the value is read back from the input (L2).
// The cost per output is the tile's sort spread over T outputs plus LOG_N levels, whatever the window.  LDS and the
// choice of the tile: gdsp_rank_tile.h.

#include "gdsp_rank_tile.h"

static_assert (2 * (GDSP_SLIDING_PERCENTILE_MAX_WINDOW - 1) < (1 << RF_MAX_LOG), "the largest window must leave half a tile of outputs");

template <int LOG_N>
__device__ __forceinline__
void rankfilt_tile (const double* __restrict__ in, double* __restrict__ out, uint32_t n, uint32_t tile,
                    uint32_t wL, uint32_t wR, uint32_t pThousandths)
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

	rf_tile_build<LOG_N> (S, in, s0, nloc);                                 // stage, sort, matrix

	// ---- one range-quantile query per output
	for (int64_t o=tid ; o<T ; o+=THREADS)
		{
		const int64_t i = o0 + o;
		if (i >= (int64_t) n) break;
		const int64_t first = (i > (int64_t) wL)? i - wL : 0;
		const int64_t last  = (i + wR < (int64_t) n)? i + wR : (int64_t) n - 1;
		const uint32_t lo = (uint32_t) (first - s0), hi = (uint32_t) (last + 1 - s0);
		const uint32_t r  = rf_tile_query<LOG_N> (S, lo, hi, gdsp_rank_of (hi - lo, pThousandths));
		out[i] = gdsp_value_of (gdsp_key_of (in[s0 + S.idx[r]]));            // (the staged copy, from L2; -0.0 folded as the key was)
		}
	}

template <int LOG_N>
__global__ __launch_bounds__((1 << LOG_N) / 8) __attribute__((amdgpu_waves_per_eu ((LOG_N == 13)? 8 : 1)))   // (13: <= 64 VGPRs, two tiles per CU)
void rankfilt_kernel (const double* __restrict__ in, double* __restrict__ out, uint32_t n, uint32_t ntiles,
                      uint32_t wL, uint32_t wR, uint32_t pThousandths)
	{ rankfilt_tile<LOG_N> (in, out, n, gdsp_xcd_tile (blockIdx.x, ntiles), wL, wR, pThousandths); }

template <int LOG_N>                                                        // one grid over every vector of the table (gdsp_common.h)
__global__ __launch_bounds__((1 << LOG_N) / 8) __attribute__((amdgpu_waves_per_eu ((LOG_N == 13)? 8 : 1)))   // (13: <= 64 VGPRs, two tiles per CU)
void rankfilt_batch_kernel (GdspBatch B, uint32_t wL, uint32_t wR, uint32_t pThousandths)
	{
	const double* in;  double* out;  uint32_t n;
	const uint32_t tile = gdsp_batch_tile (B, in, out, n);
	rankfilt_tile<LOG_N> (in, out, n, tile, wL, wR, pThousandths);
	}

template <int LOG_N>
static void rankfilt_launch (const gdsp_batch_item* items, int nitems, uint32_t wL, uint32_t wR, uint32_t P, hipStream_t s)
	{
	const uint64_t T = (1u << LOG_N) - (uint64_t) (wL + wR);
	if (nitems == 1)
		{
		if (items[0].n == 0) return;
		const uint32_t ntiles = (uint32_t) (((uint64_t) items[0].n + T - 1) / T);
		hipLaunchKernelGGL ((rankfilt_kernel<LOG_N>), dim3(ntiles), dim3((1 << LOG_N) / 8), 0, s,
		                    items[0].d_in, items[0].d_out, items[0].n, ntiles, wL, wR, P);
		return;
		}
	gdsp_batch_run (items, nitems, [=] (uint32_t n) { return ((uint64_t) n + T - 1) / T; },
		[&] (const GdspBatch& B, uint32_t tiles)
			{
			hipLaunchKernelGGL ((rankfilt_batch_kernel<LOG_N>), dim3(tiles), dim3((1 << LOG_N) / 8), 0, s, B, wL, wR, P);
			});
	}

static int rankfilt_run (const gdsp_batch_item* items, int nitems, uint32_t W, uint32_t P, void* stream)
	{
	const uint32_t wL = (W - 1) / 2, wR = (W - 1) - wL;
	hipStream_t s = gdsp_stream (stream);
	switch (rf_tile_log (W))
		{
		case 10: rankfilt_launch<10> (items, nitems, wL, wR, P, s);  break;
		case 11: rankfilt_launch<11> (items, nitems, wL, wR, P, s);  break;
		case 12: rankfilt_launch<12> (items, nitems, wL, wR, P, s);  break;
		default: rankfilt_launch<13> (items, nitems, wL, wR, P, s);  break;
		}
	GDSP_LAUNCH_CHECK ();
	return GDSP_OK;
	}

extern "C" {

uint32_t gdsp_sliding_percentile_tile (uint32_t W)
	{
	if ((W < 1) || (W > GDSP_SLIDING_PERCENTILE_MAX_WINDOW)) return 0;
	return (1u << rf_tile_log (W)) - (W - 1);
	}

int gdsp_sliding_percentile (const double* d_in, double* d_out, uint32_t n, uint32_t W, uint32_t pThousandths, void* stream)
	{
	GDSP_REQUIRE (W >= 1, "window must be >= 1");
	GDSP_REQUIRE (W <= GDSP_SLIDING_PERCENTILE_MAX_WINDOW, "window above GDSP_SLIDING_PERCENTILE_MAX_WINDOW");
	GDSP_REQUIRE (pThousandths <= 100000, "percentile above 100 (100000 thousandths)");
	if (n == 0) return GDSP_OK;
	GDSP_REQUIRE ((d_in != NULL) && (d_out != NULL), "NULL vector");
	GDSP_REQUIRE (d_in != d_out, "out-of-place operator: d_out must not alias d_in");
	gdsp_batch_item item = { d_in, d_out, n };
	return rankfilt_run (&item, 1, W, pThousandths, stream);
	}

int gdsp_sliding_percentile_batch (const gdsp_batch_item* items, int nitems, uint32_t W, uint32_t pThousandths, void* stream)
	{
	GDSP_REQUIRE (W >= 1, "window must be >= 1");
	GDSP_REQUIRE (W <= GDSP_SLIDING_PERCENTILE_MAX_WINDOW, "window above GDSP_SLIDING_PERCENTILE_MAX_WINDOW");
	GDSP_REQUIRE (pThousandths <= 100000, "percentile above 100 (100000 thousandths)");
	int rc = gdsp_batch_check (items, nitems, false);
	if (rc != GDSP_OK) return rc;
	if (nitems == 0) return GDSP_OK;
	return rankfilt_run (items, nitems, W, pThousandths, stream);
	}

} // extern "C"
