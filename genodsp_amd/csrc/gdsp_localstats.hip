// gdsp_localstats.hip -- localstats: every base against the mean and variance of the window centred on it.
//
// Not an operator of the reference.  Definition (include/genodsp_hip.h): slidingsum's window [lo, hi] =
// [max(0, c-lft), min(n-1, c+rgt)], rgt = (W-1)/2, lft = W-1-rgt, m = hi-lo+1; S1 = sum of v, S2 = sum of fl(v v) over
// it; mean = fl(S1/m), N = fl(fl(m S2) - fl(S1 S1)), variance = N <= 0 ? +0 : fl(N / fl(m m)), stddev = sqrt(variance);
// the written value is one of them, or v relative to them.  Every step is one rounded operation (__dmul_rn and friends:
// never contracted); only the two window sums may be associated freely.
//
// The tile -- the staged inputs in LDS, the block sums and their scan, P(e), the slide, the choice of outputs per thread and
// the trip of the results through LDS -- is gdsp_window_sums_tile.h's, which localcorrelate shares; its comments hold the
// layout and its reasons.  Here: the terms (v, fl(v v)), the figure, and the two forms: 512 threads and 8192 staged
// values (76.3 KiB of LDS, two workgroups per CU) while that leaves a tile of at least 4096 outputs, 1024 threads and
// 16384 staged values (152.4 KiB, one per CU) for the longer windows.

#include "gdsp_window_sums_tile.h"

#define LS_SMALL    512                                                   // threads of the two forms
#define LS_LARGE    1024
#define LS_MIN_TILE 4096                                                  // the small form is used while its tile is at least this
#define LS_NWHAT    6

struct LsTerms                                                            // S1 = sum of v, S2 = sum of fl(v v)
	{
	static constexpr int INPUTS = 1, SUMS = 2;
	static __device__ __forceinline__ void add (double p[SUMS], const double in[INPUTS])
		{ p[0] = __dadd_rn (p[0], in[0]);  p[1] = __dadd_rn (p[1], __dmul_rn (in[0], in[0])); }
	};
template <int THREADS> using LsLds = WsLds<THREADS, LsTerms::INPUTS, LsTerms::SUMS>;
static_assert (2 * sizeof (LsLds<LS_SMALL>) <= 160 * 1024, "two workgroups per CU");
static_assert (sizeof (LsLds<LS_LARGE>) <= 160 * 1024, "one workgroup per CU");

// host and device: the form and the outputs per tile
__host__ __device__ constexpr bool     ls_small (uint32_t lft, uint32_t rgt) { return ws_even (lft) + ws_even (rgt) + LS_MIN_TILE <= LS_SMALL * WS_G; }
__host__ __device__ constexpr uint32_t ls_tile (uint32_t lft, uint32_t rgt) { return ws_tile (ls_small (lft, rgt)? LS_SMALL : LS_LARGE, lft, rgt); }
static_assert (ls_tile ((GDSP_LOCALSTATS_MAX_WINDOW - 1) - (GDSP_LOCALSTATS_MAX_WINDOW - 1) / 2, (GDSP_LOCALSTATS_MAX_WINDOW - 1) / 2) == LS_MIN_TILE,
               "the largest window leaves the long form a tile of 4096 outputs");

struct LsArgs { WsArgs win;  int haveFloor, haveMinSd;  double floor, minSd; };

template <int WHAT>
__device__ __forceinline__ double ls_figure (double x, double S1, double S2, double md, const LsArgs& A)
	{
	const double mean = __ddiv_rn (S1, md);
	if ((WHAT == GDSP_LOCALSTATS_MEAN) || (WHAT == GDSP_LOCALSTATS_DIFFERENCE) || (WHAT == GDSP_LOCALSTATS_RATIO))
		{
		const double bg = (A.haveFloor && (A.floor > mean))? A.floor : mean;
		if (WHAT == GDSP_LOCALSTATS_MEAN)       return bg;
		if (WHAT == GDSP_LOCALSTATS_DIFFERENCE) return __dsub_rn (x, bg);
		return (bg == 0.0)? 0.0 : __ddiv_rn (x, bg);
		}
	const double N   = __dsub_rn (__dmul_rn (md, S2), __dmul_rn (S1, S1));
	const double var = (N <= 0.0)? 0.0 : __ddiv_rn (N, __dmul_rn (md, md));
	if (WHAT == GDSP_LOCALSTATS_VARIANCE) return var;
	double sd = __dsqrt_rn (var);
	if (A.haveMinSd && (A.minSd > sd)) sd = A.minSd;
	if (WHAT == GDSP_LOCALSTATS_STDDEV) return sd;
	return (sd == 0.0)? 0.0 : __ddiv_rn (__dsub_rn (x, mean), sd);
	}

template <int THREADS, int WHAT>
__global__ __launch_bounds__(THREADS)
void localstats_kernel (GdspBatch B, LsArgs A)                            // one grid over every vector of the table (gdsp_common.h)
	{
	__shared__ __attribute__((aligned(16))) LsLds<THREADS> S;
	const double* in;  double* out;  uint32_t n;
	const uint32_t tile = gdsp_batch_tile (B, in, out, n);
	const WsTile   t    = ws_tile_of<THREADS> (A.win, tile);
	ws_stage<THREADS> (S.v[0], in, t.g0, n);
	ws_block_sums<THREADS, LsTerms> (S);
	ws_outputs<THREADS, LsTerms> (S, A.win, t, n, out, [A] (int e, const double* sums, double md)
		{ return ls_figure<WHAT> (S.v[0][ws_at (e)], sums[0], sums[1], md, A); });
	}

template <int THREADS>
static void localstats_launch (const GdspBatch& B, uint32_t tiles, int what, const LsArgs& A, hipStream_t s)
	{
	switch (what)
		{
		case GDSP_LOCALSTATS_ZSCORE:     hipLaunchKernelGGL ((localstats_kernel<THREADS, GDSP_LOCALSTATS_ZSCORE>),     dim3(tiles), dim3(THREADS), 0, s, B, A);  break;
		case GDSP_LOCALSTATS_MEAN:       hipLaunchKernelGGL ((localstats_kernel<THREADS, GDSP_LOCALSTATS_MEAN>),       dim3(tiles), dim3(THREADS), 0, s, B, A);  break;
		case GDSP_LOCALSTATS_VARIANCE:   hipLaunchKernelGGL ((localstats_kernel<THREADS, GDSP_LOCALSTATS_VARIANCE>),   dim3(tiles), dim3(THREADS), 0, s, B, A);  break;
		case GDSP_LOCALSTATS_STDDEV:     hipLaunchKernelGGL ((localstats_kernel<THREADS, GDSP_LOCALSTATS_STDDEV>),     dim3(tiles), dim3(THREADS), 0, s, B, A);  break;
		case GDSP_LOCALSTATS_DIFFERENCE: hipLaunchKernelGGL ((localstats_kernel<THREADS, GDSP_LOCALSTATS_DIFFERENCE>), dim3(tiles), dim3(THREADS), 0, s, B, A);  break;
		default:                         hipLaunchKernelGGL ((localstats_kernel<THREADS, GDSP_LOCALSTATS_RATIO>),      dim3(tiles), dim3(THREADS), 0, s, B, A);  break;
		}
	}

static int localstats_run (const gdsp_batch_item* items, int nitems, uint32_t W, int what,
                           int haveFloor, double floor, int haveMinSd, double minSd, void* stream)
	{
	LsArgs A;
	WsArgs& win = A.win;
	win = ws_window (W);
	const bool     small = ls_small (win.lft, win.rgt);
	const uint64_t T     = ls_tile (win.lft, win.rgt);
	win.per = ws_per ((uint32_t) T, small? LS_SMALL : LS_LARGE);
	A.haveFloor = haveFloor? 1 : 0;  A.floor = floor;  A.haveMinSd = haveMinSd? 1 : 0;  A.minSd = minSd;
	hipStream_t s = gdsp_stream (stream);
	gdsp_batch_run (items, nitems, [=] (uint32_t n) { return ((uint64_t) n + T - 1) / T; },
		[&] (const GdspBatch& B, uint32_t tiles)
			{
			if (small) localstats_launch<LS_SMALL> (B, tiles, what, A, s);
			else       localstats_launch<LS_LARGE> (B, tiles, what, A, s);
			});
	GDSP_LAUNCH_CHECK ();
	return GDSP_OK;
	}

#define LS_CHECK_ARGS() \
	GDSP_REQUIRE (W >= 1, "window must be >= 1"); \
	GDSP_REQUIRE (W <= GDSP_LOCALSTATS_MAX_WINDOW, "window above GDSP_LOCALSTATS_MAX_WINDOW"); \
	GDSP_REQUIRE ((what >= 0) && (what < LS_NWHAT), "what must be one of GDSP_LOCALSTATS_ZSCORE ... GDSP_LOCALSTATS_RATIO")

extern "C" {

uint32_t gdsp_localstats_tile (uint32_t W)
	{
	if ((W < 1) || (W > GDSP_LOCALSTATS_MAX_WINDOW)) return 0;
	const uint32_t rgt = (W - 1) / 2;
	return ls_tile ((W - 1) - rgt, rgt);
	}

int gdsp_localstats (const double* d_in, double* d_out, uint32_t n, uint32_t W, int what,
                     int haveFloor, double floor, int haveMinSd, double minSd, void* stream)
	{
	LS_CHECK_ARGS ();
	GDSP_REQUIRE ((n == 0) || (d_in != d_out), "out-of-place operator: d_out must not alias d_in");
	if (n == 0) return GDSP_OK;
	GDSP_REQUIRE ((d_in != NULL) && (d_out != NULL), "NULL vector");
	GDSP_REQUIRE (gdsp_aligned16 (d_in) && gdsp_aligned16 (d_out), "vectors must be 16-byte aligned");
	gdsp_batch_item item = { d_in, d_out, n };
	return localstats_run (&item, 1, W, what, haveFloor, floor, haveMinSd, minSd, stream);      // the same kernel, a table of one
	}

int gdsp_localstats_batch (const gdsp_batch_item* items, int nitems, uint32_t W, int what,
                           int haveFloor, double floor, int haveMinSd, double minSd, void* stream)
	{
	LS_CHECK_ARGS ();
	int rc = gdsp_batch_check (items, nitems, false);
	if (rc != GDSP_OK) return rc;
	if (nitems == 0) return GDSP_OK;
	return localstats_run (items, nitems, W, what, haveFloor, floor, haveMinSd, minSd, stream);
	}

} // extern "C"
