// gdsp_lagcorr.hip -- crosscorrelate / autocorrelate (not in the reference): the covariance of x against y shifted by
// every lag of a range, exactly (include/genodsp_hip.h has the definitions).  For each lag d the products
// fl(fl(x[i] - meanx) * fl(y[i+d] - meany)) over the positions where both are finite and inside the chromosome are summed
// into an integer image of their own (gdsp_xsum.hip's); the host rounds each image once.  N bases times D lags products:
// the one pass of the project that is bound by the FP64 pipe, not by HBM.
//
// A workgroup is four waves and LG_BLOCK = 256 lags (blockIdx.y picks the block): lane l of every wave owns the
// LG_LPL = 4 consecutive lags 4l .. 4l+3 of the block, the waves split a tile of LG_TILE positions in four.  The tile's
// dx and the tile's dy widened by the block of lags are staged in LDS, centred at the load; dy lies there in LG_LPL
// planes by index modulo 4, so that the one new value a lane needs per position (its window of dy slides by one) is
// at consecutive addresses over the lanes.  Per four positions a lane reads four dx (broadcast) and four new dy, and
// grows its four two-term expansions by sixteen products, TwoSum unchecked; a residual that is not exactly zero (a real
// one, or the NaN of an overflow or of a product that is not finite) sends the lane back to the expansions it had before
// those sixteen and through them the careful way (xs_grow: residuals go to the lag's device image; products that are not
// finite are counted).  Expansions, counts and INF counts stay in registers over all the tiles of a workgroup and are
// deposited once at its end: grid x lags atomics, not tiles x lags.
//
// Only a clean tile takes that route: a whole tile, with y inside the chromosome for every lag of the block, and no
// value or centred value that is not finite.  There every product is taken and the count is arithmetic.  Any other tile
// -- the two ends of a chromosome, chromosomes shorter than a tile, stretches with NaN -- is walked from global memory
// position by position with every test spelled out (exact, not fast).

#include <float.h>
#include <math.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "gdsp_common.h"
#include "gdsp_xsum_dev.h"

#define LG_THREADS   256
#define LG_WAVES     (LG_THREADS / 64)
#define LG_LPL       4                                // consecutive lags of a lane
#define LG_BLOCK     (64 * LG_LPL)                    // lags of a workgroup
#define LG_TILE      1024                             // positions of a tile
#define LG_WPOS      (LG_TILE / LG_WAVES)             // positions of a wave in a tile
#define LG_PLANE     328                              // slots of a plane of dy: (LG_TILE + LG_BLOCK) / LG_LPL = 320, and 8 so
                                                      // that the planes start 64 bytes apart modulo 128 (the staging writes)
#define LG_MAX_LAGS  4096
#define LG_WG_TARGET (256 * 4)                        // workgroups of a launch: all resident, equal shares
#define LG_LAUNCH_TILES ((1u << 28) / LG_TILE)        // tiles of a launch: were every product of it to flush, a word of a
                                                      // lag's image still grows by less than 2^28 * 2 * 2^32 before the carry
#define LG_W         GDSP_XSUM_WORDS

static_assert ((LG_TILE + LG_BLOCK) / LG_LPL <= LG_PLANE, "a plane holds the widened tile");
static_assert (LG_WPOS % 4 == 0, "a wave walks its positions four at a time");

struct LagBatch
	{
	const double* x[GDSP_BATCH_MAX];
	const double* y[GDSP_BATCH_MAX];
	uint32_t      n[GDSP_BATCH_MAX];
	uint32_t      tile0[GDSP_BATCH_MAX + 1];          // pair v owns the tiles [tile0[v], tile0[v+1])
	};

// a[] += p exactly, p any double: a p that is not finite is counted and not added
__device__ __forceinline__ void lag_take (double (&a)[XS_K], double p, unsigned long long* img, uint32_t& infs)
	{
	if (xs_finite (p)) xs_grow (a, p, img);
	else               infs++;
	}

__device__ __forceinline__ int lag_dy_slot (int p) { return (p & (LG_LPL-1)) * LG_PLANE + (p >> 2); }

__global__ __launch_bounds__(LG_THREADS)
void lag_kernel (LagBatch P, uint32_t tLo, uint32_t tHi, int32_t lagLo, uint32_t nlags, double meanx, double meany,
                 unsigned long long* __restrict__ d_acc)
	{
	__shared__ double dxL[LG_TILE];
	__shared__ double dyL[LG_LPL * LG_PLANE];

	const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t k0   = blockIdx.y * LG_BLOCK;                          // the block's first lag, as an index
	const uint32_t kAct = (nlags - k0 < LG_BLOCK)? nlags - k0 : LG_BLOCK; // its lags
	const int64_t  dlo  = (int64_t) lagLo + k0, dhi = dlo + kAct - 1;
	const uint32_t myk  = k0 + lane * LG_LPL;                             // the lane's first lag, as an index

	double   a[LG_LPL][XS_K];
	uint64_t cnt[LG_LPL], clean = 0;
	uint32_t infs[LG_LPL];
#pragma unroll
	for (int j=0 ; j<LG_LPL ; j++) { a[j][0] = a[j][1] = 0.0;  cnt[j] = 0;  infs[j] = 0; }

	uint32_t v = 0;
	for (uint32_t g=tLo+blockIdx.x ; g<tHi ; g+=gridDim.x)
		{
		while (g >= P.tile0[v+1]) v++;
		const double* __restrict__ gx = P.x[v];
		const double* __restrict__ gy = P.y[v];
		const int64_t n  = P.n[v];
		const int64_t t0 = (int64_t) (g - P.tile0[v]) * LG_TILE;
		if ((t0 + LG_TILE - 1 + dhi < 0) || (t0 + dlo >= n)) continue;        // no x[i] of the tile meets a y[i+d] of the block

		const bool inside = (t0 + LG_TILE <= n) && (t0 + dlo >= 0) && (t0 + LG_TILE - 1 + dhi < n);
		bool fast = false;
		if (inside)
			{
			int dirty = 0;
			for (int k=threadIdx.x ; k<LG_TILE ; k+=LG_THREADS)
				{
				const double x = gx[t0 + k], dx = __dsub_rn (x, meanx);
				dirty |= !xs_finite (x) || !xs_finite (dx);
				dxL[k] = dx;
				}
			const int need = LG_TILE + (int) kAct - 1;                        // values of y the block's lags reach
			for (int p=threadIdx.x ; p<LG_TILE+LG_BLOCK ; p+=LG_THREADS)
				{
				double dy = 0.0;
				if (p < need)
					{
					const double y = gy[t0 + dlo + p];
					dy = __dsub_rn (y, meany);
					dirty |= !xs_finite (y) || !xs_finite (dy);
					}
				dyL[lag_dy_slot (p)] = dy;
				}
			fast = !__syncthreads_or (dirty);
			}

		if (fast)
			{
			clean += LG_WPOS;
			const double* plane = dyL + lane;
			int s = (wave * LG_WPOS) >> 2;
			double w[2*LG_LPL - 1];
#pragma unroll
			for (int k=0 ; k<LG_LPL-1 ; k++) w[k] = plane[k*LG_PLANE + s];
#pragma unroll 1
			for (int i=wave*LG_WPOS ; i<(wave+1)*LG_WPOS ; i+=LG_LPL, s++)
				{
				w[LG_LPL-1] = plane[(LG_LPL-1)*LG_PLANE + s];
#pragma unroll
				for (int k=0 ; k<LG_LPL-1 ; k++) w[LG_LPL+k] = plane[k*LG_PLANE + s + 1];
				double dx[LG_LPL], keep[LG_LPL][XS_K];
#pragma unroll
				for (int u=0 ; u<LG_LPL ; u++) dx[u] = dxL[i+u];
				bool bad = false;
#pragma unroll
				for (int j=0 ; j<LG_LPL ; j++) { keep[j][0] = a[j][0];  keep[j][1] = a[j][1]; }
#pragma unroll
				for (int u=0 ; u<LG_LPL ; u++)
#pragma unroll
					for (int j=0 ; j<LG_LPL ; j++)
						{
						double r = __dmul_rn (dx[u], w[u+j]);
#pragma unroll
						for (int k=0 ; k<XS_K ; k++)
							{
							const double t  = __dadd_rn (a[j][k], r);
							const double bp = __dsub_rn (t, a[j][k]);
							r       = __dadd_rn (__dsub_rn (a[j][k], __dsub_rn (t, bp)), __dsub_rn (r, bp));
							a[j][k] = t;
							}
						bad |= (r != 0.0);
						}
				if (bad)
					{
#pragma unroll
					for (int j=0 ; j<LG_LPL ; j++) { a[j][0] = keep[j][0];  a[j][1] = keep[j][1]; }
#pragma unroll 1
					for (int u=0 ; u<LG_LPL ; u++)
						{
						const double dxu = dxL[i+u];
#pragma unroll
						for (int j=0 ; j<LG_LPL ; j++)
							{
							if (myk + j >= nlags) continue;
							const double p = __dmul_rn (dxu, dyL[lag_dy_slot (i + u + lane*LG_LPL + j)]);
							lag_take (a[j], p, d_acc + (size_t) (myk + j) * LG_W, infs[j]);
							}
						}
					}
#pragma unroll
				for (int k=0 ; k<LG_LPL-1 ; k++) w[k] = w[LG_LPL+k];
				}
			}
		else
			{
			const int64_t iLo = t0 + wave * LG_WPOS;
			const int64_t iHi = (iLo + LG_WPOS < n)? iLo + LG_WPOS : n;
#pragma unroll
			for (int j=0 ; j<LG_LPL ; j++)
				{
				if (myk + j >= nlags) continue;
				const int64_t d = (int64_t) lagLo + myk + j;
				unsigned long long* img = d_acc + (size_t) (myk + j) * LG_W;
				int64_t lo = (iLo > -d)? iLo : -d;                              // 0 <= i + d < n
				int64_t hi = (iHi < n - d)? iHi : n - d;
#pragma unroll 1
				for (int64_t i=lo ; i<hi ; i++)
					{
					const double x = gx[i], y = gy[i + d];
					if (!xs_finite (x) || !xs_finite (y)) continue;
					cnt[j]++;
					lag_take (a[j], __dmul_rn (__dsub_rn (x, meanx), __dsub_rn (y, meany)), img, infs[j]);
					}
				}
			}
		if (inside) __syncthreads ();                                         // (the tile is read; the next one may be staged)
		}

#pragma unroll
	for (int j=0 ; j<LG_LPL ; j++)
		{
		if (myk + j >= nlags) continue;
		unsigned long long* img = d_acc + (size_t) (myk + j) * LG_W;
#pragma unroll
		for (int k=0 ; k<XS_K ; k++) xs_deposit (img, a[j][k]);
		const uint64_t c = cnt[j] + clean;
		if (c != 0)       atomicAdd (&img[GDSP_XSUM_WORD_COUNT], (unsigned long long) c);
		if (infs[j] != 0) atomicAdd (&img[GDSP_XSUM_WORD_INF],   (unsigned long long) infs[j]);
		}
	}

// every image in canonical digits: the launches' images then add without overflow, and equal sums are equal words
__global__ void lag_carry_kernel (unsigned long long* __restrict__ d_acc, uint32_t nlags)
	{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k < nlags) xs_carry (d_acc + (size_t) k * LG_W);
	}

extern "C" {

uint32_t gdsp_lag_tile  (void) { return LG_TILE; }
uint32_t gdsp_lag_block (void) { return LG_BLOCK; }

int gdsp_lag_products_batch (const gdsp_xsum_pair* pairs, int npairs, int32_t lagLo, uint32_t nlags, double meanx, double meany,
                             uint64_t* d_acc, void* stream)
	{
	GDSP_REQUIRE (d_acc != NULL, "NULL accumulator");
	GDSP_REQUIRE ((npairs == 0) || (pairs != NULL), "NULL pairs");
	GDSP_REQUIRE ((nlags >= 1) && (nlags <= LG_MAX_LAGS), "the number of lags must be 1 .. 4096");
	GDSP_REQUIRE ((int64_t) lagLo + nlags - 1 <= INT32_MAX, "the last lag is beyond int32");
	GDSP_REQUIRE ((fabs (meanx) <= DBL_MAX) && (fabs (meany) <= DBL_MAX), "the means must be finite");
	for (int i=0 ; i<npairs ; i++)
		GDSP_REQUIRE (((((uintptr_t) pairs[i].d_x) | ((uintptr_t) pairs[i].d_y)) & 7) == 0, "both vectors of a pair must be 8-byte aligned");
	hipStream_t s = gdsp_stream (stream);
	unsigned long long* acc = reinterpret_cast<unsigned long long*> (d_acc);
	const uint32_t lagBlocks = (nlags + LG_BLOCK - 1) / LG_BLOCK;
	int i = 0;
	while (i < npairs)
		{
		LagBatch B;
		int k = 0;
		B.tile0[0] = 0;
		for ( ; (i<npairs) && (k<GDSP_BATCH_MAX) ; i++)
			{
			if (pairs[i].n == 0) continue;
			B.x[k] = pairs[i].d_x;  B.y[k] = pairs[i].d_y;  B.n[k] = pairs[i].n;
			B.tile0[k+1] = B.tile0[k] + (uint32_t) (((uint64_t) pairs[i].n + LG_TILE - 1) / LG_TILE);
			k++;
			}
		for (int j=k ; j<GDSP_BATCH_MAX ; j++) { B.x[j] = NULL;  B.y[j] = NULL;  B.n[j] = 0;  B.tile0[j+1] = B.tile0[k]; }
		const uint32_t tiles = B.tile0[k];
		for (uint32_t tLo=0 ; tLo<tiles ; tLo+=LG_LAUNCH_TILES)
			{
			const uint32_t tHi = (tiles - tLo < LG_LAUNCH_TILES)? tiles : tLo + LG_LAUNCH_TILES;
			uint32_t gx = LG_WG_TARGET / lagBlocks;
			if (gx > tHi - tLo) gx = tHi - tLo;
			hipLaunchKernelGGL (lag_kernel, dim3 (gx, lagBlocks), dim3 (LG_THREADS), 0, s, B, tLo, tHi, lagLo, nlags, meanx, meany, acc);
			GDSP_LAUNCH_CHECK ();
			hipLaunchKernelGGL (lag_carry_kernel, dim3 ((nlags + 63) / 64), dim3 (64), 0, s, acc, nlags);
			GDSP_LAUNCH_CHECK ();
			}
		}
	return GDSP_OK;
	}

} // extern "C"

// ------------------------------------------------------------------------------------------- end to end ----
static gdsp_comm* lgComm = NULL;                             // see gdsp_genome_lag_correlation_use_comm
static uint64_t   lgLast[8];                                 // see gdsp_genome_lag_correlation_last

// fl(a * b), never contracted into what follows
static double lg_mul (double a, double b) { volatile double p = a * b;  return p; }

extern "C" {

int gdsp_genome_lag_correlation_use_comm (gdsp_comm* comm) { lgComm = comm;  return GDSP_OK; }

void gdsp_genome_lag_correlation_last (uint64_t out[8]) { memcpy (out, lgLast, sizeof(lgLast)); }

int gdsp_genome_lag_correlation (const gdsp_xsum_pair* pairs, int npairs, int32_t lagLo, uint32_t nlags, gdsp_reduce_fn reduce,
                                 void* reduceCtx, double* fig, uint64_t* count, double* cov, double* corr)
	{
	GDSP_REQUIRE ((fig != NULL) && (count != NULL) && (cov != NULL) && (corr != NULL), "NULL result");
	GDSP_REQUIRE ((npairs == 0) || (pairs != NULL), "NULL pairs");
	GDSP_REQUIRE ((nlags >= 1) && (nlags <= LG_MAX_LAGS), "the number of lags must be 1 .. 4096");
	GDSP_REQUIRE ((int64_t) lagLo + nlags - 1 <= INT32_MAX, "the last lag is beyond int32");
	GDSP_REQUIRE (!((lgComm != NULL) && (reduce != NULL)), "a host reduction hook next to a communicator");
	memset (lgLast, 0, sizeof(lgLast));

	// the sample's figures: correlate's two passes over whole chromosomes, window 1, no limits
	std::vector<gdsp_xsum_pair> whole (pairs, pairs + std::max (npairs, 0));
	for (auto& p : whole) p.first = 0;
	int rc = gdsp_genome_correlation (whole.data (), npairs, 1, -DBL_MAX, DBL_MAX, -DBL_MAX, DBL_MAX, reduce, reduceCtx, fig);
	if (rc != GDSP_OK) return rc;
	const uint64_t n = (uint64_t) fig[GDSP_CORR_COUNT];
	lgLast[0] = n;
	for (uint32_t k=0 ; k<nlags ; k++) { count[k] = 0;  cov[k] = corr[k] = NAN; }
	if (n == 0) return GDSP_OK;                                  // (no means to centre on)
	const double meanx = fig[GDSP_CORR_MEANX], meany = fig[GDSP_CORR_MEANY];

	std::vector<gdsp_xsum_source> xs (whole.size ());
	for (size_t i=0 ; i<whole.size () ; i++)
		{ xs[i].d_v = whole[i].d_x;  xs[i].n = whole[i].n;  xs[i].first = 0;  xs[i].device = whole[i].device;  xs[i].stream = whole[i].stream; }
	const size_t words = (size_t) nlags * LG_W;
	std::vector<uint64_t> img (words);
	std::vector<gdsp_xsum_pair> mine;
	auto onDevice = [&] (const gdsp_xsum_source* its, int nits, uint64_t* d_acc, void* stream) -> int
		{
		// (as xp_genome_pass of gdsp_xsum_pair.hip: a device's pairs are those whose x it was handed)
		mine.clear ();
		for (int i=0 ; (i<npairs) && (nits>0) ; i++) { if (whole[i].device == its[0].device) mine.push_back (whole[i]); }
		GDSP_REQUIRE ((int) mine.size () == nits, "the pairs of a device are not its sources");
		for (int i=0 ; i<nits ; i++) GDSP_REQUIRE (mine[i].d_x == its[i].d_v, "the pairs of a device are not its sources");
		GDSP_HIP_TRY (hipMemsetAsync (d_acc, 0, words * sizeof(uint64_t), gdsp_stream (stream)));
		return gdsp_lag_products_batch (mine.data (), nits, lagLo, nlags, meanx, meany, d_acc, stream);
		};
	rc = gdsp_reduce_sources ("gdsp_genome_lag_correlation", "accumulators", lgComm, xs.data (), npairs, words, onDevice,
	                          reduce, reduceCtx, img.data ());
	if (rc != GDSP_OK) return rc;

	const double varx = fig[GDSP_CORR_VARX], vary = fig[GDSP_CORR_VARY];
	const bool xok = (varx > 0) && (varx <= DBL_MAX), yok = (vary > 0) && (vary <= DBL_MAX);
	int ex = 0, ey = 0;
	const double mx = frexp (fig[GDSP_CORR_SDX], &ex), my = frexp (fig[GDSP_CORR_SDY], &ey);
	for (uint32_t k=0 ; k<nlags ; k++)
		{
		const uint64_t* w = img.data () + (size_t) k * LG_W;
		count[k]   = w[GDSP_XSUM_WORD_COUNT];
		lgLast[1] += w[GDSP_XSUM_WORD_COUNT];
		lgLast[2] += w[GDSP_XSUM_WORD_FLUSHES];
		lgLast[3] += w[GDSP_XSUM_WORD_INF];
		if (w[GDSP_XSUM_WORD_INF] != 0) continue;                // (cov and corr stay NaN)
		cov[k] = gdsp_xsum_div_round (w, n);
		if (!(xok && yok)) continue;
		double r = ldexp (cov[k], -(ex + ey)) / lg_mul (mx, my);
		if (r >  1.0) r =  1.0;
		if (r < -1.0) r = -1.0;
		corr[k] = r;
		}
	return GDSP_OK;
	}

} // extern "C"
