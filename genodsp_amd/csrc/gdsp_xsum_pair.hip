// gdsp_xsum_pair.hip -- correlate (not in the reference): the signal against a second track, exactly.  Two signals are
// walked together over the pair sample (gdsp_sample.h: x's sample, of which the pairs count whose x AND y pass their
// limits and are finite), and the exact sums of x and y, then of the squared and crossed deviations from their means,
// are each rounded once, on the host, at the end (include/genodsp_hip.h has the definitions).
//
// The accumulator is gdsp_xsum.hip's integer image, one per sum, side by side: pass 1 fills two (Sx, Sy), pass 2 three
// (sum of qxx, of qyy, of qxy).  Every image carries n in its count word and its own INF and FLUSHES words.  Integer
// words add associatively, so the images of a genome do not depend on the cut into pairs, devices or ranks, on the
// grid or on the dispatch order.
//
// The pass (xsum_pair_kernel) is xsum_kernel with two streams: the frame is x's 16-byte frame, tiles of XP_TILE values,
// XP_UNROLL 16-byte loads in flight per lane and stream (as many bytes per lane as xsum_kernel has for its one).  A y
// that is congruent to x modulo 16 bytes -- always so in the driver, where vector and partner share their offset --
// takes the same 16-byte loads; any other y is read value by value (exact, not fast).  Each lane grows two expansions
// per sum (gdsp_xsum_dev.h); the wave tree, the carry and the integer atomics to the device images are xsum_kernel's.
//
// Pass 2 per pair: dx = fl(x - meanx), dy = fl(y - meany), qxx = fl(dx dx), qyy = fl(dy dy), qxy = fl(dx dy)
// (__dsub_rn / __dmul_rn: never contracted).  A q that is not finite (+inf, -inf, or the NaN of inf * 0) is counted in
// its image's GDSP_XSUM_WORD_INF and not added.

#include <float.h>
#include <math.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "gdsp_common.h"
#include "gdsp_xsum_dev.h"
#include "gdsp_sample.h"
#include "gdsp_corr_derive.h"

#define XP_THREADS    256
#define XP_UNROLL     4                               // 16-byte loads in flight per lane and stream
#define XP_TILE       (XP_THREADS * XP_UNROLL * 2)    // 2048 pairs = 16 KiB of each stream
#define XP_MAX_BLOCKS (256 * 4)                       // every workgroup resident: equal shares finish together
#define XP_W          GDSP_XSUM_WORDS

static_assert (GDSP_BATCH_MAX <= 32, "GdspSamplePair.same is a mask of 32 bits");

// PASS 1 adds x and y, PASS 2 adds qxx, qyy and qxy; WINDOWED: the window is above 1
template <int PASS, bool WINDOWED>
__global__ __launch_bounds__(XP_THREADS)
void xsum_pair_kernel (GdspSamplePair P, uint32_t window, double lo, double hi, double ylo, double yhi, double meanx,
                       double meany, unsigned long long* __restrict__ d_acc)
	{
	constexpr int NI = (PASS == 1)? 2 : 3;                // images
	__shared__ unsigned long long acc[NI * XP_W];
	for (int i=threadIdx.x ; i<NI*XP_W ; i+=XP_THREADS) acc[i] = 0;
	__syncthreads ();

	double a[NI][2][XS_K];                                // per sum, one expansion for each value of a 16-byte load
#pragma unroll
	for (int s=0 ; s<NI ; s++)
#pragma unroll
		for (int h=0 ; h<2 ; h++)
#pragma unroll
			for (int k=0 ; k<XS_K ; k++) a[s][h][k] = 0.0;
	uint32_t cnt = 0, infs[NI];
#pragma unroll
	for (int s=0 ; s<NI ; s++) infs[s] = 0;

	auto take = [&] (const int h, double x, double y, bool sampled)
		{
		const bool in = sampled && !(x < lo) && !(x > hi) && xs_finite (x) && !(y < ylo) && !(y > yhi) && xs_finite (y);
		cnt += in;
		double t[NI];
		if (PASS == 1) { t[0] = x;  t[1] = y; }
		else
			{
			const double dx = __dsub_rn (x, meanx), dy = __dsub_rn (y, meany);
			t[0] = __dmul_rn (dx, dx);  t[1] = __dmul_rn (dy, dy);  t[NI-1] = __dmul_rn (dx, dy);
			}
#pragma unroll
		for (int s=0 ; s<NI ; s++)
			{
			const bool big = (PASS == 2) && in && !xs_finite (t[s]);          // q = +-inf or NaN
			infs[s] += big;
			xs_grow (a[s][h], (in && !big)? t[s] : 0.0, acc + s*XP_W);
			}
		};

	const uint32_t T = P.x.tile0[P.x.nvec];
	uint32_t v = 0;
	for (uint32_t g=blockIdx.x ; g<T ; g+=gridDim.x)
		{
		const GdspSamplePairTile t = gdsp_sample_pair_tile<XP_TILE> (P, g, v);
		v = t.x.v;
		const double*  xb = t.x.base;
		const double*  yb = t.ybase;
		const uint64_t m = t.x.m, j0 = t.x.j0, lead = t.x.lead;
		auto sampled = [&] (uint64_t j) -> bool { return gdsp_sampled<WINDOWED> (t.x, window, j); };
		if ((j0 + XP_TILE <= m) && t.same)
			{
			const double2* p = reinterpret_cast<const double2*> (xb + j0) + threadIdx.x;
			const double2* q = reinterpret_cast<const double2*> (yb + j0) + threadIdx.x;
			double2 dx[XP_UNROLL], dy[XP_UNROLL];
#pragma unroll
			for (int u=0 ; u<XP_UNROLL ; u++) { dx[u] = gdsp_ld2 (&p[u*XP_THREADS]);  dy[u] = gdsp_ld2 (&q[u*XP_THREADS]); }
#pragma unroll
			for (int u=0 ; u<XP_UNROLL ; u++)
				{
				const uint64_t j = j0 + 2 * ((uint64_t) u*XP_THREADS + threadIdx.x);
				take (0, dx[u].x, dy[u].x, sampled (j));
				take (1, dx[u].y, dy[u].y, sampled (j + 1));
				}
			}
		else
			{
			// the end of a frame, or a y of the other alignment: value by value.  Frame index 0 of a frame with a lead is
			// not a value of the pair (never sampled) and, for such a y, not an address to read: the index is clamped
			for (uint64_t j = j0 + threadIdx.x ; (j < m) && (j < j0 + XP_TILE) ; j += XP_THREADS)
				{
				const uint64_t jy = (j < lead)? lead : j;
				take (0, xb[jy], yb[jy], sampled (j));
				}
			}
		}

	// per sum: the lane's two expansions, then the wave's 64 as a tree (xsum_kernel)
	const int lane = threadIdx.x & 63;
#pragma unroll
	for (int s=0 ; s<NI ; s++)
		{
		unsigned long long* img = acc + s*XP_W;
#pragma unroll
		for (int k=0 ; k<XS_K ; k++) xs_grow (a[s][0], a[s][1][k], img);
		for (int off=1 ; off<64 ; off<<=1)
			{
			double t[XS_K];
#pragma unroll
			for (int k=0 ; k<XS_K ; k++) t[k] = __shfl_down (a[s][0][k], off, 64);
			const bool mine = (lane & (2*off - 1)) == 0;
#pragma unroll
			for (int k=0 ; k<XS_K ; k++) xs_grow (a[s][0], mine? t[k] : 0.0, img);
			}
		}
	uint64_t c = cnt;
	for (int off=32 ; off>0 ; off>>=1) c += __shfl_down (c, off, 64);
#pragma unroll
	for (int s=0 ; s<NI ; s++)
		{
		uint64_t f = infs[s];
		for (int off=32 ; off>0 ; off>>=1) f += __shfl_down (f, off, 64);
		if (lane == 0)
			{
			unsigned long long* img = acc + s*XP_W;
#pragma unroll
			for (int k=0 ; k<XS_K ; k++) xs_deposit (img, a[s][0][k]);
			if (c != 0) atomicAdd (&img[GDSP_XSUM_WORD_COUNT], (unsigned long long) c);
			if (f != 0) atomicAdd (&img[GDSP_XSUM_WORD_INF],   (unsigned long long) f);
			}
		}
	__syncthreads ();
	if (threadIdx.x < NI) xs_carry (acc + threadIdx.x*XP_W);   // canonical digits: the workgroups' images then add without overflow
	__syncthreads ();
	for (int i=threadIdx.x ; i<NI*XP_W ; i+=XP_THREADS) { if (acc[i] != 0) atomicAdd (&d_acc[i], acc[i]); }
	}

// the pairs as sources of their x: what the sample walk and gdsp_reduce_sources take
static std::vector<gdsp_xsum_source> xp_sources (const gdsp_xsum_pair* pairs, int npairs)
	{
	std::vector<gdsp_xsum_source> xs ((size_t) std::max (npairs, 0));
	for (int i=0 ; i<npairs ; i++)
		{ xs[i].d_v = pairs[i].d_x;  xs[i].n = pairs[i].n;  xs[i].first = pairs[i].first;  xs[i].device = pairs[i].device;  xs[i].stream = pairs[i].stream; }
	return xs;
	}

// xs: xp_sources (pairs, npairs)
static int xsum_pair_launch (int pass, const gdsp_xsum_pair* pairs, const gdsp_xsum_source* xs, int npairs, uint32_t window,
                             double lo, double hi, double ylo, double yhi, double meanx, double meany, uint64_t* d_acc, void* stream)
	{
	GDSP_REQUIRE (d_acc != NULL, "NULL accumulator");
	GDSP_REQUIRE ((npairs == 0) || (pairs != NULL), "NULL pairs");
	if (window == 0) window = 1;
	hipStream_t s = gdsp_stream (stream);
	int i = 0;
	while (i < npairs)
		{
		GdspSamplePair P;
		const int k = gdsp_sample_pair_next (P, pairs, xs, npairs, &i, window, XP_TILE, 0x7FFFFFFFull);
		GDSP_REQUIRE (k >= 0, "both vectors of a pair must be 8-byte aligned");
		if (k == 0) continue;
		const uint32_t tiles  = P.x.tile0[k];
		const uint32_t blocks = (tiles < XP_MAX_BLOCKS)? tiles : XP_MAX_BLOCKS;
		unsigned long long* acc = reinterpret_cast<unsigned long long*> (d_acc);
		const dim3 grid (blocks), block (XP_THREADS);
		if (pass == 1)
			{
			if (window == 1) hipLaunchKernelGGL ((xsum_pair_kernel<1, false>), grid, block, 0, s, P, window, lo, hi, ylo, yhi, meanx, meany, acc);
			else             hipLaunchKernelGGL ((xsum_pair_kernel<1, true>),  grid, block, 0, s, P, window, lo, hi, ylo, yhi, meanx, meany, acc);
			}
		else
			{
			if (window == 1) hipLaunchKernelGGL ((xsum_pair_kernel<2, false>), grid, block, 0, s, P, window, lo, hi, ylo, yhi, meanx, meany, acc);
			else             hipLaunchKernelGGL ((xsum_pair_kernel<2, true>),  grid, block, 0, s, P, window, lo, hi, ylo, yhi, meanx, meany, acc);
			}
		GDSP_LAUNCH_CHECK ();
		}
	return GDSP_OK;
	}

extern "C" {

uint32_t gdsp_xsum_pair_tile (void) { return XP_TILE; }

int gdsp_xsum_pair_accumulate_batch (const gdsp_xsum_pair* pairs, int npairs, uint32_t window, double lo, double hi,
                                     double ylo, double yhi, uint64_t* d_acc, void* stream)
	{
	GDSP_REQUIRE ((npairs == 0) || (pairs != NULL), "NULL pairs");
	return xsum_pair_launch (1, pairs, xp_sources (pairs, npairs).data (), npairs, window, lo, hi, ylo, yhi, 0.0, 0.0, d_acc, stream);
	}

int gdsp_xsum_pair_accumulate_dev_batch (const gdsp_xsum_pair* pairs, int npairs, uint32_t window, double lo, double hi,
                                         double ylo, double yhi, double meanx, double meany, uint64_t* d_acc, void* stream)
	{
	GDSP_REQUIRE ((fabs (meanx) <= DBL_MAX) && (fabs (meany) <= DBL_MAX), "the means must be finite");
	GDSP_REQUIRE ((npairs == 0) || (pairs != NULL), "NULL pairs");
	return xsum_pair_launch (2, pairs, xp_sources (pairs, npairs).data (), npairs, window, lo, hi, ylo, yhi, meanx, meany, d_acc, stream);
	}

} // extern "C"

// ------------------------------------------------------------------------------------------- end to end ----
static gdsp_comm* xpComm = NULL;                             // see gdsp_genome_correlation_use_comm
static uint64_t   xpLast[8];                                 // see gdsp_genome_correlation_last

// one pass over every pair, the devices' images (2 or 3, side by side) reduced into img (host words, global)
static int xp_genome_pass (int pass, const gdsp_xsum_pair* pairs, int npairs, const gdsp_xsum_source* xs, uint32_t window,
                           double lo, double hi, double ylo, double yhi, double meanx, double meany,
                           gdsp_reduce_fn reduce, void* reduceCtx, uint64_t* img)
	{
	const int images = (pass == 1)? 2 : 3;
	std::vector<gdsp_xsum_pair> mine;
	auto onDevice = [&] (const gdsp_xsum_source* its, int nits, uint64_t* d_acc, void* stream) -> int
		{
		// its: the x of this device's pairs.  gdsp_reduce_sources (gdsp_comm.hip) hands a device the sources whose
		// `device` is its own, in the caller's order; the pairs are picked by that rule, and checked against `its`
		mine.clear ();
		for (int i=0 ; (i<npairs) && (nits>0) ; i++) { if (pairs[i].device == its[0].device) mine.push_back (pairs[i]); }
		GDSP_REQUIRE ((int) mine.size () == nits, "the pairs of a device are not its sources");
		for (int i=0 ; i<nits ; i++) GDSP_REQUIRE (mine[i].d_x == its[i].d_v, "the pairs of a device are not its sources");
		int rc = GDSP_OK;
		for (int k=0 ; (k<images) && (rc == GDSP_OK) ; k++) rc = gdsp_xsum_init (d_acc + k*XP_W, stream);
		if (rc == GDSP_OK)
			rc = xsum_pair_launch (pass, mine.data (), its, nits, window, lo, hi, ylo, yhi, meanx, meany, d_acc, stream);
		for (int k=0 ; (k<images) && (rc == GDSP_OK) ; k++) rc = gdsp_xsum_fold (d_acc + k*XP_W, stream);
		return rc;
		};
	return gdsp_reduce_sources ("gdsp_genome_correlation", "accumulators", xpComm, xs, npairs, (size_t) images * XP_W,
	                            onDevice, reduce, reduceCtx, img);
	}

extern "C" {

int gdsp_genome_correlation_use_comm (gdsp_comm* comm) { xpComm = comm;  return GDSP_OK; }

void gdsp_genome_correlation_last (uint64_t out[8]) { memcpy (out, xpLast, sizeof(xpLast)); }

int gdsp_genome_correlation (const gdsp_xsum_pair* pairs, int npairs, uint32_t window, double lo, double hi,
                             double ylo, double yhi, gdsp_reduce_fn reduce, void* reduceCtx, double* out)
	{
	GDSP_REQUIRE (out != NULL, "NULL result");
	GDSP_REQUIRE ((npairs == 0) || (pairs != NULL), "NULL pairs");
	GDSP_REQUIRE (!((xpComm != NULL) && (reduce != NULL)), "a host reduction hook next to a communicator");
	const std::vector<gdsp_xsum_source> xs = xp_sources (pairs, npairs);
	uint64_t img[3 * XP_W];
	int rc = xp_genome_pass (1, pairs, npairs, xs.data (), window, lo, hi, ylo, yhi, 0.0, 0.0, reduce, reduceCtx, img);
	if (rc != GDSP_OK) return rc;
	const uint64_t n = img[GDSP_XSUM_WORD_COUNT];
	memset (xpLast, 0, sizeof(xpLast));
	xpLast[0] = n;  xpLast[1] = img[GDSP_XSUM_WORD_FLUSHES] + img[XP_W + GDSP_XSUM_WORD_FLUSHES];
	out[GDSP_CORR_COUNT] = (double) n;
	out[GDSP_CORR_SUMX]  = gdsp_xsum_round (img);
	out[GDSP_CORR_SUMY]  = gdsp_xsum_round (img + XP_W);
	for (int k=GDSP_CORR_MEANX ; k<GDSP_CORR_FIGURES ; k++) out[k] = NAN;
	if (n == 0) return GDSP_OK;
	const double meanx = out[GDSP_CORR_MEANX] = gdsp_xsum_div_round (img, n);
	const double meany = out[GDSP_CORR_MEANY] = gdsp_xsum_div_round (img + XP_W, n);
	rc = xp_genome_pass (2, pairs, npairs, xs.data (), window, lo, hi, ylo, yhi, meanx, meany, reduce, reduceCtx, img);
	if (rc != GDSP_OK) return rc;
	for (int k=0 ; k<3 ; k++) { xpLast[2] += img[k*XP_W + GDSP_XSUM_WORD_FLUSHES];  xpLast[3+k] = img[k*XP_W + GDSP_XSUM_WORD_INF]; }
	out[GDSP_CORR_VARX] = gdsp_xsum_div_round (img, n);                                       // (+inf when some qxx was not finite)
	out[GDSP_CORR_VARY] = gdsp_xsum_div_round (img + XP_W, n);
	out[GDSP_CORR_COV]  = (img[2*XP_W + GDSP_XSUM_WORD_INF] != 0)? NAN : gdsp_xsum_div_round (img + 2*XP_W, n);
	gdsp_corr_derive (out);
	return GDSP_OK;
	}

} // extern "C"
