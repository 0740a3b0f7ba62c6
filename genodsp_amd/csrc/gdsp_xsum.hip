// gdsp_xsum.hip -- genome-wide stats (`stats`, `normalize`; not in the reference): the exact sum of the sampled genome
// and the exact sum of the squared deviations from its mean, each rounded once, on the host, at the end.
//
// The accumulator is an integer image of GDSP_XSUM_WORDS u64 words (include/genodsp_hip.h): digit k holds a signed
// multiple of 2^(32k-1074), so every finite double is a sum of three digits and the image spans 2^-1074 .. 2^1102.
// Integer words add associatively: the image of a genome is the same whatever the order, the cut into vectors, stretches,
// devices or ranks, the grid or the dispatch order -- the u64 SUM of the images is the image of the union.
//
// The pass (xsum_kernel): one read of the signal over every vector of a table of up to 32 (the batch convention of
// gdsp_common.h; 16-byte loads of 32 KiB tiles, a grid of at most XS_MAX_BLOCKS workgroups walking the tiles).  Each lane
// keeps two floating-point expansions of XS_K terms in registers, grown with TwoSum (ExBLAS): a summand enters term 0,
// the rounding error term 1, and so on.  Only a residual that is still non-zero after the last term -- or a summand whose
// TwoSum would overflow -- is deposited into the workgroup's image in LDS (ds_add_u64).  On read depth and on N(0,10^2)
// values that almost never happens (GDSP_XSUM_WORD_FLUSHES counts it); adversarial data stays exact and gets slower.
// At the end the lanes' expansions are added up a tree per wave (a lane takes the terms of the lane `off` above it:
// each term is added once), lane 0 deposits its terms, one lane carries the LDS image into canonical digits and the
// workgroup adds its non-zero words to the device image with integer atomics -- the fold of the workgroups' images, in
// no particular order because integer addition has none.  gdsp_xsum_fold canonicalises the device image (a second, tiny
// launch), so that images can be compared word for word and all-reduced with room to spare.
//
// Pass 2 is the same kernel with q = fl(fl(v - mean)^2) as the summand (__dsub_rn / __dmul_rn: never contracted); a q
// of +inf is counted in GDSP_XSUM_WORD_INF instead of being added.  Rounding (gdsp_xsum_round, gdsp_xsum_div_round) is
// host code that needs no GPU.

#include <float.h>
#include <math.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "gdsp_common.h"
#include "gdsp_xsum_dev.h"                              // xs_split, xs_deposit, xs_grow: shared with gdsp_intervalstats.hip
#include "gdsp_sample.h"                                // the table of sources and which of their values are sampled

#define XS_THREADS    256
#define XS_UNROLL     8                               // 16-byte loads in flight per lane
#define XS_TILE       (XS_THREADS * XS_UNROLL * 2)    // 4096 values = 32 KiB
#define XS_MAX_BLOCKS (256 * 4)                 // every workgroup resident (5 fit on a CU): equal shares finish together
#define XS_D          GDSP_XSUM_DIGITS

static_assert (GDSP_XSUM_WORDS == 72 && XS_D == 68, "the layout below");

// PASS 1 adds v, PASS 2 adds fl(fl(v - mean)^2); WINDOWED: the window is above 1
template <int PASS, bool WINDOWED>
__global__ __launch_bounds__(XS_THREADS)
void xsum_kernel (GdspSample B, uint32_t window, double lo, double hi, double mean, unsigned long long* __restrict__ d_acc)
	{
	__shared__ unsigned long long acc[GDSP_XSUM_WORDS];
	for (int i=threadIdx.x ; i<GDSP_XSUM_WORDS ; i+=XS_THREADS) acc[i] = 0;
	__syncthreads ();

	double   ax[XS_K], ay[XS_K];
#pragma unroll
	for (int k=0 ; k<XS_K ; k++) { ax[k] = 0.0;  ay[k] = 0.0; }
	uint32_t cnt = 0, infs = 0;
	auto take = [&] (double (&a)[XS_K], double x, bool sampled)
		{
		const bool in = sampled && !(x < lo) && !(x > hi) && xs_finite (x);   // percentile's tests; NaN and +-inf never
		double t = x;
		if (PASS == 2) { const double d = __dsub_rn (x, mean);  t = __dmul_rn (d, d); }
		const bool big = (PASS == 2) && in && !xs_finite (t);                  // q = +inf
		cnt  += in;
		infs += big;
		xs_grow (a, (in && !big)? t : 0.0, acc);
		};

	const uint32_t T = B.tile0[B.nvec];
	uint32_t v = 0;
	for (uint32_t g=blockIdx.x ; g<T ; g+=gridDim.x)
		{
		const GdspSampleTile t = gdsp_sample_tile<XS_TILE> (B, g, v);
		v = t.v;
		const double*  base = t.base;
		const uint64_t m = t.m, j0 = t.j0;
		auto sampled = [&] (uint64_t j) -> bool { return gdsp_sampled<WINDOWED> (t, window, j); };
		if (j0 + XS_TILE <= m)
			{
			const double2* p = reinterpret_cast<const double2*> (base + j0) + threadIdx.x;
			double2 d[XS_UNROLL];
#pragma unroll
			for (int u=0 ; u<XS_UNROLL ; u++) d[u] = gdsp_ld2 (&p[u*XS_THREADS]);
#pragma unroll
			for (int u=0 ; u<XS_UNROLL ; u++)
				{
				const uint64_t j = j0 + 2 * ((uint64_t) u*XS_THREADS + threadIdx.x);
				take (ax, d[u].x, sampled (j));
				take (ay, d[u].y, sampled (j + 1));
				}
			}
		else
			{
			for (uint64_t j = j0 + threadIdx.x ; j < m ; j += XS_THREADS) take (ax, base[j], sampled (j));
			}
		}

	// the lane's two expansions, then the wave's 64 as a tree: lane l takes lane l+off's terms when l % 2off == 0
#pragma unroll
	for (int k=0 ; k<XS_K ; k++) xs_grow (ax, ay[k], acc);
	const int lane = threadIdx.x & 63;
	for (int off=1 ; off<64 ; off<<=1)
		{
		double t[XS_K];
#pragma unroll
		for (int k=0 ; k<XS_K ; k++) t[k] = __shfl_down (ax[k], off, 64);
		const bool mine = (lane & (2*off - 1)) == 0;
#pragma unroll
		for (int k=0 ; k<XS_K ; k++) xs_grow (ax, mine? t[k] : 0.0, acc);
		}
	uint64_t c = cnt, f = infs;
	for (int off=32 ; off>0 ; off>>=1) { c += __shfl_down (c, off, 64);  f += __shfl_down (f, off, 64); }
	if (lane == 0)
		{
#pragma unroll
		for (int k=0 ; k<XS_K ; k++) xs_deposit (acc, ax[k]);
		if (c != 0) atomicAdd (&acc[GDSP_XSUM_WORD_COUNT], (unsigned long long) c);
		if (f != 0) atomicAdd (&acc[GDSP_XSUM_WORD_INF],   (unsigned long long) f);
		}
	__syncthreads ();
	if (threadIdx.x == 0) xs_carry (acc);                    // canonical digits: the workgroups' images then add without overflow
	__syncthreads ();
	if ((threadIdx.x < GDSP_XSUM_WORDS) && (acc[threadIdx.x] != 0)) atomicAdd (&d_acc[threadIdx.x], acc[threadIdx.x]);
	}

// the device image in canonical digits (one lane: 68 steps)
__global__ void xsum_fold_kernel (unsigned long long* d_acc)
	{
	if (threadIdx.x != 0) return;
	xs_carry (d_acc);
	}

static int xsum_launch (int pass, const gdsp_xsum_source* sources, int nsources, uint32_t window, double lo, double hi,
                        double mean, uint64_t* d_acc, void* stream)
	{
	GDSP_REQUIRE (d_acc != NULL, "NULL accumulator");
	GDSP_REQUIRE ((nsources == 0) || (sources != NULL), "NULL sources");
	if (window == 0) window = 1;
	hipStream_t s = gdsp_stream (stream);
	int i = 0;
	while (i < nsources)
		{
		GdspSample B;
		const int k = gdsp_sample_next (B, sources, nsources, &i, window, XS_TILE, 0x7FFFFFFFull);
		GDSP_REQUIRE (k >= 0, "a source must be 8-byte aligned");
		if (k == 0) continue;
		const uint32_t tiles  = B.tile0[k];
		const uint32_t blocks = (tiles < XS_MAX_BLOCKS)? tiles : XS_MAX_BLOCKS;
		unsigned long long* acc = reinterpret_cast<unsigned long long*> (d_acc);
		if (pass == 1)
			{
			if (window == 1) hipLaunchKernelGGL ((xsum_kernel<1, false>), dim3(blocks), dim3(XS_THREADS), 0, s, B, window, lo, hi, mean, acc);
			else             hipLaunchKernelGGL ((xsum_kernel<1, true>),  dim3(blocks), dim3(XS_THREADS), 0, s, B, window, lo, hi, mean, acc);
			}
		else
			{
			if (window == 1) hipLaunchKernelGGL ((xsum_kernel<2, false>), dim3(blocks), dim3(XS_THREADS), 0, s, B, window, lo, hi, mean, acc);
			else             hipLaunchKernelGGL ((xsum_kernel<2, true>),  dim3(blocks), dim3(XS_THREADS), 0, s, B, window, lo, hi, mean, acc);
			}
		GDSP_LAUNCH_CHECK ();
		}
	return GDSP_OK;
	}

// ------------------------------------------------------------------------------------------ host rounding ----
// the image's value as a sign and a magnitude in 32-bit limbs (least significant first), weight of limb 0: 2^-1074
static void xs_magnitude (const uint64_t* img, std::vector<uint32_t>& mag, bool& neg)
	{
	mag.assign (XS_D + 3, 0);
	__int128 carry = 0;
	for (int w=0 ; w<XS_D ; w++)
		{
		const __int128 x = (__int128) (int64_t) img[w] + carry;
		mag[w] = (uint32_t) (x & 0xFFFFFFFF);
		carry  = x >> 32;                                   // (arithmetic: floor division)
		}
	for (int w=XS_D ; w<XS_D+3 ; w++) { mag[w] = (uint32_t) (carry & 0xFFFFFFFF);  carry >>= 32; }
	neg = (mag[XS_D+2] >> 31) != 0;                         // two's complement over the limbs
	if (neg)
		{
		uint64_t c = 1;
		for (auto& l : mag) { const uint64_t x = (uint64_t) (uint32_t) ~l + c;  l = (uint32_t) x;  c = x >> 32; }
		}
	}

static inline bool xs_bit (const std::vector<uint32_t>& L, int64_t i)
	{ return (i >= 0) && ((size_t) (i >> 5) < L.size ()) && ((L[i >> 5] >> (i & 31)) & 1); }

// (-1)^neg * (L + something in (0,1) when sticky) * 2^scale, rounded once to nearest, ties to even
double xs_round_limbs (const std::vector<uint32_t>& L, bool sticky, int scale, bool neg)      // (gdsp_xsum_dev.h)
	{
	int64_t h = -1;
	for (int64_t w=(int64_t) L.size ()-1 ; (w>=0) && (h<0) ; w--)
		{ if (L[w] != 0) h = w*32 + 31 - __builtin_clz (L[w]); }
	if (h < 0) return 0.0;                                  // (an exact zero: +0.0)
	const int64_t lsb = std::max<int64_t> (h - 52 + scale, -1074);   // weight of the result's last bit
	const int64_t s   = lsb - scale;                        // bits of L below it
	uint64_t mant = 0;
	for (int64_t i=h ; i>=std::max<int64_t> (s, 0) ; i--) mant = (mant << 1) | (xs_bit (L, i)? 1 : 0);
	if (s <= 0) { const double r = ldexp ((double) mant, (int) (scale + std::max<int64_t> (s, 0)));  return neg? -r : r; }   // exact
	const bool half = xs_bit (L, s - 1);
	for (int64_t i=0 ; (i<s-1) && !sticky ; i++) sticky = xs_bit (L, i);
	if (half && (sticky || (mant & 1))) mant++;             // (mant may reach 2^53: still exact as a double)
	const double r = ldexp ((double) mant, (int) lsb);       // exact, or +-inf beyond DBL_MAX
	return neg? -r : r;
	}

extern "C" {

int gdsp_xsum_init (uint64_t* d_acc, void* stream)
	{
	GDSP_REQUIRE (d_acc != NULL, "NULL accumulator");
	GDSP_HIP_TRY (hipMemsetAsync (d_acc, 0, GDSP_XSUM_WORDS * sizeof(uint64_t), gdsp_stream (stream)));
	return GDSP_OK;
	}

int gdsp_xsum_accumulate_batch (const gdsp_xsum_source* sources, int nsources, uint32_t window, double lo, double hi,
                                uint64_t* d_acc, void* stream)
	{ return xsum_launch (1, sources, nsources, window, lo, hi, 0.0, d_acc, stream); }

int gdsp_xsum_accumulate_sq_batch (const gdsp_xsum_source* sources, int nsources, uint32_t window, double lo, double hi,
                                   double mean, uint64_t* d_acc, void* stream)
	{
	GDSP_REQUIRE (fabs (mean) <= DBL_MAX, "the mean must be finite");
	return xsum_launch (2, sources, nsources, window, lo, hi, mean, d_acc, stream);
	}

int gdsp_xsum_fold (uint64_t* d_acc, void* stream)
	{
	GDSP_REQUIRE (d_acc != NULL, "NULL accumulator");
	hipLaunchKernelGGL (xsum_fold_kernel, dim3(1), dim3(64), 0, gdsp_stream (stream), reinterpret_cast<unsigned long long*> (d_acc));
	GDSP_LAUNCH_CHECK ();
	return GDSP_OK;
	}

void gdsp_xsum_add_host (uint64_t* h_acc, double x)
	{
	if (!(fabs (x) <= DBL_MAX)) return;
	uint32_t w;  uint64_t c0, c1, c2;
	xs_split (x, w, c0, c1, c2);
	h_acc[w] += c0;  h_acc[w + 1] += c1;  h_acc[w + 2] += c2;
	h_acc[GDSP_XSUM_WORD_COUNT]++;
	}

double gdsp_xsum_round (const uint64_t* h_acc)
	{
	if (h_acc[GDSP_XSUM_WORD_INF] != 0) return HUGE_VAL;
	std::vector<uint32_t> mag;
	bool neg;
	xs_magnitude (h_acc, mag, neg);
	return xs_round_limbs (mag, false, -1074, neg);
	}

double gdsp_xsum_div_round (const uint64_t* h_acc, uint64_t n)
	{
	if (n == 0) return NAN;
	if (h_acc[GDSP_XSUM_WORD_INF] != 0) return HUGE_VAL;
	std::vector<uint32_t> mag;
	bool neg;
	xs_magnitude (h_acc, mag, neg);
	// long division of mag * 2^128 by n, limb by limb from the top: the quotient has at least 64 bits more than the
	// result keeps, and the remainder only says whether anything is left (sticky)
	std::vector<uint32_t> num (4, 0);
	num.insert (num.end (), mag.begin (), mag.end ());
	std::vector<uint32_t> q (num.size (), 0);
	unsigned __int128 r = 0;
	for (int64_t w=(int64_t) num.size ()-1 ; w>=0 ; w--)
		{
		const unsigned __int128 x = (r << 32) | num[w];
		q[w] = (uint32_t) (x / n);
		r    = x % n;
		}
	return xs_round_limbs (q, r != 0, -1074 - 128, neg);
	}

} // extern "C"

// ------------------------------------------------------------------------------------------- end to end ----
static gdsp_comm* xsComm = NULL;                             // see gdsp_genome_stats_use_comm
static uint64_t   xsLast[4];                                 // see gdsp_genome_stats_last

// one pass over every source, the devices' images reduced into img (host words, global)
static int xs_genome_pass (int pass, const gdsp_xsum_source* sources, int nsources, uint32_t window, double lo, double hi,
                           double mean, gdsp_reduce_fn reduce, void* reduceCtx, uint64_t* img)
	{
	auto onDevice = [&] (const gdsp_xsum_source* mine, int nmine, uint64_t* d_acc, void* stream) -> int
		{
		int rc = gdsp_xsum_init (d_acc, stream);
		if (rc == GDSP_OK) rc = (pass == 1)? gdsp_xsum_accumulate_batch (mine, nmine, window, lo, hi, d_acc, stream)
		                                   : gdsp_xsum_accumulate_sq_batch (mine, nmine, window, lo, hi, mean, d_acc, stream);
		if (rc == GDSP_OK) rc = gdsp_xsum_fold (d_acc, stream);
		return rc;
		};
	return gdsp_reduce_sources ("gdsp_genome_stats", "accumulator", xsComm, sources, nsources, GDSP_XSUM_WORDS, onDevice,
	                            reduce, reduceCtx, img);
	}

extern "C" {

int gdsp_genome_stats_use_comm (gdsp_comm* comm) { xsComm = comm;  return GDSP_OK; }

void gdsp_genome_stats_last (uint64_t out[4]) { memcpy (out, xsLast, sizeof(xsLast)); }

int gdsp_genome_stats (const gdsp_xsum_source* sources, int nsources, uint32_t window, double lo, double hi,
                       gdsp_reduce_fn reduce, void* reduceCtx, double* out)
	{
	GDSP_REQUIRE (out != NULL, "NULL result");
	GDSP_REQUIRE ((nsources == 0) || (sources != NULL), "NULL sources");
	GDSP_REQUIRE (!((xsComm != NULL) && (reduce != NULL)), "a host reduction hook next to a communicator");
	uint64_t img[GDSP_XSUM_WORDS];
	int rc = xs_genome_pass (1, sources, nsources, window, lo, hi, 0.0, reduce, reduceCtx, img);
	if (rc != GDSP_OK) return rc;
	const uint64_t n = img[GDSP_XSUM_WORD_COUNT];
	xsLast[0] = n;  xsLast[1] = img[GDSP_XSUM_WORD_FLUSHES];  xsLast[2] = 0;  xsLast[3] = 0;
	out[0] = (double) n;
	out[1] = gdsp_xsum_round (img);
	if (n == 0) { out[2] = out[3] = out[4] = NAN;  return GDSP_OK; }
	out[2] = gdsp_xsum_div_round (img, n);
	rc = xs_genome_pass (2, sources, nsources, window, lo, hi, out[2], reduce, reduceCtx, img);
	if (rc != GDSP_OK) return rc;
	xsLast[2] = img[GDSP_XSUM_WORD_FLUSHES];  xsLast[3] = img[GDSP_XSUM_WORD_INF];
	out[3] = gdsp_xsum_div_round (img, n);
	out[4] = sqrt (out[3]);
	return GDSP_OK;
	}

} // extern "C"
