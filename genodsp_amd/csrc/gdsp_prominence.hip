// gdsp_prominence.hip -- prominence: how far every base stands above its surroundings, inside a window.
//
// Not an operator of the reference.  Definition (include/genodsp_hip.h): for base i with x = v[i] the left walk goes
// over j = i-1, i-2, ... while j >= max(0, i-wL) and not v[j] > x, mL the smallest value it meets (x to begin with);
// the right walk likewise up to min(n-1, i+wR); base = the larger of mL and mR, prominence = x - base (+0.0 where
// x == base).  wL = (W-1)/2, wR = W-1-wL: bestmax's centring.  Only comparisons and one subtraction: bit exact.
//
// One workgroup owns T outputs and stages the PR_NS inputs they read (HL + T + HR, the two reaches rounded up to even
// so that every tile starts on a 16-byte boundary of the vector).  Per tile:
//   1. (max, min) summaries of every aligned block of 8, 64 and 512 staged positions: a wave covers 64 positions, three
//      exchange steps give the blocks of 8 and three more the block of 64; twelve threads fold those into the blocks of
//      512.  Positions outside the vector are staged as 0.0; a summary is only ever used for a block that lies wholly
//      inside a base's window, and a window never leaves the vector, so what the padding holds decides nothing.
//   2. a base whose left or right walk is empty (window of 1, chromosome end), or which has a strictly greater
//      neighbour, is finished: prominence 0, base x.  The others (candidates; about one base in twenty of a smoothed
//      signal, every base of an all-zero one) are compacted into a list, one ballot and one LDS counter add per wave.
//   3. one lane per candidate walks outwards: single values up to a multiple of 8, blocks of 8 up to a multiple of 64,
//      blocks of 64 up to a multiple of 512, blocks of 512, and down again through 64, 8 and single values as the
//      window's end comes near.  A block whose max is not above x gives its min and is skipped whole; a block whose max
//      is above x is entered at the next smaller size.  That is at most 7 steps per level and direction plus
//      wL/512 -- under 50 LDS reads per side whatever the data (an all-zero genome: every base is a candidate and every
//      walk covers its whole window).  The results wait in registers until every walk has read the inputs,
//   4. then replace the candidates' values in the staged copy, and
//   5. the tile leaves as 16-byte non-temporal stores (prominence: 0.0 at the bases that were no candidates).
//
// LDS: 48 KiB of values, 12 KiB of candidate indices, 13.7 KiB of summaries, 0.75 KiB of candidate masks: 74.4 KiB, two
// 1024-thread workgroups per CU.

#include "gdsp_common.h"

#define PR_NS      6144                                                   // staged positions per tile
#define PR_THREADS 1024                                                   // six positions per thread; a wave covers a block of 64
#define PR_PER     (PR_NS / PR_THREADS)
static_assert (PR_THREADS % 64 == 0, "a wave must cover whole blocks");
static_assert (PR_NS % (2 * PR_THREADS) == 0, "every thread stages the same number of 16-byte words");
static_assert (PR_NS % 512 == 0, "whole blocks of 512");
static_assert (PR_NS / 512 <= PR_THREADS, "one thread per block of 512");
static_assert (2 * ((GDSP_PROMINENCE_MAX_WINDOW + 1) / 2 + 1) < PR_NS, "the largest window must leave outputs in a tile");

struct PrLds
	{
	double   v[PR_NS];                                                    // staged inputs; the candidates' results in the end
	double2  s8[PR_NS/8], s64[PR_NS/64], s512[PR_NS/512];                 // (max, min) of every aligned block
	uint64_t cand[PR_NS/64];                                              // which positions of the block of 64 are candidates
	uint16_t list[PR_NS];                                                 // the candidates' positions, in no particular order
	uint32_t count;
	};
static_assert (sizeof (PrLds) <= 80 * 1024, "two workgroups per CU");

// host and device: the reaches rounded up to even, and the outputs per tile
__host__ __device__ __forceinline__ uint32_t pr_even (uint32_t w) { return (w + 1) & ~1u; }
__host__ __device__ __forceinline__ uint32_t pr_tile (uint32_t wL, uint32_t wR) { return PR_NS - pr_even (wL) - pr_even (wR); }

// one step over a block: false when the block holds a value above x (the walk enters it at the next smaller size)
__device__ __forceinline__ bool pr_take (const double2 s, double x, double& m)
	{
	if (s.x > x) return false;
	if (s.y < m) m = s.y;
	return true;
	}

// the left walk from position p down to lo (lo <= p): the smallest value met, x to begin with.  t: positions [t, p)
// have been walked; cap: the largest block size still worth trying (3: 512, 2: 64, 1: 8, 0: single values)
__device__ __forceinline__ double pr_walk_left (const PrLds& S, int p, int lo, double x)
	{
	double m = x;
	int t = p, cap = 3;
	while ((t > lo) && (t & 7)) { const double y = S.v[--t];  if (y > x) return m;  if (y < m) m = y; }
	if (cap >= 1) while ((t - 8   >= lo) && (t & 63))  { if (!pr_take (S.s8  [(t >> 3) - 1], x, m)) { cap = 0;  break; }  t -= 8; }
	if (cap >= 2) while ((t - 64  >= lo) && (t & 511)) { if (!pr_take (S.s64 [(t >> 6) - 1], x, m)) { cap = 1;  break; }  t -= 64; }
	if (cap >= 3) while ( t - 512 >= lo)               { if (!pr_take (S.s512[(t >> 9) - 1], x, m)) { cap = 2;  break; }  t -= 512; }
	if (cap >= 2) while ( t - 64  >= lo)               { if (!pr_take (S.s64 [(t >> 6) - 1], x, m)) { cap = 1;  break; }  t -= 64; }
	if (cap >= 1) while ( t - 8   >= lo)               { if (!pr_take (S.s8  [(t >> 3) - 1], x, m)) {           break; }  t -= 8; }
	while (t > lo) { const double y = S.v[--t];  if (y > x) return m;  if (y < m) m = y; }
	return m;
	}

// the right walk from position p up to hi (p <= hi).  t: positions (p, t) have been walked; e: one past the last position
__device__ __forceinline__ double pr_walk_right (const PrLds& S, int p, int hi, double x)
	{
	double m = x;
	const int e = hi + 1;
	int t = p + 1, cap = 3;
	while ((t < e) && (t & 7)) { const double y = S.v[t++];  if (y > x) return m;  if (y < m) m = y; }
	if (cap >= 1) while ((t + 8   <= e) && (t & 63))  { if (!pr_take (S.s8  [t >> 3], x, m)) { cap = 0;  break; }  t += 8; }
	if (cap >= 2) while ((t + 64  <= e) && (t & 511)) { if (!pr_take (S.s64 [t >> 6], x, m)) { cap = 1;  break; }  t += 64; }
	if (cap >= 3) while ( t + 512 <= e)               { if (!pr_take (S.s512[t >> 9], x, m)) { cap = 2;  break; }  t += 512; }
	if (cap >= 2) while ( t + 64  <= e)               { if (!pr_take (S.s64 [t >> 6], x, m)) { cap = 1;  break; }  t += 64; }
	if (cap >= 1) while ( t + 8   <= e)               { if (!pr_take (S.s8  [t >> 3], x, m)) {           break; }  t += 8; }
	while (t < e) { const double y = S.v[t++];  if (y > x) return m;  if (y < m) m = y; }
	return m;
	}

__device__ __forceinline__
void prominence_tile (const double* __restrict__ in, double* __restrict__ out, uint32_t n, uint32_t tile,
                      uint32_t wL, uint32_t wR, int what)
	{
	__shared__ __attribute__((aligned(16))) PrLds S;
	const int     tid  = threadIdx.x;
	const int     lane = tid & 63;
	const int     HL   = (int) pr_even (wL);
	const int     T    = (int) pr_tile (wL, wR);
	const int64_t o0   = (int64_t) tile * T;                              // first output of the tile (even)
	const int64_t g0   = o0 - HL;                                         // first staged base (even; negative in tile 0)

	// ---- stage
	if (tid == 0) S.count = 0;
	if ((g0 >= 0) && (g0 + PR_NS <= (int64_t) n))
		{
		const double2* src = reinterpret_cast<const double2*> (in + g0);
		double2*       dst = reinterpret_cast<double2*> (S.v);
		double2 r[PR_PER/2];
#pragma unroll
		for (int u=0 ; u<PR_PER/2 ; u++) r[u] = gdsp_ld2 (&src[u*PR_THREADS + tid]);    // all loads in flight
#pragma unroll
		for (int u=0 ; u<PR_PER/2 ; u++) dst[u*PR_THREADS + tid] = r[u];
		}
	else
		{
		for (int p=tid ; p<PR_NS ; p+=PR_THREADS)
			{
			const int64_t g = g0 + p;
			S.v[p] = ((g >= 0) && (g < (int64_t) n))? in[g] : 0.0;
			}
		}
	__syncthreads ();

	const int     pFirst = (g0 < 0)? (int) -g0 : 0;                       // base 0 of the vector
	const int64_t lastG  = (int64_t) n - 1 - g0;
	const int     pLast  = (lastG < PR_NS - 1)? (int) lastG : PR_NS - 1;  // base n-1 of the vector, or the tile's last position

	// ---- 1, 2. block summaries; the candidates among the outputs
#pragma unroll
	for (int u=0 ; u<PR_PER ; u++)
		{
		const int    j = u*PR_THREADS + tid;
		const double x = S.v[j];
		// (the neighbours: clamped at the two ends of the staged copy, and padding where the vector ends.  Neither decides
		//  anything: position 0 or PR_NS-1 is an output only when wL or wR is 0, and a base at an end of the vector has an
		//  empty walk -- both are finished below before l and r are looked at)
		const double l = S.v[(j > 0)? j-1 : 0];
		const double r = S.v[(j < PR_NS-1)? j+1 : PR_NS-1];
		double mx = x, mn = x;
#pragma unroll
		for (int d=1 ; d<8 ; d<<=1)
			{
			const double ox = __shfl_xor (mx, d, 64), on = __shfl_xor (mn, d, 64);
			if (ox > mx) mx = ox;
			if (on < mn) mn = on;
			}
		if ((lane & 7) == 0) S.s8[j >> 3] = make_double2 (mx, mn);
#pragma unroll
		for (int d=8 ; d<64 ; d<<=1)
			{
			const double ox = __shfl_xor (mx, d, 64), on = __shfl_xor (mn, d, 64);
			if (ox > mx) mx = ox;
			if (on < mn) mn = on;
			}
		const bool isOut = (j >= HL) && (j < HL + T) && (j <= pLast);
		const bool c     = isOut && (wL >= 1) && (wR >= 1) && (j > pFirst) && (j < pLast) && !(l > x) && !(r > x);
		const uint64_t mask = __ballot (c);
		uint32_t first = 0;
		if (lane == 0)
			{
			S.s64[j >> 6] = make_double2 (mx, mn);  S.cand[j >> 6] = mask;
			if (mask != 0) first = atomicAdd (&S.count, (uint32_t) __popcll (mask));
			}
		first = __shfl (first, 0, 64);
		if (c) S.list[first + (uint32_t) __popcll (mask & ((((uint64_t) 1) << lane) - 1))] = (uint16_t) j;
		}
	__syncthreads ();
	if (tid < PR_NS/512)
		{
		double2 s = S.s64[8*tid];
#pragma unroll
		for (int k=1 ; k<8 ; k++)
			{
			const double2 o = S.s64[8*tid + k];
			if (o.x > s.x) s.x = o.x;
			if (o.y < s.y) s.y = o.y;
			}
		S.s512[tid] = s;
		}
	__syncthreads ();

	// ---- 3. the walks (count <= T <= PR_PER * PR_THREADS)
	const uint32_t count = S.count;
	double res[PR_PER];
#pragma unroll
	for (int k=0 ; k<PR_PER ; k++)
		{
		const uint32_t c = (uint32_t) (k*PR_THREADS + tid);
		res[k] = 0.0;
		if (c >= count) continue;
		const int    p  = S.list[c];
		const double x  = S.v[p];
		const int    lo = (p - (int) wL > pFirst)? p - (int) wL : pFirst;
		const int    hi = (p + (int) wR < pLast)?  p + (int) wR : pLast;
		const double mL = pr_walk_left  (S, p, lo, x);
		const double mR = pr_walk_right (S, p, hi, x);
		const double base = (mL >= mR)? mL : mR;
		res[k] = (what == GDSP_PROMINENCE_BASE)? base : ((x == base)? 0.0 : x - base);
		}
	__syncthreads ();                                                     // every walk has read the inputs

	// ---- 4. the candidates' results take their inputs' places
#pragma unroll
	for (int k=0 ; k<PR_PER ; k++)
		{
		const uint32_t c = (uint32_t) (k*PR_THREADS + tid);
		if (c < count) S.v[S.list[c]] = res[k];
		}
	__syncthreads ();

	// ---- 5. the outputs, two per lane (HL, T and o0 are even)
	const bool zeroOthers = (what != GDSP_PROMINENCE_BASE);
#pragma unroll
	for (int u=0 ; u<PR_PER/2 ; u++)
		{
		const int q = u*PR_THREADS + tid;
		if (2*q >= T) continue;
		const int64_t g = o0 + 2*q;
		if (g >= (int64_t) n) continue;
		const int p = HL + 2*q;
		double2 y = *reinterpret_cast<const double2*> (&S.v[p]);
		if (zeroOthers)
			{
			const uint32_t bits = (uint32_t) (S.cand[p >> 6] >> (p & 63));          // (p is even: p and p+1 share a block)
			if (!(bits & 1)) y.x = 0.0;
			if (!(bits & 2)) y.y = 0.0;
			}
		if (g + 1 < (int64_t) n) gdsp_st2 (reinterpret_cast<double2*> (out + g), y);
		else                     out[g] = y.x;
		}
	}

__global__ __launch_bounds__(PR_THREADS) __attribute__((amdgpu_waves_per_eu (8)))    // (<= 64 VGPRs: two tiles per CU)
void prominence_kernel (const double* __restrict__ in, double* __restrict__ out, uint32_t n, uint32_t ntiles,
                        uint32_t wL, uint32_t wR, int what)
	{ prominence_tile (in, out, n, gdsp_xcd_tile (blockIdx.x, ntiles), wL, wR, what); }

__global__ __launch_bounds__(PR_THREADS) __attribute__((amdgpu_waves_per_eu (8)))    // one grid over every vector of the table (gdsp_common.h)
void prominence_batch_kernel (GdspBatch B, uint32_t wL, uint32_t wR, int what)
	{
	const double* in;  double* out;  uint32_t n;
	const uint32_t tile = gdsp_batch_tile (B, in, out, n);
	prominence_tile (in, out, n, tile, wL, wR, what);
	}

static int prominence_run (const gdsp_batch_item* items, int nitems, uint32_t W, int what, void* stream)
	{
	const uint32_t wL = (W - 1) / 2, wR = (W - 1) - wL;
	const uint64_t T  = pr_tile (wL, wR);
	hipStream_t s = gdsp_stream (stream);
	if (nitems == 1)
		{
		if (items[0].n == 0) return GDSP_OK;
		const uint32_t ntiles = (uint32_t) (((uint64_t) items[0].n + T - 1) / T);
		hipLaunchKernelGGL (prominence_kernel, dim3(ntiles), dim3(PR_THREADS), 0, s,
		                    items[0].d_in, items[0].d_out, items[0].n, ntiles, wL, wR, what);
		}
	else
		gdsp_batch_run (items, nitems, [=] (uint32_t n) { return ((uint64_t) n + T - 1) / T; },
			[&] (const GdspBatch& B, uint32_t tiles)
				{
				hipLaunchKernelGGL (prominence_batch_kernel, dim3(tiles), dim3(PR_THREADS), 0, s, B, wL, wR, what);
				});
	GDSP_LAUNCH_CHECK ();
	return GDSP_OK;
	}

extern "C" {

uint32_t gdsp_prominence_tile (uint32_t W)
	{
	if ((W < 1) || (W > GDSP_PROMINENCE_MAX_WINDOW)) return 0;
	const uint32_t wL = (W - 1) / 2;
	return pr_tile (wL, (W - 1) - wL);
	}

int gdsp_prominence (const double* d_in, double* d_out, uint32_t n, uint32_t W, int what, void* stream)
	{
	GDSP_REQUIRE (W >= 1, "window must be >= 1");
	GDSP_REQUIRE (W <= GDSP_PROMINENCE_MAX_WINDOW, "window above GDSP_PROMINENCE_MAX_WINDOW");
	GDSP_REQUIRE ((what == GDSP_PROMINENCE_VALUE) || (what == GDSP_PROMINENCE_BASE), "what must be GDSP_PROMINENCE_VALUE or GDSP_PROMINENCE_BASE");
	GDSP_REQUIRE ((n == 0) || (d_in != d_out), "out-of-place operator: d_out must not alias d_in");
	if (n == 0) return GDSP_OK;
	GDSP_REQUIRE ((d_in != NULL) && (d_out != NULL), "NULL vector");
	GDSP_REQUIRE (gdsp_aligned16 (d_in) && gdsp_aligned16 (d_out), "vectors must be 16-byte aligned");
	gdsp_batch_item item = { d_in, d_out, n };
	return prominence_run (&item, 1, W, what, stream);
	}

int gdsp_prominence_batch (const gdsp_batch_item* items, int nitems, uint32_t W, int what, void* stream)
	{
	GDSP_REQUIRE (W >= 1, "window must be >= 1");
	GDSP_REQUIRE (W <= GDSP_PROMINENCE_MAX_WINDOW, "window above GDSP_PROMINENCE_MAX_WINDOW");
	GDSP_REQUIRE ((what == GDSP_PROMINENCE_VALUE) || (what == GDSP_PROMINENCE_BASE), "what must be GDSP_PROMINENCE_VALUE or GDSP_PROMINENCE_BASE");
	int rc = gdsp_batch_check (items, nitems, false);
	if (rc != GDSP_OK) return rc;
	if (nitems == 0) return GDSP_OK;
	return prominence_run (items, nitems, W, what, stream);
	}

} // extern "C"
