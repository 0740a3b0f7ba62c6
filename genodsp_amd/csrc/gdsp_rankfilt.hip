// gdsp_rankfilt.hip -- slidingpercentile / median: the exact p-th percentile over a sliding window.
//
// Not an operator of the reference.  Definition (include/genodsp_hip.h): for base i of a vector of n values the
// window is [max(0, i-wL), min(n-1, i+wR)] with wL = (W-1)/2, wR = W-1-wL (bestmax's centring and edge rule,
// minmax.c:1634-1640 in the reference: bases beyond the ends are not considered); with n_i bases in it,
// out[i] is the value of the k_i-th smallest key, k_i = gdsp_percentile_rank(n_i, P), keys as gdsp_key_of (the
// order `percentile` uses: -0.0 folded onto +0.0, NaNs ordered by their bits).  Only comparisons: bit exact.
//
// One workgroup owns T outputs and stages the NS = 2^LOG_N inputs they read (T = NS - (W-1); positions past the
// vector are padding that sorts last).  Per tile:
//   1. sort of the (key, local index) pairs in LDS, ties by index, so the local ranks are a permutation: a bitonic
//      sort of each wave's block of 512 with no workgroup barrier, then pairwise merges of the blocks by binary search;
//   2. the rank-space sequence A[j] = rank of local position j;
//   3. a wavelet matrix over A: LOG_N levels, each a bit-vector (one ballot per 64 positions) with the count of
//      ones before every 64-bit word, each level the stable 0/1 partition of the one above;
//   4. one range-quantile query per output over its local range [l, r) with rank k: per level two rank queries
//      (one 16-byte LDS read each) and a step into the zeros or the ones.  The rank found indexes the sorted local
//      indices, and the value is read back from the input.
// The cost per output is the tile's sort spread over T outputs plus LOG_N levels, whatever the window: the tile
// is chosen at least about four windows long (NS >= 4(W-1), 1024 <= NS <= 8192), so at most a quarter of the
// sorted inputs are halo.
//
// LDS at NS = 8192: the sorted local indices 16 KiB + 64 KiB that hold the keys while they are sorted and then the two
// level sequences (32 KiB) and 13 levels of (word, count) (26 KiB): 80 KiB, two 1024-thread workgroups per CU, so one
// tile's barriers overlap the other's work.  The result is read back from the input (L2) through the sorted index.
// At NS = 1024: 10 KiB for 128 threads.

#include "gdsp_common.h"

#define RF_MIN_LOG 10
#define RF_MAX_LOG 13
static_assert (2 * (GDSP_SLIDING_PERCENTILE_MAX_WINDOW - 1) < (1 << RF_MAX_LOG), "the largest window must leave half a tile of outputs");

struct RfWord { uint64_t bits;  uint32_t ones;  uint32_t pad; };          // one 64-position word of a level: bits, ones before it

template <int LOG_N>
struct RfLds
	{
	static constexpr int NS    = 1 << LOG_N;
	static constexpr int WORDS = NS / 64 + 1;                               // (+1: the rank of position NS)
	uint16_t idx[NS];                                                       // local index of each sorted key: where the result is read
	union
		{
		uint64_t key[NS];                                                   // staged keys, sorted in place; dead once sorted
		struct
			{
			uint16_t seq[NS], seq2[NS];                                     // rank-space sequence of the current / next level
			RfWord   level[LOG_N][WORDS];
			uint32_t zeros[LOG_N];
			} w;
		} u;
	};

// ones of a level before position p (0 <= p <= NS)
__device__ __forceinline__ uint32_t rf_ones (const RfWord* lv, uint32_t p)
	{
	const RfWord w = lv[p >> 6];
	const uint64_t below = (((uint64_t) 1) << (p & 63)) - 1;
	return w.ones + (uint32_t) __popcll (w.bits & below);
	}

// compare-exchange t of the bitonic stage (k, j): positions a (a 0 bit inserted at log2(j) into t) and a + j, ascending
// where bit log2(k) of a is 0 (everywhere for k = 0: the last stage of a block sorts every block ascending); ties by index
__device__ __forceinline__ void rf_exchange (uint64_t* key, uint16_t* idx, int t, int j, int k)
	{
	const int a = 2*t - (t & (j-1));
	const int b = a + j;
	const uint64_t ka = key[a], kb = key[b];
	const uint16_t ia = idx[a], ib = idx[b];
	const bool up      = ((a & k) == 0);
	const bool greater = (ka > kb) || ((ka == kb) && (ia > ib));
	if (greater == up) { key[a] = kb;  key[b] = ka;  idx[a] = ib;  idx[b] = ia; }
	}

// (key[q], idx[q]) < (ka, ia): the sort's order, ties by index
__device__ __forceinline__ bool rf_below (const uint64_t* key, const uint16_t* idx, int q, uint64_t ka, uint16_t ia)
	{ const uint64_t kq = key[q];  return (kq < ka) || ((kq == ka) && (idx[q] < ia)); }

// the LDS stores of this wave are seen by its own later loads (what __syncwarp does)
__device__ __forceinline__ void rf_wave_sync ()
	{
	__builtin_amdgcn_fence (__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier ();
	__builtin_amdgcn_fence (__ATOMIC_ACQUIRE, "wavefront");
	}

template <int LOG_N>
__device__ __forceinline__
void rankfilt_tile (const double* __restrict__ in, double* __restrict__ out, uint32_t n, uint32_t tile,
                    uint32_t wL, uint32_t wR, uint32_t pThousandths)
	{
	constexpr int NS      = 1 << LOG_N;
	constexpr int THREADS = NS / 8;                                         // eight positions per thread
	__shared__ RfLds<LOG_N> S;
	const int      tid   = threadIdx.x;
	const int      lane  = tid & 63;
	const int      wave  = tid >> 6;
	const int64_t  T     = NS - (int64_t) (wL + wR);                       // outputs per tile
	const int64_t  o0    = (int64_t) tile * T;                              // first output of the tile
	const int64_t  s0    = (o0 > (int64_t) wL)? o0 - wL : 0;                // first staged base
	const int64_t  send  = (o0 + T + wR < (int64_t) n)? o0 + T + wR : (int64_t) n;
	const int      nloc  = (int) (send - s0);                               // staged bases (<= NS)

	// ---- 1. stage the keys (padding: the largest key, sorted after every real one by its index)
	double x[8];
#pragma unroll
	for (int u=0 ; u<8 ; u++) { const int j = u*THREADS + tid;  x[u] = (j < nloc)? in[s0 + j] : 0.0; }    // all loads in flight
#pragma unroll
	for (int u=0 ; u<8 ; u++)
		{
		const int j = u*THREADS + tid;
		S.u.key[j] = (j < nloc)? gdsp_key_of (x[u]) : ~(uint64_t) 0;
		S.idx[j] = (uint16_t) j;
		}
	__syncthreads ();

	// ---- sort (key, idx), ties by idx.  First every aligned block of 512 by a bitonic sort inside the wave that owns it
	// (45 stages, each pairing positions of one block, four compare-exchanges per lane: no workgroup barrier); then the
	// blocks are merged pairwise, 512 -> 1024 -> ... -> NS: an element's place in the merged run is its offset in its own
	// run plus the count of the partner run's elements below it, found by a binary search (log2 s + 1 reads).  The pairs
	// are distinct, so the places form a permutation, and every thread moves its eight elements in place between two
	// barriers.  At NS = 8192 that is 45 wave-local stages and 4 merge levels in place of the 91 stages of a whole
	// bitonic sort, 46 of them over the whole tile.
	constexpr int BLOCK = (NS < 512)? NS : 512;
	for (int k=2 ; k<=BLOCK ; k<<=1)
		{
		for (int j=k>>1 ; j>0 ; j>>=1)
			{
#pragma unroll
			for (int u=0 ; u<4 ; u++) rf_exchange (S.u.key, S.idx, wave*256 + u*64 + lane, j, (k < BLOCK)? k : 0);
			rf_wave_sync ();
			}
		}
	for (int run=BLOCK ; run<NS ; run<<=1)
		{
		__syncthreads ();                                                   // the runs of length `run` are complete
		uint64_t mk[8];
		uint16_t mi[8];
		uint16_t dst[8];
#pragma unroll
		for (int u=0 ; u<8 ; u++)
			{
			const int p  = u*THREADS + tid;
			const int r0 = p & ~(2*run - 1);                                  // the merged run
			const int pb = r0 + ((p & run)? 0 : run);                         // the partner run
			const uint64_t ka = S.u.key[p];
			const uint16_t ia = S.idx[p];
			int c = 0;                                                        // partner elements below (ka, ia)
			for (int h=run>>1 ; h>0 ; h>>=1) { if (rf_below (S.u.key, S.idx, pb + c + h - 1, ka, ia)) c += h; }
			if (rf_below (S.u.key, S.idx, pb + c, ka, ia)) c++;
			mk[u] = ka;  mi[u] = ia;  dst[u] = (uint16_t) (r0 + (p & (run - 1)) + c);
			}
		__syncthreads ();                                                   // every search has read the runs
#pragma unroll
		for (int u=0 ; u<8 ; u++) { S.u.key[dst[u]] = mk[u];  S.idx[dst[u]] = mi[u]; }
		}
	__syncthreads ();

	// ---- 2. rank-space sequence: seq[local index] = rank
	for (int r=tid ; r<NS ; r+=THREADS) S.u.w.seq[S.idx[r]] = (uint16_t) r;
	__syncthreads ();

	// ---- 3. wavelet matrix: wave w owns positions [512w, 512w+512) = words 8w .. 8w+7
	uint16_t* cur = S.u.w.seq;
	uint16_t* nxt = S.u.w.seq2;
	for (int lv=0 ; lv<LOG_N ; lv++)
		{
		const int bit = LOG_N - 1 - lv;
		uint64_t mask[8];
		uint16_t val[8];
#pragma unroll
		for (int u=0 ; u<8 ; u++)
			{
			val[u]  = cur[wave*512 + u*64 + lane];
			mask[u] = __ballot ((val[u] >> bit) & 1);
			}
		if (lane == 0)
			{
#pragma unroll
			for (int u=0 ; u<8 ; u++) S.u.w.level[lv][wave*8 + u].bits = mask[u];
			}
		__syncthreads ();
		if (wave == 0)                                                      // ones before every word: one wave scans <= 128 words
			{
			constexpr int NW = NS / 64;
			constexpr int per = (NW + 63) / 64;                               // words per lane (1 or 2)
			uint32_t c[2] = { 0, 0 };
			uint32_t tot = 0;
			for (int q=0 ; q<per ; q++)
				{
				const int w = lane*per + q;
				c[q] = (w < NW)? (uint32_t) __popcll (S.u.w.level[lv][w].bits) : 0u;
				tot += c[q];
				}
			uint32_t incl = tot;
			for (int d=1 ; d<64 ; d*=2)
				{
				const uint32_t o = __shfl_up (incl, d, 64);
				if (lane >= d) incl += o;
				}
			uint32_t run = incl - tot;
			for (int q=0 ; q<per ; q++)
				{
				const int w = lane*per + q;
				if (w < NW) S.u.w.level[lv][w].ones = run;
				run += c[q];
				}
			if (lane == 63)
				{
				S.u.w.level[lv][NW].bits = 0;
				S.u.w.level[lv][NW].ones = incl;
				S.u.w.zeros[lv] = NS - incl;
				}
			}
		__syncthreads ();
		if (lv + 1 < LOG_N)                                                 // stable partition into the next level
			{
			const uint32_t z = S.u.w.zeros[lv];
			const uint64_t lt = (((uint64_t) 1) << lane) - 1;
#pragma unroll
			for (int u=0 ; u<8 ; u++)
				{
				const int      p    = wave*512 + u*64 + lane;
				const uint32_t ones = S.u.w.level[lv][wave*8 + u].ones + (uint32_t) __popcll (mask[u] & lt);
				const bool     one  = (val[u] >> bit) & 1;
				nxt[one? z + ones : (uint32_t) p - ones] = val[u];
				}
			__syncthreads ();
			uint16_t* t = cur;  cur = nxt;  nxt = t;
			}
		}

	// ---- 4. one range-quantile query per output
	for (int64_t o=tid ; o<T ; o+=THREADS)
		{
		const int64_t i = o0 + o;
		if (i >= (int64_t) n) break;
		const int64_t first = (i > (int64_t) wL)? i - wL : 0;
		const int64_t last  = (i + wR < (int64_t) n)? i + wR : (int64_t) n - 1;
		uint32_t lo = (uint32_t) (first - s0), hi = (uint32_t) (last + 1 - s0);
		uint32_t k  = gdsp_rank_of (hi - lo, pThousandths);
		uint32_t r  = 0;
#pragma unroll
		for (int lv=0 ; lv<LOG_N ; lv++)
			{
			const uint32_t onesLo = rf_ones (S.u.w.level[lv], lo), onesHi = rf_ones (S.u.w.level[lv], hi);
			const uint32_t c = (hi - onesHi) - (lo - onesLo);                // zeros in [lo, hi)
			if (k < c) { lo = lo - onesLo;  hi = hi - onesHi; }
			else       { k -= c;  lo = S.u.w.zeros[lv] + onesLo;  hi = S.u.w.zeros[lv] + onesHi;  r |= 1u << (LOG_N - 1 - lv); }
			}
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

// the tile: NS >= 4(W-1), between 2^10 and 2^13
static int rankfilt_log (uint32_t W)
	{
	int lg = RF_MIN_LOG;
	while ((lg < RF_MAX_LOG) && ((1u << lg) < 4u * (W - 1))) lg++;
	return lg;
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
	switch (rankfilt_log (W))
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
	return (1u << rankfilt_log (W)) - (W - 1);
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
