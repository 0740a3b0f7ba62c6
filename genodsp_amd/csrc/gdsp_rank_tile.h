// gdsp_rank_tile.h -- the tile that gdsp_rankfilt.hip (slidingpercentile, median) and gdsp_localmad.hip (localmad,
// hampel) build alike: NS = 2^LOG_N staged inputs, sorted in LDS, and a wavelet matrix over their ranks that answers
// "which staged position holds the k-th smallest key of positions [lo, hi)" in LOG_N steps, whatever hi - lo is.
//
// Per tile (rf_tile_build):
//   1. sort of the (key, local index) pairs in LDS, ties by index, so the local ranks are a permutation: a bitonic
//      sort of each wave's block of 512 with no workgroup barrier, then pairwise merges of the blocks by binary search;
//   2. the rank-space sequence A[j] = rank of local position j;
//   3. a wavelet matrix over A: LOG_N levels, each a bit-vector (one ballot per 64 positions) with the count of
//      ones before every 64-bit word, each level the stable 0/1 partition of the one above.
// Per query (rf_tile_query): per level two rank queries (one 16-byte LDS read each) and a step into the zeros or the
// ones.  The rank found indexes the sorted local indices S.idx; the keys themselves are gone by then (they share a union
// with the levels), so a caller that wants the value reads the input again through S.idx.
//
// The tile is chosen at least about four windows long (NS >= 4(W-1), 1024 <= NS <= 8192), so at most a quarter of the
// sorted inputs are halo.  LDS at NS = 8192: the sorted local indices 16 KiB + 64 KiB that hold the keys while they are
// sorted and then the two level sequences (32 KiB) and 13 levels of (word, count) (26 KiB): 80 KiB, two 1024-thread
// workgroups per CU.  At NS = 1024: 10 KiB for 128 threads.
#pragma once

#include "gdsp_common.h"

#define RF_MIN_LOG 10
#define RF_MAX_LOG 13

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

// Stage in[s0 .. s0+nloc) (nloc <= NS), sort it and build the matrix: every thread of the NS/8-thread workgroup calls
// this, and the levels are complete when it returns.
template <int LOG_N>
__device__ __forceinline__
void rf_tile_build (RfLds<LOG_N>& S, const double* __restrict__ in, int64_t s0, int nloc)
	{
	constexpr int NS      = 1 << LOG_N;
	constexpr int THREADS = NS / 8;                                         // eight positions per thread
	const int      tid   = threadIdx.x;
	const int      lane  = tid & 63;
	const int      wave  = tid >> 6;

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
	}

// the rank, among the NS sorted pairs of the tile, of the k-th smallest (from 0) of the staged positions [lo, hi),
// 0 <= lo < hi <= NS and k < hi - lo: S.idx of it is a position of [lo, hi)
template <int LOG_N>
__device__ __forceinline__
uint32_t rf_tile_query (const RfLds<LOG_N>& S, uint32_t lo, uint32_t hi, uint32_t k)
	{
	uint32_t r = 0;
#pragma unroll
	for (int lv=0 ; lv<LOG_N ; lv++)
		{
		const uint32_t onesLo = rf_ones (S.u.w.level[lv], lo), onesHi = rf_ones (S.u.w.level[lv], hi);
		const uint32_t c = (hi - onesHi) - (lo - onesLo);                // zeros in [lo, hi)
		if (k < c) { lo = lo - onesLo;  hi = hi - onesHi; }
		else       { k -= c;  lo = S.u.w.zeros[lv] + onesLo;  hi = S.u.w.zeros[lv] + onesHi;  r |= 1u << (LOG_N - 1 - lv); }
		}
	return r;
	}

// the tile: NS >= 4(W-1), between 2^10 and 2^13
static inline int rf_tile_log (uint32_t W)
	{
	int lg = RF_MIN_LOG;
	while ((lg < RF_MAX_LOG) && ((1u << lg) < 4u * (W - 1))) lg++;
	return lg;
	}
