// gdsp_intervalpct.hip -- percentilesover / medianover (not in the reference): the exact order statistics of one signal
// over millions of arbitrary intervals -- short and long, overlapping, in any order (include/genodsp_hip.h).  A value is
// an input value chosen by integer comparisons of keys (gdsp_key_of, gdsp_rank_of: percentile's order and rank rule), so
// nothing here depends on tiles, grids, dispatch order or the route an interval takes.
//
// The host sorts the intervals of a call into two routes by length.
//
// SHORT (at most IP_SHORT bases): the signal is read once.  The interval's keys are staged in LDS -- a base outside the
// sample becomes the all-ones key (a NaN's: never a sampled value) and is not counted -- and sorted with the routines of
// gdsp_rank_tile.h; every k_j is then read off the sorted keys.  An interval of at most IP_WAVE_MAX bases is sorted by
// ONE wave (a bitonic sort over the next power of two, no workgroup barrier), and a workgroup of four waves takes
// IP_WAVE_ITEMS consecutive such intervals, so a million 100-base bins do not occupy a workgroup each.  Longer ones take
// a workgroup of NS/8 threads, NS = 1024, 2048 or 4096: each wave sorts its block of 512, the blocks are merged pairwise
// by binary search (the sort of rf_tile_build).
//
// LONG: a most-significant-digit radix select over the keys in HBM, for all (interval, percentile) queries of a batch at
// once and in stream order -- no host round trip between digits.  A long interval is cut into pieces of IP_PIECE bases,
// one workgroup per piece and pass.  A query keeps { prefix, remaining rank, smallest and largest matching key } in
// workspace.  In a pass the workgroup walks its piece IP_BLOCK keys at a time, in registers, and counts the current digit
// of the keys that match each still-open query's prefix into that query's LDS bins, IP_GROUP queries of its interval side
// by side (one LDS atomic per run of equal digits in a lane's eight consecutive bases: read depth is piecewise
// constant; an interval with more open queries has its piece read again per further group).  At the piece's end it adds
// the non-empty bins to each query's histogram with agent-scope atomics -- once per piece, so a whole chromosome's
// workgroups do not queue on a handful of hot addresses -- and folds the matching keys' extremes into the query.  A one-wave launch per query
// then walks the counts to the bin that holds the rank, clears the histogram and advances the state; a query whose
// smallest and largest matching key are equal is settled -- every candidate left is that value -- and its workgroups
// leave at once in later passes (integer depth: three of six passes).  No workgroup waits for another.  The histograms
// are IP_BINS 32-bit counts per query (an interval has at most 2^32 - 1 bases); a call with more long queries than the
// workspace holds runs them in batches of whole intervals.
// The refusals of a call's vectors and intervals are gdsp_interval_cut.h's (ic_check), shared with statsover and
// breadthover; nothing else of that header is used here: these routes do not cut at frame tiles.

#include <math.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "gdsp_common.h"
#include "gdsp_pieces.h"
#include "gdsp_interval_cut.h"
#include "gdsp_rank_tile.h"

#define IP_WAVE_MAX     512                           // bases one wave sorts
#define IP_WAVE_THREADS 256
#define IP_WAVE_ITEMS   16                            // consecutive one-wave intervals a workgroup takes
#define IP_MIN_LOG      10
#define IP_MAX_LOG      12
#define IP_SHORT        (1u << IP_MAX_LOG)            // bases: the longest interval of the one-read route
#define IP_PIECE        65536                         // bases of a long interval one workgroup takes per pass
#define IP_BLOCK        8192                          // of them in registers at a time
#define IP_GROUP        4                             // queries of an interval counted side by side in LDS
#define IP_THREADS      256
#define IP_PER          8                             // consecutive bases of a lane
#define IP_ROUNDS       (IP_BLOCK / (IP_THREADS * IP_PER))
#define IP_BITS         11
#define IP_BINS         (1 << IP_BITS)
#define IP_PASSES       6                             // digits of 11, 11, 11, 11, 11 and 9 bits
#define IP_PICK_THREADS 64
#define IP_CHUNK        (1u << 20)                    // intervals of one read-back
#define IP_BATCH_QUERIES 16384u                       // long queries of a batch by default: 128 MiB of histograms
#define IP_BATCH_PIECES (1u << 20)                    // pieces of a batch (one interval has at most 2^16)
#define IP_NONE         (~(uint64_t) 0)               // the key of a base outside the sample

static_assert (IP_ROUNDS * IP_THREADS * IP_PER == IP_BLOCK && IP_PIECE % IP_BLOCK == 0, "a piece is whole rounds of the workgroup");
static_assert (IP_SHORT <= 8192 && (IP_SHORT & (IP_SHORT - 1)) == 0, "the short limit of the header");
static_assert (GDSP_INTERVAL_PERCENTILES_MAX <= 32, "the open queries of an interval are a 32-bit mask");

struct IpPcts  { uint32_t p[GDSP_INTERVAL_PERCENTILES_MAX]; };                 // in the kernarg segment
struct IpShort { const double* v;  uint32_t len, slot; };                       // a short interval: its first base, its row
struct IpPiece { const double* v;  uint32_t len, q0; };                         // a piece and the first query of its interval
struct IpQuery                                                                  // a long (interval, percentile) query
	{
	uint64_t prefix, kmin, kmax;           // digits chosen so far; extremes of the matching keys of the running pass
	uint32_t rank, p;                      // rank left inside the prefix; the percentile
	uint32_t open, passes;                 // still selecting; histogram passes it was open for
	uint32_t valueSlot, countSlot;         // where its value goes, and (first query of an interval, else UINT32_MAX) the count
	};
static_assert (sizeof(IpShort) == 16 && sizeof(IpPiece) == 16 && sizeof(IpQuery) == 48, "records as staged");

// the key of a base, IP_NONE outside the sample: statsover's tests
__device__ __forceinline__ uint64_t ip_key (double x, double lo, double hi)
	{
	const bool in = !(x < lo) && !(x > hi) && (fabs (x) <= 1.7976931348623157e308);      // (false for NaN and +-inf)
	return in? gdsp_key_of (x) : IP_NONE;
	}

// ---------------------------------------------------------------------------------- short: one wave ----
struct IpWaveLds { uint64_t key[IP_WAVE_THREADS/64][IP_WAVE_MAX];  uint16_t idx[IP_WAVE_THREADS/64][IP_WAVE_MAX]; };

__global__ __launch_bounds__(IP_WAVE_THREADS)
void ip_wave_kernel (const IpShort* __restrict__ items, uint32_t nitems, IpPcts P, int np, double lo, double hi,
                     uint32_t* __restrict__ count, double* __restrict__ values)
	{
	__shared__ IpWaveLds S;
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	uint64_t* key = S.key[wave];
	uint16_t* idx = S.idx[wave];
	const uint32_t first = blockIdx.x * IP_WAVE_ITEMS;
	for (uint32_t it=first+wave ; (it<first+IP_WAVE_ITEMS) && (it<nitems) ; it+=IP_WAVE_THREADS/64)
		{
		const IpShort   w   = items[it];
		const double*   v   = w.v;
		const int       len = (int) __builtin_amdgcn_readfirstlane (w.len);
		int B = 2;
		while (B < len) B <<= 1;
		uint32_t m = 0;
		for (int j=lane ; j<B ; j+=64)
			{
			const uint64_t k = (j < len)? ip_key (v[j], lo, hi) : IP_NONE;
			key[j] = k;  idx[j] = (uint16_t) j;
			m += (k != IP_NONE);
			}
		for (int off=32 ; off>0 ; off>>=1) m += __shfl_xor (m, off, 64);
		rf_wave_sync ();
		for (int k=2 ; k<=B ; k<<=1)
			{
			for (int j=k>>1 ; j>0 ; j>>=1)
				{
				for (int t=lane ; t<B/2 ; t+=64) rf_exchange (key, idx, t, j, k);          // (k == B: every pair ascends)
				rf_wave_sync ();
				}
			}
		if (lane < np)
			values[(size_t) w.slot * np + lane] = (m != 0)? gdsp_value_of (key[gdsp_rank_of (m, P.p[lane])]) : __builtin_nan ("");
		if (lane == 0) count[w.slot] = m;
		rf_wave_sync ();                                                    // the keys were read before the next interval's are staged
		}
	}

// ----------------------------------------------------------------------------- short: one workgroup ----
template <int LOG_N>
struct IpBlockLds { uint64_t key[1 << LOG_N];  uint16_t idx[1 << LOG_N];  uint32_t m; };

template <int LOG_N>
__global__ __launch_bounds__((1 << LOG_N) / 8)
void ip_block_kernel (const IpShort* __restrict__ items, IpPcts P, int np, double lo, double hi,
                      uint32_t* __restrict__ count, double* __restrict__ values)
	{
	constexpr int NS      = 1 << LOG_N;
	constexpr int THREADS = NS / 8;
	__shared__ IpBlockLds<LOG_N> S;
	const IpShort w    = items[blockIdx.x];
	const double* v    = w.v;
	const int     len  = (int) __builtin_amdgcn_readfirstlane (w.len);
	const int     tid  = threadIdx.x, lane = tid & 63, wave = tid >> 6;

	if (tid == 0) S.m = 0;
	double x[8];
#pragma unroll
	for (int u=0 ; u<8 ; u++) { const int j = u*THREADS + tid;  x[u] = v[(j < len)? j : len-1]; }      // all loads in flight
	__syncthreads ();
	uint32_t m = 0;
#pragma unroll
	for (int u=0 ; u<8 ; u++)
		{
		const int j = u*THREADS + tid;
		const uint64_t k = (j < len)? ip_key (x[u], lo, hi) : IP_NONE;
		S.key[j] = k;  S.idx[j] = (uint16_t) j;
		m += (k != IP_NONE);
		}
	for (int off=32 ; off>0 ; off>>=1) m += __shfl_xor (m, off, 64);
	if ((lane == 0) && (m != 0)) atomicAdd (&S.m, m);
	__syncthreads ();

	// the sort of rf_tile_build: each wave's block of 512 by a bitonic sort of its own, then pairwise merges by binary search
	for (int k=2 ; k<=512 ; k<<=1)
		{
		for (int j=k>>1 ; j>0 ; j>>=1)
			{
#pragma unroll
			for (int u=0 ; u<4 ; u++) rf_exchange (S.key, S.idx, wave*256 + u*64 + lane, j, (k < 512)? k : 0);
			rf_wave_sync ();
			}
		}
	for (int run=512 ; run<NS ; run<<=1)
		{
		__syncthreads ();
		uint64_t mk[8];
		uint16_t mi[8], dst[8];
#pragma unroll
		for (int u=0 ; u<8 ; u++)
			{
			const int p  = u*THREADS + tid;
			const int r0 = p & ~(2*run - 1);
			const int pb = r0 + ((p & run)? 0 : run);
			const uint64_t ka = S.key[p];
			const uint16_t ia = S.idx[p];
			int c = 0;
			for (int h=run>>1 ; h>0 ; h>>=1) { if (rf_below (S.key, S.idx, pb + c + h - 1, ka, ia)) c += h; }
			if (rf_below (S.key, S.idx, pb + c, ka, ia)) c++;
			mk[u] = ka;  mi[u] = ia;  dst[u] = (uint16_t) (r0 + (p & (run - 1)) + c);
			}
		__syncthreads ();
#pragma unroll
		for (int u=0 ; u<8 ; u++) { S.key[dst[u]] = mk[u];  S.idx[dst[u]] = mi[u]; }
		}
	__syncthreads ();

	const uint32_t total = S.m;
	if (tid < np)
		values[(size_t) w.slot * np + tid] = (total != 0)? gdsp_value_of (S.key[gdsp_rank_of (total, P.p[tid])]) : __builtin_nan ("");
	if (tid == 0) count[w.slot] = total;
	}

// ------------------------------------------------------------------------------------ long: one pass ----
__global__ __launch_bounds__(IP_THREADS)
void ip_hist_kernel (const IpPiece* __restrict__ pieces, IpQuery* Q, uint32_t* __restrict__ hist, int np,
                     int shift, int bits, double lo, double hi)
	{
	__shared__ uint32_t bins[IP_GROUP][IP_BINS];
	const IpPiece  w   = pieces[blockIdx.x];
	const double*  v   = w.v;
	const uint32_t len = __builtin_amdgcn_readfirstlane (w.len);
	const uint32_t q0  = __builtin_amdgcn_readfirstlane (w.q0);
	uint32_t open = 0;
	for (int j=0 ; j<np ; j++) open |= (Q[q0 + j].open != 0)? (1u << j) : 0u;
	open = __builtin_amdgcn_readfirstlane (open);
	if (open == 0) return;                                                  // every query of the interval is settled

	const int      nbins = 1 << bits;
	const uint32_t mask  = (uint32_t) nbins - 1;
	const int      above = shift + bits;                                    // key bits [above, 64) must equal the prefix's
	const int      lane  = threadIdx.x & 63;
	for (int j0=0 ; j0<np ; j0+=IP_GROUP)                                   // IP_GROUP queries side by side; a further group reads the piece again
		{
		const uint32_t grp = (open >> j0) & ((1u << IP_GROUP) - 1);
		if (grp == 0) continue;
		uint64_t prefix[IP_GROUP], kmin[IP_GROUP], kmax[IP_GROUP];
#pragma unroll
		for (int g=0 ; g<IP_GROUP ; g++)
			{
			prefix[g] = (((grp >> g) & 1) != 0)? Q[q0 + j0 + g].prefix : 0;
			kmin[g] = IP_NONE;  kmax[g] = 0;
			for (int b=threadIdx.x ; b<nbins ; b+=IP_THREADS) bins[g][b] = 0;
			}
		__syncthreads ();

		for (uint32_t b0=0 ; b0<len ; b0+=IP_BLOCK)
			{
			// IP_BLOCK keys in registers, once for the group's queries: a lane's IP_PER consecutive bases per round
			uint64_t key[IP_ROUNDS][IP_PER];
#pragma unroll
			for (int r=0 ; r<IP_ROUNDS ; r++)
				{
				const uint32_t p = b0 + (uint32_t) r * IP_THREADS * IP_PER + threadIdx.x * IP_PER;
				double x[IP_PER];
#pragma unroll
				for (int i=0 ; i<IP_PER ; i++) x[i] = v[(p + i < len)? p + i : len - 1];
#pragma unroll
				for (int i=0 ; i<IP_PER ; i++) key[r][i] = (p + i < len)? ip_key (x[i], lo, hi) : IP_NONE;
				}
#pragma unroll
			for (int g=0 ; g<IP_GROUP ; g++)
				{
				if (((grp >> g) & 1) == 0) continue;
#pragma unroll
				for (int r=0 ; r<IP_ROUNDS ; r++)
					{
					uint32_t runBin = 0xFFFFFFFFu, runCnt = 0;
#pragma unroll
					for (int i=0 ; i<IP_PER ; i++)
						{
						const uint64_t k = key[r][i];
						if (k == IP_NONE) continue;
						if ((above < 64) && ((k >> above) != (prefix[g] >> above))) continue;
						const uint32_t bin = (uint32_t) (k >> shift) & mask;
						kmin[g] = (k < kmin[g])? k : kmin[g];
						kmax[g] = (k > kmax[g])? k : kmax[g];
						if (bin == runBin) runCnt++;
						else
							{
							if (runCnt != 0) atomicAdd (&bins[g][runBin], runCnt);
							runBin = bin;  runCnt = 1;
							}
						}
					if (runCnt != 0) atomicAdd (&bins[g][runBin], runCnt);
					}
				}
			}
		__syncthreads ();

#pragma unroll
		for (int g=0 ; g<IP_GROUP ; g++)
			{
			if (((grp >> g) & 1) == 0) continue;
			IpQuery&  q    = Q[q0 + j0 + g];
			uint32_t* mine = hist + (size_t) (q0 + j0 + g) * IP_BINS;
			for (int b=threadIdx.x ; b<nbins ; b+=IP_THREADS) { const uint32_t c = bins[g][b];  if (c != 0) atomicAdd (&mine[b], c); }
			uint64_t lo64 = kmin[g], hi64 = kmax[g];
			for (int off=32 ; off>0 ; off>>=1)
				{
				const uint64_t a = __shfl_down ((unsigned long long) lo64, off, 64);
				const uint64_t b = __shfl_down ((unsigned long long) hi64, off, 64);
				lo64 = (a < lo64)? a : lo64;
				hi64 = (b > hi64)? b : hi64;
				}
			if ((lane == 0) && (lo64 <= hi64))
				{
				atomicMin ((unsigned long long*) &q.kmin, (unsigned long long) lo64);
				atomicMax ((unsigned long long*) &q.kmax, (unsigned long long) hi64);
				}
			}
		__syncthreads ();                                                   // the bins were read before the next group clears them
		}
	}

// one wave per query: walk the pass's counts to the bin that holds the rank, clear them, advance the state
__global__ __launch_bounds__(IP_PICK_THREADS)
void ip_pick_kernel (IpQuery* Q, uint32_t* __restrict__ hist, int pass, int shift, int bits,
                     uint32_t* __restrict__ count, double* __restrict__ values)
	{
	__shared__ uint32_t bins[IP_BINS + IP_BINS/32];
	constexpr int PER = IP_BINS / IP_PICK_THREADS;                          // consecutive bins of a lane
	IpQuery& q = Q[blockIdx.x];
	if (q.open == 0) return;
	const int lane  = threadIdx.x;
	const int nbins = 1 << bits;
	uint32_t* mine = hist + (size_t) blockIdx.x * IP_BINS;
	for (int b=lane ; b<nbins ; b+=IP_PICK_THREADS) { bins[b + (b >> 5)] = mine[b];  mine[b] = 0; }
	rf_wave_sync ();
	uint32_t c[PER], sum = 0;
#pragma unroll
	for (int i=0 ; i<PER ; i++) { const int b = lane*PER + i;  c[i] = (b < nbins)? bins[b + (b >> 5)] : 0u;  sum += c[i]; }
	uint32_t incl = sum;
	for (int d=1 ; d<64 ; d*=2) { const uint32_t o = __shfl_up (incl, d, 64);  if (lane >= d) incl += o; }
	const uint32_t total = __shfl (incl, 63, 64);

	const uint64_t kmin = q.kmin, kmax = q.kmax;
	uint32_t rank = q.rank;
	if (pass == 0)                                                          // the first pass counted the sample
		{
		rank = gdsp_rank_of (total, q.p);
		if ((lane == 0) && (q.countSlot != UINT32_MAX)) count[q.countSlot] = total;
		}
	if ((total == 0) || (kmin == kmax) || (pass + 1 == IP_PASSES))
		{
		// nothing sampled; every candidate is one value; or the last digit is being chosen
		uint64_t key = kmin;
		if ((total != 0) && (kmin != kmax))
			{
			const uint32_t before = incl - sum;
			uint32_t seen = before;
			key = 0;
#pragma unroll
			for (int i=0 ; i<PER ; i++)
				{
				if ((rank >= seen) && (rank < seen + c[i])) key = q.prefix | ((uint64_t) (lane*PER + i) << shift);
				seen += c[i];
				}
			for (int off=32 ; off>0 ; off>>=1) key |= __shfl_xor ((unsigned long long) key, off, 64);
			}
		if (lane == 0)
			{
			values[q.valueSlot] = (total != 0)? gdsp_value_of (key) : __builtin_nan ("");
			q.open = 0;  q.passes = (uint32_t) pass + 1;
			}
		return;
		}
	uint32_t seen = incl - sum;
#pragma unroll
	for (int i=0 ; i<PER ; i++)
		{
		if ((rank >= seen) && (rank < seen + c[i]))                         // one lane, one bin
			{
			q.prefix |= (uint64_t) (lane*PER + i) << shift;
			q.rank    = rank - seen;
			q.kmin    = IP_NONE;  q.kmax = 0;
			q.passes  = (uint32_t) pass + 1;
			}
		seen += c[i];
		}
	}

// ---------------------------------------------------------------------------------------------- host ----
// the histograms: device memory only, grown on demand and kept (gdsp_malloc's: cleared before the first pass reads them)
struct IpDeviceWords
	{
	uint32_t* d;  size_t cap;
	int grow (size_t want)
		{
		if (want <= cap) return GDSP_OK;
		if (d != NULL) { (void) gdsp_free (d);  d = NULL; }
		cap = 0;
		if (gdsp_malloc ((void**) &d, want * sizeof(uint32_t)) != GDSP_OK) { d = NULL;  return GDSP_ENOMEM; }
		cap = want;
		return GDSP_OK;
		}
	};

struct IpBuffers
	{
	GdspStaged<IpShort>  shorts;
	GdspStaged<IpPiece>  pieces;
	GdspStaged<IpQuery>  queries;
	GdspStaged<uint32_t> count;
	GdspStaged<double>   values;
	IpDeviceWords        hist;
	};
static IpBuffers ipBuffers[64];
static uint64_t  ipLast[6];
static uint32_t  ipBatchQueries = 0;

static inline int ip_class_of (uint32_t len)                               // 0: one wave; 1..3: a workgroup of 2^(9+c) keys
	{
	if (len <= IP_WAVE_MAX) return 0;
	int c = 1;
	while ((1u << (IP_MIN_LOG + c - 1)) < len) c++;
	return c;
	}

// the long intervals lng[0 .. nl) of the chunk that starts at interval i0, in batches of whole intervals
static int ip_long (IpBuffers& W, const gdsp_batch_item* items, const uint32_t* h_vec, const uint32_t* h_start, const uint32_t* h_end,
                    uint32_t i0, const std::vector<uint32_t>& lng, const uint32_t* pThousandths, int np,
                    double lo, double hi, hipStream_t s)
	{
	const uint32_t limit = (ipBatchQueries != 0)? ipBatchQueries : IP_BATCH_QUERIES;
	size_t a = 0;
	while (a < lng.size ())
		{
		size_t   b = a;
		uint64_t nq = 0, npieces = 0;
		while (b < lng.size ())
			{
			const uint32_t i   = lng[b];
			const uint64_t pcs = ((uint64_t) (h_end[i] - h_start[i]) + IP_PIECE - 1) / IP_PIECE;
			if ((b > a) && ((nq + (uint64_t) np > limit) || (npieces + pcs > IP_BATCH_PIECES))) break;
			nq += (uint64_t) np;  npieces += pcs;  b++;
			}
		int rc = W.pieces.grow (npieces, "gdsp_interval_percentiles");
		if (rc == GDSP_OK) rc = W.queries.grow (nq, "gdsp_interval_percentiles", 0, 4096);
		if (rc == GDSP_OK) rc = W.hist.grow ((size_t) nq * IP_BINS);
		if (rc != GDSP_OK) return rc;
		uint32_t piece = 0, query = 0;
		for (size_t k=a ; k<b ; k++)
			{
			const uint32_t i   = lng[k];
			const double*  v   = items[(h_vec != NULL)? h_vec[i] : 0].d_in + h_start[i];
			const uint32_t len = h_end[i] - h_start[i];
			for (uint64_t off=0 ; off<len ; off+=IP_PIECE)
				{
				IpPiece& pc = W.pieces.h[piece++];
				pc.v = v + off;  pc.len = (uint32_t) std::min<uint64_t> (IP_PIECE, len - off);  pc.q0 = query;
				}
			for (int j=0 ; j<np ; j++)
				{
				IpQuery& q = W.queries.h[query++];
				q.prefix = 0;  q.kmin = IP_NONE;  q.kmax = 0;  q.rank = 0;  q.p = pThousandths[j];  q.open = 1;  q.passes = 0;
				q.valueSlot = (i - i0) * (uint32_t) np + (uint32_t) j;
				q.countSlot = (j == 0)? i - i0 : UINT32_MAX;
				}
			}
		GDSP_HIP_TRY (hipMemcpyAsync (W.pieces.d, W.pieces.h, (size_t) npieces * sizeof(IpPiece), hipMemcpyHostToDevice, s));
		GDSP_HIP_TRY (hipMemcpyAsync (W.queries.d, W.queries.h, (size_t) nq * sizeof(IpQuery), hipMemcpyHostToDevice, s));
		GDSP_HIP_TRY (hipMemsetAsync (W.hist.d, 0, (size_t) nq * IP_BINS * sizeof(uint32_t), s));
		for (int pass=0 ; pass<IP_PASSES ; pass++)
			{
			const int bits  = (pass + 1 < IP_PASSES)? IP_BITS : 64 - (IP_PASSES - 1) * IP_BITS;
			const int shift = (pass + 1 < IP_PASSES)? 64 - (pass + 1) * IP_BITS : 0;
			hipLaunchKernelGGL (ip_hist_kernel, dim3((uint32_t) npieces), dim3(IP_THREADS), 0, s, W.pieces.d, W.queries.d, W.hist.d, np,
			                    shift, bits, lo, hi);
			GDSP_LAUNCH_CHECK ();
			hipLaunchKernelGGL (ip_pick_kernel, dim3((uint32_t) nq), dim3(IP_PICK_THREADS), 0, s, W.queries.d, W.hist.d, pass, shift, bits,
			                    W.count.d, W.values.d);
			GDSP_LAUNCH_CHECK ();
			}
		GDSP_HIP_TRY (hipMemcpyAsync (W.queries.h, W.queries.d, (size_t) nq * sizeof(IpQuery), hipMemcpyDeviceToHost, s));
		GDSP_HIP_TRY (hipStreamSynchronize (s));
		uint32_t passes = 0;
		for (uint64_t k=0 ; k<nq ; k++)
			{
			passes = std::max (passes, W.queries.h[k].passes);
			ipLast[5] += (W.queries.h[k].passes < IP_PASSES);
			}
		ipLast[3] += passes;  ipLast[4]++;
		a = b;
		}
	return GDSP_OK;
	}

// intervals [i0, i1) of the call: their rows into h_count and h_values
static int ip_chunk (IpBuffers& W, const gdsp_batch_item* items, const uint32_t* h_vec, const uint32_t* h_start, const uint32_t* h_end,
                     uint32_t i0, uint32_t i1, const IpPcts& P, const uint32_t* pThousandths, int np, double lo, double hi,
                     uint32_t* h_count, double* h_values, hipStream_t s)
	{
	const uint32_t nsel = i1 - i0;
	constexpr int  CLASSES = IP_MAX_LOG - IP_MIN_LOG + 2;
	uint32_t classFirst[CLASSES + 1] = { 0 };
	std::vector<uint32_t> lng;
	for (uint32_t i=i0 ; i<i1 ; i++)
		{
		const uint32_t len = h_end[i] - h_start[i];
		if (len > IP_SHORT) lng.push_back (i);
		else                classFirst[ip_class_of (len) + 1]++;
		}
	for (int c=0 ; c<CLASSES ; c++) classFirst[c+1] += classFirst[c];
	const uint32_t nshort = classFirst[CLASSES];
	int rc = W.count.grow (nsel, "gdsp_interval_percentiles");
	if (rc == GDSP_OK) rc = W.values.grow ((size_t) nsel * np, "gdsp_interval_percentiles");
	if (rc == GDSP_OK) rc = W.shorts.grow (nshort, "gdsp_interval_percentiles");
	if (rc != GDSP_OK) return rc;

	// the short intervals, class by class, the caller's order kept inside a class (consecutive bins stay neighbours)
	if (nshort != 0)
		{
		uint32_t cursor[CLASSES];
		for (int c=0 ; c<CLASSES ; c++) cursor[c] = classFirst[c];
		for (uint32_t i=i0 ; i<i1 ; i++)
			{
			const uint32_t len = h_end[i] - h_start[i];
			if (len > IP_SHORT) continue;
			IpShort& w = W.shorts.h[cursor[ip_class_of (len)]++];
			w.v = items[(h_vec != NULL)? h_vec[i] : 0].d_in + h_start[i];  w.len = len;  w.slot = i - i0;
			}
		GDSP_HIP_TRY (hipMemcpyAsync (W.shorts.d, W.shorts.h, (size_t) nshort * sizeof(IpShort), hipMemcpyHostToDevice, s));
		for (int c=0 ; c<CLASSES ; c++)
			{
			const uint32_t cnt = classFirst[c+1] - classFirst[c];
			const IpShort* d   = W.shorts.d + classFirst[c];
			if (cnt == 0) continue;
			if (c == 0)
				hipLaunchKernelGGL (ip_wave_kernel, dim3((cnt + IP_WAVE_ITEMS - 1) / IP_WAVE_ITEMS), dim3(IP_WAVE_THREADS), 0, s,
				                    d, cnt, P, np, lo, hi, W.count.d, W.values.d);
			else if (c == 1)
				hipLaunchKernelGGL (ip_block_kernel<10>, dim3(cnt), dim3(128), 0, s, d, P, np, lo, hi, W.count.d, W.values.d);
			else if (c == 2)
				hipLaunchKernelGGL (ip_block_kernel<11>, dim3(cnt), dim3(256), 0, s, d, P, np, lo, hi, W.count.d, W.values.d);
			else
				hipLaunchKernelGGL (ip_block_kernel<12>, dim3(cnt), dim3(512), 0, s, d, P, np, lo, hi, W.count.d, W.values.d);
			GDSP_LAUNCH_CHECK ();
			}
		}
	if (!lng.empty ())
		{
		rc = ip_long (W, items, h_vec, h_start, h_end, i0, lng, pThousandths, np, lo, hi, s);
		if (rc != GDSP_OK) return rc;
		}
	GDSP_HIP_TRY (hipMemcpyAsync (W.count.h, W.count.d, (size_t) nsel * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
	GDSP_HIP_TRY (hipMemcpyAsync (W.values.h, W.values.d, (size_t) nsel * np * sizeof(double), hipMemcpyDeviceToHost, s));
	GDSP_HIP_TRY (hipStreamSynchronize (s));
	memcpy (h_count + i0, W.count.h, (size_t) nsel * sizeof(uint32_t));
	memcpy (h_values + (size_t) i0 * np, W.values.h, (size_t) nsel * np * sizeof(double));
	ipLast[0] += nsel;  ipLast[1] += nshort;  ipLast[2] += lng.size ();
	return GDSP_OK;
	}

extern "C" {

uint32_t gdsp_interval_percentiles_short (void) { return IP_SHORT; }
uint32_t gdsp_interval_percentiles_piece (void) { return IP_PIECE; }

int gdsp_interval_percentiles_set_batch (uint32_t longQueries) { ipBatchQueries = longQueries;  return GDSP_OK; }

int gdsp_interval_percentiles_batch (const gdsp_batch_item* items, int nitems, const uint32_t* h_vec, const uint32_t* h_start,
                                     const uint32_t* h_end, uint32_t count, const uint32_t* pThousandths, int np,
                                     double lo, double hi, uint32_t* h_count, double* h_values, void* stream)
	{
	memset (ipLast, 0, sizeof(ipLast));
	GDSP_REQUIRE ((np >= 1) && (np <= GDSP_INTERVAL_PERCENTILES_MAX), "the number of percentiles must be 1..16");
	GDSP_REQUIRE (pThousandths != NULL, "NULL percentiles");
	for (int j=0 ; j<np ; j++) GDSP_REQUIRE (pThousandths[j] <= 100000, "a percentile is above 100000 thousandths");
	if (count == 0) return GDSP_OK;
	int rc = ic_check (__func__, items, nitems, h_vec, h_start, h_end, count);
	if (rc != GDSP_OK) return rc;
	GDSP_REQUIRE ((h_count != NULL) && (h_values != NULL), "NULL result array");
	hipStream_t s = gdsp_stream (stream);
	int dev = 0;
	rc = gdsp_device_slot (&dev);
	if (rc != GDSP_OK) return rc;
	IpPcts P;
	for (int j=0 ; j<GDSP_INTERVAL_PERCENTILES_MAX ; j++) P.p[j] = (j < np)? pThousandths[j] : 0;
	for (uint64_t i0=0 ; (i0<count) && (rc == GDSP_OK) ; i0+=IP_CHUNK)
		rc = ip_chunk (ipBuffers[dev], items, h_vec, h_start, h_end, (uint32_t) i0, (uint32_t) std::min<uint64_t> (count, i0 + IP_CHUNK),
		               P, pThousandths, np, lo, hi, h_count, h_values, s);
	return rc;
	}

int gdsp_interval_percentiles (const double* d_v, uint32_t n, const uint32_t* h_start, const uint32_t* h_end, uint32_t count,
                               const uint32_t* pThousandths, int np, double lo, double hi,
                               uint32_t* h_count, double* h_values, void* stream)
	{
	gdsp_batch_item item;
	item.d_in = d_v;  item.d_out = NULL;  item.n = n;
	return gdsp_interval_percentiles_batch (&item, 1, NULL, h_start, h_end, count, pThousandths, np, lo, hi, h_count, h_values, stream);
	}

void gdsp_interval_percentiles_last (uint64_t out[6]) { memcpy (out, ipLast, sizeof(ipLast)); }

} // extern "C"
