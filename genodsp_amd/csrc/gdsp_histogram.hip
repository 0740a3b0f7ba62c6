// gdsp_histogram.hip -- `histogram` (not in the reference): how many sampled values of the genome fall into each bin of
// an edge table e[0] < e[1] < ... < e[B], in one read of the signal (include/genodsp_hip.h has the definition).  The
// result is integer counts, so it is a function of the sample and the table alone: counts add as u64 words whatever
// the tiles, the grid, the dispatch order, the cut into vectors, the devices or the ranks.
//
// The pass (hist_kernel): one launch per table of up to 32 sources, a grid of resident workgroups walking 32 KiB tiles
// with 16-byte non-temporal loads, sampling by window / first and unaligned heads as gdsp_sample.h has them.  Inside a tile a
// WAVE owns 1024 consecutive values and takes them in eight steps of 128 (lane l holds values 2l and 2l+1 of the step),
// so that what a wave sees in one step, and from one step to the next, is a contiguous stretch of the chromosome.
//
// Slot of a value.  The device holds the table padded with two infinities on either side, P = {-inf, -inf, e[0] .. e[B],
// +inf, +inf}, and a sampled v has slot s in 0 .. B+1 iff P[s+1] <= v < P[s+2]: slot 0 is `below`, slot k+1 is bin k, slot
// B+1 is `above`; the comparisons against the table decide, nothing else.  A lane finds the slots of its 16 values of a
// tile together, without a branch, so that the 16 chains of table reads overlap:
//   uniform hint  the guess g = clamp (trunc ((v - e[0]) * B/(e[B] - e[0])), -1, B) + 1, one read of P[g .. g+3], and
//                 s = g - 1 + (v >= P[g+1]) + (v >= P[g+2]), right whenever P[g] <= v < P[g+3] -- a guess within one slot,
//                 which is what a uniform table gives; a lane with a value that fails that test searches its 16 values
//                 instead (the hint is a hint: any table gives the right words);
//   searched      a binary search of P with a fixed number of steps (pos += step while P[pos+step] <= v, the index
//                 clamped onto the +inf pad).
//
// Counting.  Coverage is piecewise constant (runs of ~150 bases, long stretches of exact zeros), so without care all 64
// lanes of every wave add to one counter.  What shares a destination is collapsed before it reaches a counter
// (-DHG_AGGREGATE=0|1|2 builds one level everywhere for the A/B in profiles/histogram.txt; by default the level is 2 where
// a slot has fewer than four LDS copies and on the large route, and 0 -- every lane adds for itself -- where it has four
// or more, B <= 1024: measured, 16 lanes of a wave on one LDS word cost nothing, all 64 on one word cost 3 x the pass):
//   1  a lane whose two values share a slot adds 2 once; the wave then compares every slot against its first lane's and
//      against its last lane's (two ballots each: a stretch with one run boundary holds exactly those two slots) and one
//      lane adds the popcounts; lanes that hold neither add for themselves;
//   2  also: a step whose 128 values share ONE slot adds nothing at all -- the wave carries (slot, count) in scalar
//      registers across steps and tiles and adds it when the slot changes and at the end.  An all-zero genome costs one
//      add per wave.
// The counters: B <= HG_LDS_BINS: workgroup-private u32 counters in LDS, `copies` of each slot (a power of two chosen so
// that the counters take about 16 KiB; copy c of slot s is word s*copies + c, so the copies of a slot lie in adjacent
// banks and lanes that add for themselves spread over them by lane number), next to the padded table, flushed once per
// workgroup to the device's u64 words with vector atomics.  B > HG_LDS_BINS (up to 65536: 256 KiB of counters do not fit):
// the same aggregation, then a workgroup-private cache of HG_CACHE (slot, u32 count) pairs in LDS, hashed by slot: the
// first slot to claim an entry (ds_cmpst on its tag) keeps it until the flush, a slot that finds its entry taken adds to
// the device's word with a u64 atomic.  Depth has a few dozen hot slots, which all find room; the table is read through
// the cache hierarchy.  A workgroup sees fewer than 2^32 values (hist_launch bounds the tiles of a launch), so no u32
// counter can wrap before its flush.

#include <float.h>
#include <math.h>
#include <string.h>
#include <vector>
#include <map>
#include <mutex>
#include <algorithm>
#include "gdsp_common.h"
#include "gdsp_sample.h"                                // the table of sources and which of their values are sampled

// aggregation level (see above): HG_AGGREGATE_SPREAD where a slot has four or more LDS copies, HG_AGGREGATE_HOT where
// it has fewer and on the large route; -DHG_AGGREGATE=<k> forces both (the A/B)
#ifdef HG_AGGREGATE
#define HG_AGGREGATE_SPREAD HG_AGGREGATE
#define HG_AGGREGATE_HOT    HG_AGGREGATE
#else
#define HG_AGGREGATE_SPREAD 0
#define HG_AGGREGATE_HOT    2
#endif
#define HG_THREADS    256
#define HG_UNROLL     8                               // 16-byte loads in flight per lane
#define HG_VALUES     (2 * HG_UNROLL)                 // values of a tile per lane
#define HG_TILE       (HG_THREADS * HG_VALUES)        // 4096 values = 32 KiB
#define HG_CUS        256
#define HG_LDS_BINS   4096                            // counters (and the table) in LDS up to here
#define HG_LDS_WORDS  4224                            // u32 counter words a workgroup may take: copies * (B + 2) <= this
#define HG_CACHE_LOG2 12
#define HG_CACHE      (1u << HG_CACHE_LOG2)           // entries of the large route's cache (32 KiB)
#define HG_MAX_BINS   65536
#define HG_NONE       0xFFFFFFFFu
#define HG_MAX_TILES  (1u << 28)                      // per launch; a full grid has at least 512 workgroups: 2^19 + 1 tiles, 2^31 values and a bit each

// d_pad: the padded table P (nbins + 5 values); topStep: the largest power of two <= nbins + 1 (the search's first step);
// lo, hi: the sample's limits with a NaN or an infinity replaced by -+DBL_MAX, so that lo <= v && v <= hi is the whole test
struct HgTable { const double* d_pad;  uint32_t nbins, copiesLog2, topStep;  double e0, inv, lo, hi; };

// the slots of N sampled values (an unsampled one arrives as e[0]); P is the padded table (LDS or global)
template <bool UNIFORM, int N, typename EdgePtr>
__device__ __forceinline__ void hg_slots (const double (&v)[N], uint32_t (&s)[N], EdgePtr P, const HgTable& T)
	{
	bool settled = UNIFORM;
	if (UNIFORM)
		{
		const double top = (double) T.nbins;
#pragma unroll
		for (int i=0 ; i<N ; i++)
			{
			const double   t = fmin (fmax ((v[i] - T.e0) * T.inv, -1.0), top);     // (a NaN becomes -1)
			const uint32_t g = (uint32_t) ((int) t + 1);                            // 0 .. B+1
			const double p0 = P[g], p1 = P[g + 1], p2 = P[g + 2], p3 = P[g + 3];
			s[i] = g - 1 + (v[i] >= p1) + (v[i] >= p2);
			settled = settled && (v[i] >= p0) && (v[i] < p3);
			}
		}
	if (!settled)
		{
		uint32_t pos[N];
#pragma unroll
		for (int i=0 ; i<N ; i++) pos[i] = 1;                                       // P[pos] <= v all along: P[1] = -inf
		for (uint32_t step=T.topStep ; step>0 ; step>>=1)
			{
#pragma unroll
			for (int i=0 ; i<N ; i++)
				{
				const uint32_t at = min (pos[i] + step, T.nbins + 3);                   // (P[B+3] = +inf: never taken)
				if (v[i] >= P[at]) pos[i] = at;
				}
			}
#pragma unroll
		for (int i=0 ; i<N ; i++) s[i] = pos[i] - 1;
		}
	}

// slot -> word of the result: bins first, then below, above
__device__ __forceinline__ uint32_t hg_word (uint32_t slot, uint32_t nbins) { return (slot == 0)? nbins : ((slot > nbins)? nbins + 1 : slot - 1); }

template <bool LDS> struct HgCounters;
template <> struct HgCounters<true>
	{
	uint32_t* cnt;  uint32_t shift, mask;
	__device__ __forceinline__ void add (uint32_t slot, uint32_t c, uint32_t copy) const
		{ if (slot != HG_NONE) atomicAdd (&cnt[(slot << shift) + (copy & mask)], c); }
	};
template <> struct HgCounters<false>
	{
	uint32_t* tag;  uint32_t* cnt;  unsigned long long* d;  uint32_t nbins;
	__device__ __forceinline__ void add (uint32_t slot, uint32_t c, uint32_t) const
		{
		if (slot == HG_NONE) return;
		const uint32_t h = (slot * 0x9E3779B1u) >> (32 - HG_CACHE_LOG2);
		uint32_t t = *(volatile uint32_t*) &tag[h];
		if (t == HG_NONE) { t = atomicCAS (&tag[h], HG_NONE, slot);  if (t == HG_NONE) t = slot; }
		if (t == slot) atomicAdd (&cnt[h], c);
		else           atomicAdd (&d[hg_word (slot, nbins)], (unsigned long long) c);
		}
	};

// LDS: counters and table in LDS; UNIFORM: guess first; WINDOWED: the window is above 1; AGG: aggregation level
template <bool LDS, bool UNIFORM, bool WINDOWED, int AGG>
__global__ __launch_bounds__(HG_THREADS)
void hist_kernel (GdspSample B, HgTable T, uint32_t window, unsigned long long* __restrict__ d_counts)
	{
	extern __shared__ double hg_lds[];         // LDS: nbins + 5 table values, then (nbins + 2) << copiesLog2 counters; or the cache
	const uint32_t nslots = T.nbins + 2;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	HgCounters<LDS> C;
	if constexpr (LDS)
		{
		uint32_t* cnt = reinterpret_cast<uint32_t*> (hg_lds + (T.nbins + 5));
		for (uint32_t i=threadIdx.x ; i<T.nbins+5 ; i+=HG_THREADS) hg_lds[i] = T.d_pad[i];
		for (uint32_t i=threadIdx.x ; i<(nslots << T.copiesLog2) ; i+=HG_THREADS) cnt[i] = 0;
		C.cnt = cnt;  C.shift = T.copiesLog2;  C.mask = (1u << T.copiesLog2) - 1;
		}
	else
		{
		C.tag = reinterpret_cast<uint32_t*> (hg_lds);  C.cnt = C.tag + HG_CACHE;  C.d = d_counts;  C.nbins = T.nbins;
		for (uint32_t i=threadIdx.x ; i<HG_CACHE ; i+=HG_THREADS) { C.tag[i] = HG_NONE;  C.cnt[i] = 0; }
		}
	__syncthreads ();

	uint32_t sampledHere = 0;                                  // this lane's sampled values (n)
	uint32_t pendSlot = HG_NONE, pendCount = 0;                // HG_AGGREGATE 2: the wave's run (the same in every lane)
	const uint32_t tiles = B.tile0[B.nvec];
	uint32_t v = 0;
	for (uint32_t g=blockIdx.x ; g<tiles ; g+=gridDim.x)
		{
		const GdspSampleTile t = gdsp_sample_tile<HG_TILE> (B, g, v);
		v = t.v;
		const double*  base = t.base;
		const uint64_t m = t.m, j0 = t.j0;
		auto wanted = [&] (double x, uint64_t j) -> bool               // stats' tests; NaN and +-inf never
			{ return (x >= T.lo) && (x <= T.hi) && gdsp_sampled<WINDOWED> (t, window, j); };
		if (j0 + HG_TILE <= m)
			{
			// the wave's 1024 values: step u is the 128 values from j0 + (wave*HG_UNROLL + u) * 128
			const double2* p = reinterpret_cast<const double2*> (base + j0) + wave * (HG_UNROLL * 64) + lane;
			double2 d[HG_UNROLL];
#pragma unroll
			for (int u=0 ; u<HG_UNROLL ; u++) d[u] = gdsp_ld2 (&p[u*64]);
			double   x[HG_VALUES];
			uint32_t k[HG_VALUES];
			uint32_t in = 0;
#pragma unroll
			for (int u=0 ; u<HG_UNROLL ; u++)
				{
				const uint64_t j = j0 + 2 * ((uint64_t) (wave * HG_UNROLL + u) * 64 + lane);
				const bool in0 = wanted (d[u].x, j), in1 = wanted (d[u].y, j + 1);
				in |= ((uint32_t) in0 << (2*u)) | ((uint32_t) in1 << (2*u + 1));
				x[2*u]     = in0? d[u].x : T.e0;
				x[2*u + 1] = in1? d[u].y : T.e0;
				}
			if constexpr (LDS) hg_slots<UNIFORM> (x, k, (const double*) hg_lds, T);
			else               hg_slots<UNIFORM> (x, k, T.d_pad, T);
			sampledHere += __popc (in);
#pragma unroll
			for (int u=0 ; u<HG_UNROLL ; u++)
				{
				const uint32_t k0 = ((in >> (2*u)) & 1)? k[2*u] : HG_NONE;
				const uint32_t k1 = ((in >> (2*u + 1)) & 1)? k[2*u + 1] : HG_NONE;
				if constexpr (AGG == 0)
					{
					C.add (k0, 1, lane);
					C.add (k1, 1, lane);
					continue;
					}
				const uint32_t kf = __builtin_amdgcn_readfirstlane (k0);
				const unsigned long long f0 = __ballot (k0 == kf), f1 = __ballot (k1 == kf);
				if ((AGG >= 2) && ((f0 & f1) == ~0ull))               // 128 values, one slot (or none sampled)
					{
					if (kf == pendSlot) pendCount += 128;
					else
						{
						if (lane == 0) C.add (pendSlot, pendCount, wave);
						pendSlot = kf;  pendCount = 128;
						}
					}
				else
					{
					const uint32_t kl = __builtin_amdgcn_readlane (k1, 63);
					const unsigned long long l0 = __ballot (k0 == kl), l1 = __ballot (k1 == kl);
					if (lane == 0)
						{
						C.add (kf, (uint32_t) (__popcll (f0) + __popcll (f1)), wave);
						if (kl != kf) C.add (kl, (uint32_t) (__popcll (l0) + __popcll (l1)), wave);
						}
					const bool own0 = (k0 != kf) && (k0 != kl), own1 = (k1 != kf) && (k1 != kl);
					if (own0 && own1 && (k0 == k1)) C.add (k0, 2, lane);
					else
						{
						if (own0) C.add (k0, 1, lane);
						if (own1) C.add (k1, 1, lane);
						}
					}
				}
			}
		else
			{
			for (uint64_t j = j0 + threadIdx.x ; j < m ; j += HG_THREADS)     // a source's last, partial tile
				{
				const double xj = base[j];
				const bool   in = wanted (xj, j);
				double   x1[1] = { in? xj : T.e0 };
				uint32_t k1[1];
				if constexpr (LDS) hg_slots<UNIFORM> (x1, k1, (const double*) hg_lds, T);
				else               hg_slots<UNIFORM> (x1, k1, T.d_pad, T);
				sampledHere += in;
				C.add (in? k1[0] : HG_NONE, 1, lane);
				}
			}
		}
	if ((AGG >= 2) && (lane == 0)) C.add (pendSlot, pendCount, wave);

	unsigned long long c = sampledHere;
	for (int off=32 ; off>0 ; off>>=1) c += __shfl_down (c, off, 64);
	if ((lane == 0) && (c != 0)) atomicAdd (&d_counts[nslots], c);
	__syncthreads ();
	if constexpr (LDS)
		{
		const uint32_t copies = 1u << T.copiesLog2;
		for (uint32_t s=threadIdx.x ; s<nslots ; s+=HG_THREADS)
			{
			unsigned long long sum = 0;
			for (uint32_t q=0 ; q<copies ; q++) sum += C.cnt[(s << T.copiesLog2) + q];
			if (sum != 0) atomicAdd (&d_counts[hg_word (s, T.nbins)], sum);
			}
		}
	else
		{
		for (uint32_t h=threadIdx.x ; h<HG_CACHE ; h+=HG_THREADS)
			{ if ((C.tag[h] != HG_NONE) && (C.cnt[h] != 0)) atomicAdd (&d_counts[hg_word (C.tag[h], T.nbins)], (unsigned long long) C.cnt[h]); }
		}
	}

// ------------------------------------------------------------------------------------------------ host ----
// is the table strictly increasing and finite?
static bool hg_table_ok (const double* e, uint32_t nbins)
	{
	if ((e == NULL) || (nbins < 1) || (nbins > HG_MAX_BINS)) return false;
	for (uint32_t k=0 ; k<=nbins ; k++)
		{
		if (!(fabs (e[k]) <= DBL_MAX)) return false;
		if ((k > 0) && !(e[k-1] < e[k])) return false;
		}
	return true;
	}

// the device copy of the padded table last used on each device (kept for the run: a caller that counts again and again
// with one table uploads it once).  A new table waits for whatever may still be reading the old one.
struct HgEdgeCache { double* d = NULL;  size_t cap = 0;  std::vector<double> host; };
static std::map<int, HgEdgeCache> hgEdges;
static std::mutex                 hgEdgesLock;

static int hg_device_table (const double* h_edges, uint32_t nbins, hipStream_t s, const double** d_pad)
	{
	int device = 0;
	GDSP_HIP_TRY (hipGetDevice (&device));
	std::lock_guard<std::mutex> hold (hgEdgesLock);
	HgEdgeCache& c = hgEdges[device];
	const size_t count = (size_t) nbins + 1;
	if ((c.host.size () != count) || (memcmp (c.host.data (), h_edges, count * sizeof(double)) != 0))
		{
		GDSP_HIP_TRY (hipDeviceSynchronize ());
		c.host.clear ();
		if (c.cap < count + 4)
			{
			if (c.d != NULL) (void) hipFree (c.d);
			c.d = NULL;  c.cap = 0;
			if (hipMalloc ((void**) &c.d, (count + 4) * sizeof(double)) != hipSuccess)
				{ c.d = NULL;  gdsp_set_error ("gdsp_histogram: no device memory for the edge table");  return GDSP_ENOMEM; }
			c.cap = count + 4;
			}
		std::vector<double> pad (count + 4);
		pad[0] = pad[1] = -HUGE_VAL;  pad[count + 2] = pad[count + 3] = HUGE_VAL;
		memcpy (&pad[2], h_edges, count * sizeof(double));
		GDSP_HIP_TRY (hipMemcpyAsync (c.d, pad.data (), (count + 4) * sizeof(double), hipMemcpyHostToDevice, s));
		GDSP_HIP_TRY (hipStreamSynchronize (s));
		c.host.assign (h_edges, h_edges + count);
		}
	*d_pad = c.d;
	return GDSP_OK;
	}

template <bool LDS, bool UNIFORM, int AGG>
static void hg_dispatch (bool windowed, uint32_t blocks, size_t lds, hipStream_t s, const GdspSample& B, const HgTable& T,
                         uint32_t window, unsigned long long* d_counts)
	{
	if (windowed) hipLaunchKernelGGL ((hist_kernel<LDS, UNIFORM, true, AGG>),  dim3(blocks), dim3(HG_THREADS), lds, s, B, T, window, d_counts);
	else          hipLaunchKernelGGL ((hist_kernel<LDS, UNIFORM, false, AGG>), dim3(blocks), dim3(HG_THREADS), lds, s, B, T, window, d_counts);
	}

static int hist_launch (const gdsp_xsum_source* sources, int nsources, uint32_t window, double lo, double hi,
                        const double* h_edges, uint32_t nbins, int uniform, uint64_t* d_counts, void* stream)
	{
	GDSP_REQUIRE (d_counts != NULL, "NULL counts");
	GDSP_REQUIRE ((nsources == 0) || (sources != NULL), "NULL sources");
	GDSP_REQUIRE (hg_table_ok (h_edges, nbins), "the edge table must hold 2 .. 65537 strictly increasing finite values");
	if (window == 0) window = 1;
	hipStream_t s = gdsp_stream (stream);

	HgTable T;
	T.nbins = nbins;  T.e0 = h_edges[0];
	T.inv = (double) nbins / (h_edges[nbins] - h_edges[0]);      // (inf - or 0 - when that overflows: only the first guess suffers)
	// !(v < lo) && !(v > hi) && v finite  <=>  lo' <= v && v <= hi' with a NaN limit (no limit) and an infinity pulled in
	T.lo = (lo >= -DBL_MAX)? lo : -DBL_MAX;
	T.hi = (hi <=  DBL_MAX)? hi :  DBL_MAX;
	T.topStep = 1;
	while (2 * (uint64_t) T.topStep <= (uint64_t) nbins + 1) T.topStep *= 2;
	const bool inLds = (nbins <= HG_LDS_BINS);
	T.copiesLog2 = 0;
	while (inLds && (T.copiesLog2 < 4) && (((uint64_t) (nbins + 2) << (T.copiesLog2 + 1)) <= HG_LDS_WORDS)) T.copiesLog2++;
	const size_t lds = inLds? ((size_t) (nbins + 5) * sizeof(double) + (((size_t) (nbins + 2) << T.copiesLog2) * sizeof(uint32_t)))
	                        : (size_t) HG_CACHE * 2 * sizeof(uint32_t);
	// every workgroup resident, so that equal shares finish together: 160 KiB of LDS per CU, at most 4 workgroups on each
	const uint32_t perCu = (uint32_t) std::min<size_t> (4, (160 * 1024) / (lds + 1024));
	const uint32_t maxBlocks = HG_CUS * perCu;
	T.d_pad = NULL;

	int i = 0;
	while (i < nsources)
		{
		GdspSample B;
		const int k = gdsp_sample_next (B, sources, nsources, &i, window, HG_TILE, HG_MAX_TILES);
		GDSP_REQUIRE (k >= 0, "a source must be 8-byte aligned");
		if (k == 0) continue;
		if (T.d_pad == NULL)
			{
			int rc = hg_device_table (h_edges, nbins, s, &T.d_pad);
			if (rc != GDSP_OK) return rc;
			}
		const uint32_t tiles  = B.tile0[k];
		const uint32_t blocks = (tiles < maxBlocks)? tiles : maxBlocks;
		unsigned long long* acc = reinterpret_cast<unsigned long long*> (d_counts);
		const bool windowed = (window != 1);
		// measured (profiles/histogram.txt): with 16 lanes or fewer of a wave on one LDS word the unaggregated adds cost
		// nothing and the aggregation's ballots do; with all 64 on one word (one copy) they cost 3 x the pass
		if (inLds && (T.copiesLog2 >= 2))
			{
			if (uniform) hg_dispatch<true,  true,  HG_AGGREGATE_SPREAD> (windowed, blocks, lds, s, B, T, window, acc);
			else         hg_dispatch<true,  false, HG_AGGREGATE_SPREAD> (windowed, blocks, lds, s, B, T, window, acc);
			}
		else if (inLds)
			{
			if (uniform) hg_dispatch<true,  true,  HG_AGGREGATE_HOT> (windowed, blocks, lds, s, B, T, window, acc);
			else         hg_dispatch<true,  false, HG_AGGREGATE_HOT> (windowed, blocks, lds, s, B, T, window, acc);
			}
		else
			{
			if (uniform) hg_dispatch<false, true,  HG_AGGREGATE_HOT> (windowed, blocks, lds, s, B, T, window, acc);
			else         hg_dispatch<false, false, HG_AGGREGATE_HOT> (windowed, blocks, lds, s, B, T, window, acc);
			}
		GDSP_LAUNCH_CHECK ();
		}
	return GDSP_OK;
	}

extern "C" {

int gdsp_histogram_uniform_edges (double lo, double width, uint32_t nbins, double* h_edges)
	{
	GDSP_REQUIRE (h_edges != NULL, "NULL edges");
	GDSP_REQUIRE ((nbins >= 1) && (nbins <= HG_MAX_BINS), "1 .. 65536 bins");
	for (uint32_t k=0 ; k<=nbins ; k++) h_edges[k] = fma ((double) k, width, lo);       // each edge rounded once
	GDSP_REQUIRE (hg_table_ok (h_edges, nbins), "lo + k*width is not strictly increasing and finite over the bins");
	return GDSP_OK;
	}

int gdsp_histogram_init (uint64_t* d_counts, uint32_t nbins, void* stream)
	{
	GDSP_REQUIRE (d_counts != NULL, "NULL counts");
	GDSP_REQUIRE ((nbins >= 1) && (nbins <= HG_MAX_BINS), "1 .. 65536 bins");
	GDSP_HIP_TRY (hipMemsetAsync (d_counts, 0, ((size_t) nbins + 3) * sizeof(uint64_t), gdsp_stream (stream)));
	return GDSP_OK;
	}

int gdsp_histogram_accumulate_batch (const gdsp_xsum_source* sources, int nsources, uint32_t window, double lo, double hi,
                                     const double* h_edges, uint32_t nbins, int uniform, uint64_t* d_counts, void* stream)
	{ return hist_launch (sources, nsources, window, lo, hi, h_edges, nbins, uniform, d_counts, stream); }

} // extern "C"

// ------------------------------------------------------------------------------------------- end to end ----
static gdsp_comm* hgComm = NULL;                             // see gdsp_genome_histogram_use_comm

extern "C" {

int gdsp_genome_histogram_use_comm (gdsp_comm* comm) { hgComm = comm;  return GDSP_OK; }

int gdsp_genome_histogram (const gdsp_xsum_source* sources, int nsources, uint32_t window, double lo, double hi,
                           const double* h_edges, uint32_t nbins, int uniform,
                           gdsp_reduce_fn reduce, void* reduceCtx, uint64_t* h_counts)
	{
	GDSP_REQUIRE (h_counts != NULL, "NULL result");
	GDSP_REQUIRE ((nsources == 0) || (sources != NULL), "NULL sources");
	GDSP_REQUIRE (hg_table_ok (h_edges, nbins), "the edge table must hold 2 .. 65537 strictly increasing finite values");
	GDSP_REQUIRE (!((hgComm != NULL) && (reduce != NULL)), "a host reduction hook next to a communicator");
	auto onDevice = [&] (const gdsp_xsum_source* mine, int nmine, uint64_t* d_counts, void* stream) -> int
		{
		int rc = gdsp_histogram_init (d_counts, nbins, stream);
		if (rc == GDSP_OK) rc = hist_launch (mine, nmine, window, lo, hi, h_edges, nbins, uniform, d_counts, stream);
		return rc;
		};
	return gdsp_reduce_sources ("gdsp_genome_histogram", "counts", hgComm, sources, nsources, (size_t) nbins + 3, onDevice,
	                            reduce, reduceCtx, h_counts);
	}

} // extern "C"
