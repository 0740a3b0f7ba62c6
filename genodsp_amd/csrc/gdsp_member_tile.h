// gdsp_member_tile.h -- what gdsp_distance.hip (distance) and gdsp_fillgaps.hip (fillgaps) build alike: a predicate over
// the bases of every vector of a table (gdsp_common.h: GdspBatch) as membership bits, each workgroup tile's extent, and
// the join that tells every tile where the nearest member and non-member lie beyond it, across any number of tiles that
// have none.  Two launches in stream order, whose bodies are here; each user wraps them in kernels of its own
// (dt_bits_tile takes the predicate as a functor) and follows them with its own third launch, which reads the words and
// the carries back.
//   1. bits    8 B/base read.  A workgroup turns its tile of the signal into membership bits -- lanes load 16 bytes each,
//              wave ballots gather the predicate, 128 bases become two 64-bit words, as gdsp_morph.hip stages them
//              (here a lane shuffle puts the predicates in base order before the ballot; interleaving the even and odd
//              ballots with scalar shifts, and the extents beside them, held this launch at 4.9 TB/s where it now reads
//              at 6.0) -- and writes them to workspace (1/8 B/base) with the tile's extent: its first and last member,
//              its first and last non-member.
//   2. join    one workgroup per vector scans the extents: every tile learns the last member and non-member before it
//              and the first of each behind it, across any number of tiles that have none.
// No workgroup waits for another in either: there is no look-back and no flag to poll.
//
// Positions are uint32 (n <= 2^32-1, so a position is at most 2^32-2 and DT_NONE never is one); "last" figures travel
// as position + 1 with 0 for none, so that max joins them as min joins the "first" ones.
//
// The host half: the workspace of the two launches, one per device for both users, and the event by which calls on several
// streams of a device take it in turn (dt_work_take, dt_work_done).
#pragma once

#include <algorithm>
#include "gdsp_common.h"
#include "gdsp_pieces.h"

#define DT_THREADS     256
#define DT_TILE         8192                     // bases per workgroup: 64 KiB read by launch 1, 64 KiB written by launch 3
#define DT_WORDS        (DT_TILE / 64)           // 128 mask words per tile
#define DT_CHUNKS       (DT_TILE / 128)          // wave-steps per tile
#define DT_UNROLL       8                        // 16-byte loads in flight per lane
#define DT_JOIN_THREADS 1024
#define DT_NONE         0xFFFFFFFFu

// the predicates.  segments' test: a NaN is never a member
struct DtAbove
	{
	double T;  int ties;
	__device__ __forceinline__ bool operator() (double x) const { return ties? (x >= T) : (x > T); }
	};
// anything but the two zeros and the NaNs
struct DtNonzero
	{
	__device__ __forceinline__ bool operator() (double x) const { return (x != 0) && (x == x); }
	};

// a tile's extent: x = first member, y = last member + 1, z = first non-member, w = last non-member + 1
struct DtExtent { uint32_t firstM, lastM1, firstN, lastN1; };

// the word of the bases [start, start+64): its members, and those of its clear bits that are bases of the vector
__device__ __forceinline__ void dt_extend (DtExtent& e, uint64_t word, uint64_t start, uint32_t n)
	{
	if (word != 0)
		{
		e.firstM = min (e.firstM, (uint32_t) (start + __builtin_ctzll (word)));
		e.lastM1 = max (e.lastM1, (uint32_t) (start + 64 - __builtin_clzll (word)));
		}
	if (start >= n) return;
	const uint64_t inside = (start + 64 <= n)? ~0ULL : ((1ULL << (n - start)) - 1);
	const uint64_t clear  = ~word & inside;
	if (clear != 0)
		{
		e.firstN = min (e.firstN, (uint32_t) (start + __builtin_ctzll (clear)));
		e.lastN1 = max (e.lastN1, (uint32_t) (start + 64 - __builtin_clzll (clear)));
		}
	}

// ---- launch 1 (DT_THREADS threads): tile `gt` of the table -> its DT_WORDS mask words (bits past the vector's end are
// clear) and its extent.  Tiles that lie wholly inside the vector load unconditionally (a predicated load gets its own
// branch and wait).
template <class Member>
__device__ __forceinline__ void dt_bits_tile (const GdspBatch& B, const Member member, unsigned long long* __restrict__ words,
                                              uint4* __restrict__ extent)
	{
	__shared__ DtExtent part[DT_THREADS/64];
	__shared__ uint64_t tileWords[DT_WORDS];
	const double* unused;  double* v;  uint32_t n;
	const uint32_t t         = gdsp_batch_tile (B, unused, v, n);
	const uint32_t gt        = gdsp_xcd_tile (blockIdx.x, B.tile0[GDSP_BATCH_MAX]);       // the tile's index in the table
	const uint64_t tileStart = (uint64_t) t * DT_TILE;
	const int      lane      = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const bool     interior  = (tileStart + DT_TILE <= (uint64_t) n);

	for (int c0 = wave*DT_UNROLL ; c0 < DT_CHUNKS ; c0 += (DT_THREADS/64)*DT_UNROLL)
		{
		double2 d[DT_UNROLL];
		bool    hx[DT_UNROLL], hy[DT_UNROLL];
		if (interior)
			{
#pragma unroll
			for (int u=0 ; u<DT_UNROLL ; u++)
				{
				d[u]  = gdsp_ld2 (reinterpret_cast<const double2*> (v + tileStart + 128*(c0+u) + 2*lane));
				hx[u] = hy[u] = true;
				}
			}
		else
			{
#pragma unroll
			for (int u=0 ; u<DT_UNROLL ; u++)
				{
				const uint64_t g = tileStart + 128*(c0+u) + 2*lane;
				hx[u] = (g < (uint64_t) n);
				hy[u] = (g + 1 < (uint64_t) n);
				d[u].x = hx[u]? v[g]   : 0.0;
				d[u].y = hy[u]? v[g+1] : 0.0;
				}
			}
#pragma unroll
		for (int u=0 ; u<DT_UNROLL ; u++)
			{
			// base k of the chunk's first 64 sits in lane k/2, of its last 64 in lane 32 + k/2: one shuffle each brings
			// its predicate to lane k, and the ballots are the two mask words (no bit interleave on the scalar unit)
			const int c      = c0 + u;
			const int packed = (int) (hx[u] && member (d[u].x)) | ((int) (hy[u] && member (d[u].y)) << 1);
			const int lower  = __shfl (packed, lane >> 1, 64), upper = __shfl (packed, 32 + (lane >> 1), 64);
			const uint64_t wA = __ballot (((lower >> (lane & 1)) & 1) != 0);
			const uint64_t wB = __ballot (((upper >> (lane & 1)) & 1) != 0);
			if (lane == 0) { tileWords[2*c] = wA;  tileWords[2*c+1] = wB; }
			}
		}
	__syncthreads ();

	// one thread per word: the word goes to the workspace, its set and clear bits into the tile's extent
	DtExtent e = { DT_NONE, 0, DT_NONE, 0 };
	if (threadIdx.x < DT_WORDS)
		{
		const uint64_t word = tileWords[threadIdx.x];
		words[(size_t) gt * DT_WORDS + threadIdx.x] = word;
		dt_extend (e, word, tileStart + 64*(uint64_t) threadIdx.x, n);
		}
	for (int off=32 ; off>0 ; off>>=1)
		{
		e.firstM = min (e.firstM, (uint32_t) __shfl_xor ((int) e.firstM, off, 64));
		e.lastM1 = max (e.lastM1, (uint32_t) __shfl_xor ((int) e.lastM1, off, 64));
		e.firstN = min (e.firstN, (uint32_t) __shfl_xor ((int) e.firstN, off, 64));
		e.lastN1 = max (e.lastN1, (uint32_t) __shfl_xor ((int) e.lastN1, off, 64));
		}
	if (lane == 0) part[wave] = e;
	__syncthreads ();
	if (threadIdx.x == 0)
		{
		for (int w=1 ; w<DT_THREADS/64 ; w++)
			{
			e.firstM = min (e.firstM, part[w].firstM);  e.lastM1 = max (e.lastM1, part[w].lastM1);
			e.firstN = min (e.firstN, part[w].firstN);  e.lastN1 = max (e.lastN1, part[w].lastN1);
			}
		extent[gt] = make_uint4 (e.firstM, e.lastM1, e.firstN, e.lastN1);
		}
	}

// ---- launch 2 (DT_JOIN_THREADS threads): workgroup s joins the extents of vector s (the scan never crosses into another
// vector's tiles).  carry[tile]: x = first member behind the tile, y = last member before it + 1, z and w the same for
// non-members; DT_NONE / 0 where the vector has none there.  Every thread owns a stretch of consecutive tiles.
__device__ __forceinline__ void dt_join_vector (const GdspBatch& B, const uint4* __restrict__ extent, uint4* __restrict__ carry)
	{
	__shared__ uint32_t a[4][DT_JOIN_THREADS];
	const uint32_t t0  = B.tile0[blockIdx.x], nt = B.tile0[blockIdx.x + 1] - t0;
	const uint32_t per = (nt + DT_JOIN_THREADS - 1) / DT_JOIN_THREADS;
	const uint32_t lo  = min (threadIdx.x * per, nt), hi = min (lo + per, nt);
	const int      me  = (int) threadIdx.x;
	uint32_t firstM = DT_NONE, lastM1 = 0, firstN = DT_NONE, lastN1 = 0;
	for (uint32_t b=lo ; b<hi ; b++)
		{
		const uint4 e = extent[t0 + b];
		firstM = min (firstM, e.x);  lastM1 = max (lastM1, e.y);  firstN = min (firstN, e.z);  lastN1 = max (lastN1, e.w);
		}
	a[0][me] = firstM;  a[1][me] = lastM1;  a[2][me] = firstN;  a[3][me] = lastN1;
	__syncthreads ();
	for (int d=1 ; d<DT_JOIN_THREADS ; d*=2)                   // min from the right for the firsts, max from the left for the lasts
		{
		const uint32_t fm = (me + d < DT_JOIN_THREADS)? a[0][me + d] : DT_NONE;
		const uint32_t lm = (me - d >= 0)?              a[1][me - d] : 0;
		const uint32_t fn = (me + d < DT_JOIN_THREADS)? a[2][me + d] : DT_NONE;
		const uint32_t ln = (me - d >= 0)?              a[3][me - d] : 0;
		__syncthreads ();
		a[0][me] = min (a[0][me], fm);  a[1][me] = max (a[1][me], lm);
		a[2][me] = min (a[2][me], fn);  a[3][me] = max (a[3][me], ln);
		__syncthreads ();
		}
	lastM1 = (me > 0)? a[1][me - 1] : 0;
	lastN1 = (me > 0)? a[3][me - 1] : 0;
	for (uint32_t b=lo ; b<hi ; b++)
		{
		const uint4 e = extent[t0 + b];
		carry[t0 + b].y = lastM1;  carry[t0 + b].w = lastN1;
		lastM1 = max (lastM1, e.y);  lastN1 = max (lastN1, e.w);
		}
	firstM = (me + 1 < DT_JOIN_THREADS)? a[0][me + 1] : DT_NONE;
	firstN = (me + 1 < DT_JOIN_THREADS)? a[2][me + 1] : DT_NONE;
	for (uint32_t b=hi ; b>lo ; b--)
		{
		const uint4 e = extent[t0 + b - 1];
		carry[t0 + b - 1].x = firstM;  carry[t0 + b - 1].z = firstN;
		firstM = min (firstM, e.x);  firstN = min (firstN, e.z);
		}
	}

// ---------------------------------------------------------------------------------------------- host ----
// per device: the mask words, extents and carries of one table of vectors; grown on demand and kept.  gdsp_malloc's
// (poisoned under GDSP_POISON): launch 1 writes every word and extent of every tile, launch 2 every carry, before
// anything is read.  Calls on one device share it, distance's and fillgaps' alike: each call's stream first waits for the
// event the call before it recorded behind its last launch (a dependency between streams that the runtime keeps; the host
// does not wait), so calls on several streams of a device -- the driver's shards of one GPU -- take the workspace in turn.
struct DtWork { void* d;  size_t cap;  hipEvent_t done; };
inline DtWork dtWork[64];
#define DT_TILE_BYTES ((size_t) DT_WORDS * 8 + 2 * sizeof(uint4))

static inline uint64_t dt_tiles (uint32_t n) { return ((uint64_t) n + DT_TILE - 1) / DT_TILE; }

// the largest table of a call decides the workspace (gdsp_batch_run: GDSP_BATCH_MAX vectors at a time); 0: nothing to do
static inline uint64_t dt_most_tiles (const gdsp_batch_item* items, int nitems)
	{
	uint64_t most = 0, sum = 0;
	int      k = 0;
	for (int i=0 ; i<nitems ; i++)
		{
		if (items[i].n == 0) continue;
		if (k == GDSP_BATCH_MAX) { k = 0;  sum = 0; }
		sum += dt_tiles (items[i].n);  k++;
		most = std::max (most, sum);
		}
	return most;
	}

// the current device's workspace for tables of up to `most` tiles, behind whatever call had it before on any stream
static inline int dt_work_take (uint64_t most, hipStream_t s, DtWork** work, unsigned long long** words, uint4** extent, uint4** carry)
	{
	int dev = 0;
	int rc = gdsp_device_slot (&dev);
	if (rc != GDSP_OK) return rc;
	DtWork& W = dtWork[dev];
	if (most * DT_TILE_BYTES > W.cap)
		{
		if (W.d != NULL) { (void) gdsp_free (W.d);  W.d = NULL;  W.cap = 0; }
		rc = gdsp_malloc (&W.d, most * DT_TILE_BYTES);
		if (rc != GDSP_OK) { W.d = NULL;  return rc; }
		W.cap = most * DT_TILE_BYTES;
		}
	*words  = (unsigned long long*) W.d;
	*extent = (uint4*) (*words + most * DT_WORDS);
	*carry  = *extent + most;
	if (W.done == NULL) GDSP_HIP_TRY (hipEventCreateWithFlags (&W.done, hipEventDisableTiming));
	else                GDSP_HIP_TRY (hipStreamWaitEvent (s, W.done, 0));
	*work = &W;
	return GDSP_OK;
	}

// behind the call's last launch
static inline int dt_work_done (DtWork* W, hipStream_t s)
	{
	GDSP_HIP_TRY (hipEventRecord (W->done, s));
	return GDSP_OK;
	}
