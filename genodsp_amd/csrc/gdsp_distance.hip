// gdsp_distance.hip -- distance: every base to the nearest base above a threshold (not in the reference).
//
// The definition is at gdsp_distance (include/genodsp_hip.h).  With S = {i : v[i] above T}, dilate asks "is a member of
// S within r of here" and erode "does S cover everything within r of here" (gdsp_morph.hip); this is the figure under
// both, for every r at once.  A distance has no bounded reach, so nothing can be answered from one tile and its halo.
// Three launches in stream order over every vector of a table (gdsp_common.h: GdspBatch), in place; the first two are
// gdsp_member_tile.h's, which fillgaps (gdsp_fillgaps.hip) runs with its own predicate and its own third launch:
//   1. bits   8 B/base read.  A workgroup turns its tile of the signal into membership bits -- lanes load 16 bytes each,
//              wave ballots gather the predicate, 128 bases become two 64-bit words, as gdsp_morph.hip stages them
//              (here a lane shuffle puts the predicates in base order before the ballot; interleaving the even and odd
//              ballots with scalar shifts, and the extents beside them, held this launch at 4.9 TB/s where it now reads
//              at 6.0) -- and writes them to workspace (1/8 B/base) with the tile's extent: its first and last member,
//              its first and last non-member.
//   2. join    one workgroup per vector scans the extents: every tile learns the last member and non-member before it
//              and the first of each behind it, across any number of tiles that have none.
//   3. write   1/8 B/base read, 8 B/base written.  A workgroup reads its tile's 128 words back, builds per word the
//              distance from the word's first bit to the member before it and from its last bit to the member behind it
//              (inside the tile by one scan over the words, beyond it from the join), the same for the complement when
//              the result is signed, and writes the doubles over the signal with 16-byte stores.
// The signal has been read completely when the first base is written, and no workgroup waits for another: there is no
// look-back and no flag to poll, so nothing here can hang on the order in which the hardware starts workgroups.
// Only predicates and integer distances are involved; the result is the definition's, bit for bit.
//
// Positions are uint32 (n <= 2^32-1, so a position is at most 2^32-2 and DT_NONE never is one); "last" figures travel
// as position + 1 with 0 for none, so that max joins them as min joins the "first" ones.

#include <stdlib.h>
#include "gdsp_common.h"
#include "gdsp_pieces.h"
#include "gdsp_member_tile.h"

#define DT_FAR          0x7FFFFFFF               // "no set bit in the words behind" inside a tile

// ---- launches 1 and 2: gdsp_member_tile.h, with segments' test as the predicate
__global__ __launch_bounds__(DT_THREADS)
void dt_bits_kernel (GdspBatch B, double T, int tiesAbove, unsigned long long* __restrict__ words, uint4* __restrict__ extent)
	{ dt_bits_tile (B, DtAbove { T, tiesAbove }, words, extent); }

__global__ __launch_bounds__(DT_JOIN_THREADS)
void dt_join_kernel (GdspBatch B, const uint4* __restrict__ extent, uint4* __restrict__ carry)
	{ dt_join_vector (B, extent, carry); }

// ---- launch 3.  Tables per mask word w of the tile, for the set (entries 0 .. DT_WORDS-1) and for its complement
// (DT_WORDS ..): before[w] = bases from the word's first bit back to the set bit before the word, behind[w] = bases
// from its last bit on to the set bit behind the word; DT_NONE where there is none.  The complement always has one:
// positions -1 and n are not in S.

// one base: bit b of word w, whose mask word is x
template <bool SIGNED, int TO>
__device__ __forceinline__ double dt_value (uint64_t x, int w, int b, const uint32_t* before, const uint32_t* behind,
                                            uint32_t none, uint32_t cap)
	{
	const bool     inside = SIGNED && (((x >> b) & 1) != 0);       // a member of a signed result: asks about the complement
	const uint64_t xs     = inside? ~x : x;
	const int      tw     = inside? DT_WORDS + w : w;
	uint32_t dl = DT_NONE, dr = DT_NONE;
	if (TO != GDSP_DISTANCE_RIGHT)
		{
		const uint64_t lower = xs << (63 - b);
		const uint32_t far   = before[tw];
		dl = (lower != 0)? (uint32_t) __builtin_clzll (lower) : ((far == DT_NONE)? DT_NONE : far + (uint32_t) b);
		}
	if (TO != GDSP_DISTANCE_LEFT)
		{
		const uint64_t upper = xs >> b;
		const uint32_t far   = behind[tw];
		dr = (upper != 0)? (uint32_t) __builtin_ctzll (upper) : ((far == DT_NONE)? DT_NONE : far + (uint32_t) (63 - b));
		}
	uint32_t d = min (dl, dr);
	if (d == DT_NONE) d = none;
	if ((cap != 0) && (d > cap)) d = cap;
	const double r = (double) d;
	return inside? -r : r;
	}

template <bool SIGNED, int TO>
__global__ __launch_bounds__(DT_THREADS)
void dt_write_kernel (GdspBatch B, const unsigned long long* __restrict__ words, const uint4* __restrict__ carry, uint32_t cap)
	{
	__shared__ uint64_t mask[DT_WORDS];
	__shared__ uint32_t before[2*DT_WORDS], behind[2*DT_WORDS];
	__shared__ int      partLast[DT_THREADS/64], partFirst[DT_THREADS/64];
	static_assert (DT_THREADS == 2*DT_WORDS, "one thread per word, for the set and for its complement");
	static_assert (DT_WORDS == 128, "each half of the workgroup is two waves");

	const double* unused;  double* out;  uint32_t n;
	const uint32_t t         = gdsp_batch_tile (B, unused, out, n);
	const uint32_t gt        = gdsp_xcd_tile (blockIdx.x, B.tile0[GDSP_BATCH_MAX]);
	const uint64_t tileStart = (uint64_t) t * DT_TILE;

	// threads 0..127 take the set's words, 128..255 the complement's; inside a tile one scan over the words, by lanes
	// and then over the two waves of a half
		{
		const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
		const int      comp = threadIdx.x >> 7, w = threadIdx.x & (DT_WORDS - 1);
		const uint64_t m = words[(size_t) gt * DT_WORDS + w];
		const uint64_t x = comp? ~m : m;
		if (comp == 0) mask[w] = m;
		int last  = (x != 0)? 64*w + 63 - __builtin_clzll (x) : -1;          // prefix max -> the last set bit up to this word
		int first = (x != 0)? 64*w + __builtin_ctzll (x) : DT_FAR;            // suffix min -> the first one from this word on
		for (int d=1 ; d<64 ; d*=2)
			{
			const int up = __shfl_up (last, d, 64), down = __shfl_down (first, d, 64);
			if (lane >= d)     last  = max (last, up);
			if (lane + d < 64) first = min (first, down);
			}
		if (lane == 63) partLast[wave]  = last;
		if (lane == 0)  partFirst[wave] = first;
		int prev = __shfl_up (last, 1, 64), next = __shfl_down (first, 1, 64);
		if (lane == 0)  prev = -1;
		if (lane == 63) next = DT_FAR;
		__syncthreads ();
		if ((wave & 1) == 1) prev = max (prev, partLast[wave - 1]);
		if ((wave & 1) == 0) next = min (next, partFirst[wave + 1]);

		const uint4    cr        = carry[gt];
		const uint32_t wordStart = (uint32_t) tileStart + 64u * (uint32_t) w;      // (words past the vector's end: nobody reads their entries)
		uint32_t bef, beh;
		if (comp == 0)
			{
			bef = (prev >= 0)?      (uint32_t) (64*w - prev)        : ((cr.y != 0)?       wordStart - (cr.y - 1)   : DT_NONE);
			beh = (next != DT_FAR)? (uint32_t) (next - (64*w + 63)) : ((cr.x != DT_NONE)? cr.x - (wordStart + 63u) : DT_NONE);
			}
		else
			{
			bef = (prev >= 0)?      (uint32_t) (64*w - prev)        : ((cr.w != 0)? wordStart - (cr.w - 1) : wordStart + 1u);
			beh = (next != DT_FAR)? (uint32_t) (next - (64*w + 63)) : (((cr.z != DT_NONE)? cr.z : n) - (wordStart + 63u));
			}
		if (SIGNED || (comp == 0)) { before[comp*DT_WORDS + w] = bef;  behind[comp*DT_WORDS + w] = beh; }
		}
	__syncthreads ();

	// two adjacent bases per lane, one 16-byte store; a base with nothing on the asked side gets the cap, or n without one
	const uint32_t none = (cap != 0)? cap : n;
	for (int q = threadIdx.x ; q < DT_TILE/2 ; q += DT_THREADS)
		{
		const uint64_t g = tileStart + 2*(uint64_t) q;
		if (g >= (uint64_t) n) break;
		const int      w = q >> 5, b = (2*q) & 63;
		const uint64_t x = mask[w];
		const double   r0 = dt_value<SIGNED, TO> (x, w, b,     before, behind, none, cap);
		const double   r1 = dt_value<SIGNED, TO> (x, w, b + 1, before, behind, none, cap);
		if (g + 1 < (uint64_t) n) gdsp_st2 (reinterpret_cast<double2*> (out + g), make_double2 (r0, r1));
		else                      out[g] = r0;
		}
	}

// ---------------------------------------------------------------------------------------------- host ----
// the workspace of launches 1 and 2, and how calls take it in turn: gdsp_member_tile.h
static double dtTimes[3];

// GDSP_DISTANCE_TIMES=1: the three launches are timed with events (profiles/distance.txt); the call then waits for them
static bool dt_timed (void)
	{
	static const bool value = [] () { const char* e = getenv ("GDSP_DISTANCE_TIMES");  return (e != NULL) && (e[0] == '1'); } ();
	return value;
	}

template <bool SIGNED>
static void dt_write_launch (const GdspBatch& B, uint32_t tiles, hipStream_t s, const unsigned long long* words, const uint4* carry,
                             int to, uint32_t cap)
	{
	if (to == GDSP_DISTANCE_LEFT)
		hipLaunchKernelGGL ((dt_write_kernel<SIGNED, GDSP_DISTANCE_LEFT>), dim3(tiles), dim3(DT_THREADS), 0, s, B, words, carry, cap);
	else if (to == GDSP_DISTANCE_RIGHT)
		hipLaunchKernelGGL ((dt_write_kernel<SIGNED, GDSP_DISTANCE_RIGHT>), dim3(tiles), dim3(DT_THREADS), 0, s, B, words, carry, cap);
	else
		hipLaunchKernelGGL ((dt_write_kernel<SIGNED, GDSP_DISTANCE_NEAREST>), dim3(tiles), dim3(DT_THREADS), 0, s, B, words, carry, cap);
	}

static int dt_run (const gdsp_batch_item* items, int nitems, double T, int tiesAbove, int to, int isSigned, uint32_t cap, void* stream)
	{
	GDSP_REQUIRE (T == T, "the threshold is NaN");
	GDSP_REQUIRE ((to == GDSP_DISTANCE_NEAREST) || (to == GDSP_DISTANCE_LEFT) || (to == GDSP_DISTANCE_RIGHT), "unknown side");
	int rc = gdsp_batch_check (items, nitems, true);
	if (rc != GDSP_OK) return rc;
	dtTimes[0] = dtTimes[1] = dtTimes[2] = 0;

	const uint64_t most = dt_most_tiles (items, nitems);
	if (most == 0) return GDSP_OK;
	hipStream_t s = gdsp_stream (stream);
	DtWork* W;  unsigned long long* words;  uint4 *extent, *carry;
	rc = dt_work_take (most, s, &W, &words, &extent, &carry);
	if (rc != GDSP_OK) return rc;
	const bool  timed = dt_timed ();
	hipEvent_t  ev[4] = { NULL, NULL, NULL, NULL };
	if (timed) { for (int k=0 ; k<4 ; k++) GDSP_HIP_TRY (hipEventCreate (&ev[k])); }
	hipError_t late = hipSuccess;
	gdsp_batch_run (items, nitems, dt_tiles,
		[&] (const GdspBatch& B, uint32_t tiles)
			{
			if (timed) (void) hipEventRecord (ev[0], s);
			hipLaunchKernelGGL (dt_bits_kernel, dim3(tiles), dim3(DT_THREADS), 0, s, B, T, tiesAbove, words, extent);
			if (timed) (void) hipEventRecord (ev[1], s);
			hipLaunchKernelGGL (dt_join_kernel, dim3(B.nvec), dim3(DT_JOIN_THREADS), 0, s, B, (const uint4*) extent, carry);
			if (timed) (void) hipEventRecord (ev[2], s);
			if (isSigned) dt_write_launch<true>  (B, tiles, s, words, carry, to, cap);
			else          dt_write_launch<false> (B, tiles, s, words, carry, to, cap);
			if (!timed) return;
			(void) hipEventRecord (ev[3], s);
			if (hipEventSynchronize (ev[3]) != hipSuccess) { late = hipErrorUnknown;  return; }
			for (int k=0 ; k<3 ; k++) { float ms = 0;  (void) hipEventElapsedTime (&ms, ev[k], ev[k+1]);  dtTimes[k] += ms; }
			});
	if (timed) { for (int k=0 ; k<4 ; k++) (void) hipEventDestroy (ev[k]); }
	GDSP_LAUNCH_CHECK ();
	GDSP_HIP_TRY (late);
	return dt_work_done (W, s);
	}

extern "C" {

uint32_t gdsp_distance_tile (void) { return DT_TILE; }

int gdsp_distance_batch (const gdsp_batch_item* items, int nitems, double T, int tiesAbove, int to, int isSigned, uint32_t cap,
                         void* stream)
	{ return dt_run (items, nitems, T, tiesAbove, to, isSigned, cap, stream); }

int gdsp_distance (double* d_v, uint32_t n, double T, int tiesAbove, int to, int isSigned, uint32_t cap, void* stream)
	{
	gdsp_batch_item item;
	item.d_in = NULL;  item.d_out = d_v;  item.n = n;
	return dt_run (&item, 1, T, tiesAbove, to, isSigned, cap, stream);
	}

void gdsp_distance_times (double ms[3]) { for (int k=0 ; k<3 ; k++) ms[k] = dtTimes[k]; }

} // extern "C"
