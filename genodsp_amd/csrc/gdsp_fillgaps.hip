// gdsp_fillgaps.hip -- fillgaps: the signal interpolated across its uncovered bases (not in the reference).
//
// The definition is at gdsp_fillgaps (include/genodsp_hip.h).  A base is known or it is not; a run of unknown bases takes
// its values from the known base before it and the known base behind it, however far away those are, so -- as for
// distance (gdsp_distance.hip) -- nothing can be answered from one tile and its halo.  Three launches in stream order over
// every vector of a table (gdsp_common.h: GdspBatch), in place; the first two are gdsp_member_tile.h's, which distance
// runs too, here with "known" as the predicate (segments' threshold test, or "neither zero nor NaN"):
//   1. bits    8 B/base read: the known bases as mask words, and every tile's extent.
//   2. join    per vector: every tile learns the last known base before it and the first one behind it.
//   3. write   A tile whose extent holds no unknown base returns at once: it reads its extent, 16 bytes, and nothing
//              else.  So does, after its carry, a tile without a known base that lies in a gap nobody fills (no known base
//              in the whole vector, or a gap longer than --maxgap: the carry gives its length).  Any other tile reads its
//              128 words back and finds per word the position of the known base before it and of the one behind it
//              (inside the tile by one scan over the words, beyond it from the join).  Then two adjacent bases per lane:
//              a pair without an unknown base is skipped; otherwise the lane finds l and r for each unknown base -- inside
//              the word from the mask, beyond it from the two tables --, reads v[l] and v[r] (a gather, but every base
//              of a gap asks for the same two addresses, and both are known bases) and, where something in the pair
//              changes, writes the pair with one 16-byte non-temporal store; a base of the pair that keeps its value
//              (a known one, or an unknown one that nobody fills) is read just before, for the store to put it back.
//              The tile itself is not read: only known values and the few kept ones are (a first form read every pair
//              with an unknown base whole, 16 B/base there, and took 10.9 ms where one base in 64 is known).
//              Traffic: nothing in tiles that are skipped; elsewhere the lines that hold known bases, at most 8 B/base,
//              and at most 8 B/base written.
// What is read after being written: launch 3 reads, from outside the pair a lane owns, the values of known bases only
// (v[l] and v[r], in this tile or in any other).  No launch changes a known base: a 16-byte store that covers a known
// base beside an unknown one writes the known base's own bits back, read in the same lane just before (so is an unknown
// base that stays as it is beside one that is filled: nobody else reads or writes it).  So no value is
// ever read after it was written with different contents, whichever workgroup runs first; and no workgroup waits for
// another: there is no look-back and no flag to poll.
// An index is dereferenced only where its side exists: DT_NONE never reaches an address.
// The arithmetic is a subtraction, a multiplication, a division and an addition, each rounded once (the library is built
// with -ffp-contract=off), and a clamp; the result is the definition's, bit for bit.

#include <stdlib.h>
#include "gdsp_common.h"
#include "gdsp_pieces.h"
#include "gdsp_member_tile.h"

#define FG_FAR 0x7FFFFFFF                        // "no set bit in the words behind" inside a tile

// ---- launches 1 and 2: gdsp_member_tile.h
template <bool NONZERO>
__global__ __launch_bounds__(DT_THREADS)
void fg_bits_kernel (GdspBatch B, double T, int tiesAbove, unsigned long long* __restrict__ words, uint4* __restrict__ extent)
	{
	if constexpr (NONZERO) dt_bits_tile (B, DtNonzero {}, words, extent);
	else                   dt_bits_tile (B, DtAbove { T, tiesAbove }, words, extent);
	}

__global__ __launch_bounds__(DT_JOIN_THREADS)
void fg_join_kernel (GdspBatch B, const uint4* __restrict__ extent, uint4* __restrict__ carry)
	{ dt_join_vector (B, extent, carry); }

// ---- launch 3

// between a = v[l] and b = v[r] (both known, so neither is a NaN), k of d bases on: every step rounded once
__device__ __forceinline__ double fg_linear (double a, double b, uint32_t k, uint32_t d)
	{
	if (a == b) return a;
	const double x  = a + ((b - a) * (double) k) / (double) d;
	const double lo = (a < b)? a : b, hi = (a < b)? b : a;
	return (x < lo)? lo : ((x > hi)? hi : x);                  // (a NaN from inf - inf passes)
	}

// one unknown base: position i of the vector, bit b (clear) of the tile's word w, whose mask word is x.  True: it takes
// `out`; false: it keeps its own value, which is not looked at here
template <int HOW>
__device__ __forceinline__ bool fg_value (const double* v, uint64_t x, int w, int b, uint32_t i, uint32_t n,
                                          const uint32_t* prevPos, const uint32_t* nextPos, bool extend, uint32_t maxgap,
                                          double& out)
	{
	const uint64_t lower = x << (63 - b), upper = x >> b;
	const uint32_t l     = (lower != 0)? i - (uint32_t) __builtin_clzll (lower) : prevPos[w];
	const uint32_t r     = (upper != 0)? i + (uint32_t) __builtin_ctzll (upper) : nextPos[w];
	const bool     haveL = (l != DT_NONE), haveR = (r != DT_NONE);
	if (!haveL && !haveR) return false;
	// the gap: from behind l, or from the vector's start, up to r, or to the vector's end
	const uint64_t from = haveL? (uint64_t) l + 1 : 0, to = haveR? (uint64_t) r : (uint64_t) n;
	if ((maxgap != 0) && (to - from > (uint64_t) maxgap)) return false;

	if ((HOW == GDSP_FILL_LINEAR) && haveL && haveR)
		{
		out = fg_linear (v[l], v[r], i - l, r - l);
		return true;
		}
	bool left;                                                  // the side the value comes from (it exists)
	if      (HOW == GDSP_FILL_LEFT)  left = haveL;
	else if (HOW == GDSP_FILL_RIGHT) left = !haveR;
	else                             left = haveL && (!haveR || ((HOW == GDSP_FILL_NEAREST) && (i - l <= r - i)));
	const bool wanted = (HOW == GDSP_FILL_LEFT)? haveL : ((HOW == GDSP_FILL_RIGHT)? haveR : (haveL && haveR));
	if (!wanted && !extend) return false;                       // the mode needs a side that does not exist
	out = v[left? l : r];
	return true;
	}

template <int HOW>
__global__ __launch_bounds__(DT_THREADS)
void fg_write_kernel (GdspBatch B, const unsigned long long* __restrict__ words, const uint4* __restrict__ extent,
                      const uint4* __restrict__ carry, int extend, uint32_t maxgap)
	{
	__shared__ uint64_t mask[DT_WORDS];
	__shared__ uint32_t prevPos[DT_WORDS], nextPos[DT_WORDS];  // per word: the known base before it / behind it, DT_NONE for none
	__shared__ int      partLast[2], partFirst[2];
	static_assert (DT_WORDS == 128, "the words of a tile are two waves' worth");
	static_assert (DT_THREADS >= DT_WORDS, "one thread per word");

	// (x, y: first known base of the tile, last + 1; z: its first unknown one.  carry x, y: the first known base behind
	// the tile, the last one before it + 1)
	const uint32_t gt = gdsp_xcd_tile (blockIdx.x, B.tile0[GDSP_BATCH_MAX]);
	const uint4    ex = extent[gt];
	if (ex.z == DT_NONE) return;                               // nothing unknown here (before the tile's vector is even looked up)

	const double* unused;  double* v;  uint32_t n;
	const uint32_t t         = gdsp_batch_tile (B, unused, v, n);
	const uint64_t tileStart = (uint64_t) t * DT_TILE;
	const uint4    cr        = carry[gt];
	if (ex.x == DT_NONE)                                       // nothing known here: the tile lies inside one gap
		{
		if ((cr.x == DT_NONE) && (cr.y == 0)) return;          // ... the whole vector does
		const uint64_t from = cr.y, to = (cr.x != DT_NONE)? (uint64_t) cr.x : (uint64_t) n;
		if ((maxgap != 0) && (to - from > (uint64_t) maxgap)) return;
		}

	// waves 0 and 1 take the words: one scan over them, by lanes and then over the two waves
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int w    = threadIdx.x & (DT_WORDS - 1);
	int prev = -1, next = FG_FAR;
	if (wave < 2)
		{
		const uint64_t m = words[(size_t) gt * DT_WORDS + w];
		mask[w] = m;
		int last  = (m != 0)? 64*w + 63 - __builtin_clzll (m) : -1;          // prefix max -> the last set bit up to this word
		int first = (m != 0)? 64*w + __builtin_ctzll (m) : FG_FAR;            // suffix min -> the first one from this word on
		for (int d=1 ; d<64 ; d*=2)
			{
			const int up = __shfl_up (last, d, 64), down = __shfl_down (first, d, 64);
			if (lane >= d)     last  = max (last, up);
			if (lane + d < 64) first = min (first, down);
			}
		if (lane == 63) partLast[wave]  = last;
		if (lane == 0)  partFirst[wave] = first;
		prev = __shfl_up (last, 1, 64);  next = __shfl_down (first, 1, 64);
		if (lane == 0)  prev = -1;
		if (lane == 63) next = FG_FAR;
		}
	__syncthreads ();
	if (wave < 2)
		{
		if (wave == 1) prev = max (prev, partLast[0]);
		if (wave == 0) next = min (next, partFirst[1]);
		prevPos[w] = (prev >= 0)?      (uint32_t) tileStart + (uint32_t) prev : ((cr.y != 0)? cr.y - 1 : DT_NONE);
		nextPos[w] = (next != FG_FAR)? (uint32_t) tileStart + (uint32_t) next : cr.x;
		}
	__syncthreads ();

	// two adjacent bases per lane
	for (int q = threadIdx.x ; q < DT_TILE/2 ; q += DT_THREADS)
		{
		const uint64_t g = tileStart + 2*(uint64_t) q;
		if (g >= (uint64_t) n) break;
		const int      ww = q >> 5, b = (2*q) & 63;
		const uint64_t x  = mask[ww];
		const int      known = (int) ((x >> b) & 3);
		if (known == 3) continue;
		const bool two = (g + 1 < (uint64_t) n);
		double2 cur;
		bool    f0 = false, f1 = false;
		if ((known & 1) == 0)
			f0 = fg_value<HOW> (v, x, ww, b,     (uint32_t) g,     n, prevPos, nextPos, extend != 0, maxgap, cur.x);
		if (two && ((known & 2) == 0))
			f1 = fg_value<HOW> (v, x, ww, b + 1, (uint32_t) g + 1, n, prevPos, nextPos, extend != 0, maxgap, cur.y);
		if (!f0 && !f1) continue;                              // nothing of the pair changes
		if (!f0)        cur.x = v[g];                          // a known base, or one that stays unknown: its own bits go back
		if (two && !f1) cur.y = v[g+1];
		if (two) gdsp_st2 (reinterpret_cast<double2*> (v + g), cur);
		else     v[g] = cur.x;
		}
	}

// ---------------------------------------------------------------------------------------------- host ----
// the workspace of launches 1 and 2, and how calls take it in turn: gdsp_member_tile.h
static double fgTimes[3];

// GDSP_FILLGAPS_TIMES=1: the three launches are timed with events (profiles/fillgaps.txt); the call then waits for them
static bool fg_timed (void)
	{
	static const bool value = [] () { const char* e = getenv ("GDSP_FILLGAPS_TIMES");  return (e != NULL) && (e[0] == '1'); } ();
	return value;
	}

static void fg_write_launch (const GdspBatch& B, uint32_t tiles, hipStream_t s, const unsigned long long* words, const uint4* extent,
                             const uint4* carry, int how, int extend, uint32_t maxgap)
	{
	if (how == GDSP_FILL_LINEAR)
		hipLaunchKernelGGL ((fg_write_kernel<GDSP_FILL_LINEAR>), dim3(tiles), dim3(DT_THREADS), 0, s, B, words, extent, carry, extend, maxgap);
	else if (how == GDSP_FILL_NEAREST)
		hipLaunchKernelGGL ((fg_write_kernel<GDSP_FILL_NEAREST>), dim3(tiles), dim3(DT_THREADS), 0, s, B, words, extent, carry, extend, maxgap);
	else if (how == GDSP_FILL_LEFT)
		hipLaunchKernelGGL ((fg_write_kernel<GDSP_FILL_LEFT>), dim3(tiles), dim3(DT_THREADS), 0, s, B, words, extent, carry, extend, maxgap);
	else
		hipLaunchKernelGGL ((fg_write_kernel<GDSP_FILL_RIGHT>), dim3(tiles), dim3(DT_THREADS), 0, s, B, words, extent, carry, extend, maxgap);
	}

static int fg_run (const gdsp_batch_item* items, int nitems, double T, int tiesAbove, int known, int how, int ends, uint32_t maxgap,
                   void* stream)
	{
	GDSP_REQUIRE ((known == GDSP_FILL_KNOWN_ABOVE) || (known == GDSP_FILL_KNOWN_NONZERO), "unknown test for known bases");
	GDSP_REQUIRE ((known == GDSP_FILL_KNOWN_NONZERO) || (T == T), "the threshold is NaN");
	GDSP_REQUIRE ((how == GDSP_FILL_LINEAR) || (how == GDSP_FILL_NEAREST) || (how == GDSP_FILL_LEFT) || (how == GDSP_FILL_RIGHT),
	              "unknown way to fill");
	GDSP_REQUIRE ((ends == GDSP_FILL_ENDS_EXTEND) || (ends == GDSP_FILL_ENDS_KEEP), "unknown treatment of the ends");
	int rc = gdsp_batch_check (items, nitems, true);
	if (rc != GDSP_OK) return rc;
	fgTimes[0] = fgTimes[1] = fgTimes[2] = 0;

	const uint64_t most = dt_most_tiles (items, nitems);
	if (most == 0) return GDSP_OK;
	hipStream_t s = gdsp_stream (stream);
	DtWork* W;  unsigned long long* words;  uint4 *extent, *carry;
	rc = dt_work_take (most, s, &W, &words, &extent, &carry);
	if (rc != GDSP_OK) return rc;
	const bool  timed  = fg_timed ();
	const int   extend = (ends == GDSP_FILL_ENDS_EXTEND);
	hipEvent_t  ev[4]  = { NULL, NULL, NULL, NULL };
	if (timed) { for (int k=0 ; k<4 ; k++) GDSP_HIP_TRY (hipEventCreate (&ev[k])); }
	hipError_t late = hipSuccess;
	gdsp_batch_run (items, nitems, dt_tiles,
		[&] (const GdspBatch& B, uint32_t tiles)
			{
			if (timed) (void) hipEventRecord (ev[0], s);
			if (known == GDSP_FILL_KNOWN_NONZERO)
				hipLaunchKernelGGL (fg_bits_kernel<true>,  dim3(tiles), dim3(DT_THREADS), 0, s, B, T, tiesAbove, words, extent);
			else
				hipLaunchKernelGGL (fg_bits_kernel<false>, dim3(tiles), dim3(DT_THREADS), 0, s, B, T, tiesAbove, words, extent);
			if (timed) (void) hipEventRecord (ev[1], s);
			hipLaunchKernelGGL (fg_join_kernel, dim3(B.nvec), dim3(DT_JOIN_THREADS), 0, s, B, (const uint4*) extent, carry);
			if (timed) (void) hipEventRecord (ev[2], s);
			fg_write_launch (B, tiles, s, words, extent, carry, how, extend, maxgap);
			if (!timed) return;
			(void) hipEventRecord (ev[3], s);
			if (hipEventSynchronize (ev[3]) != hipSuccess) { late = hipErrorUnknown;  return; }
			for (int k=0 ; k<3 ; k++) { float ms = 0;  (void) hipEventElapsedTime (&ms, ev[k], ev[k+1]);  fgTimes[k] += ms; }
			});
	if (timed) { for (int k=0 ; k<4 ; k++) (void) hipEventDestroy (ev[k]); }
	GDSP_LAUNCH_CHECK ();
	GDSP_HIP_TRY (late);
	return dt_work_done (W, s);
	}

extern "C" {

uint32_t gdsp_fillgaps_tile (void) { return DT_TILE; }

int gdsp_fillgaps_batch (const gdsp_batch_item* items, int nitems, double T, int tiesAbove, int known, int how, int ends,
                         uint32_t maxgap, void* stream)
	{ return fg_run (items, nitems, T, tiesAbove, known, how, ends, maxgap, stream); }

int gdsp_fillgaps (double* d_v, uint32_t n, double T, int tiesAbove, int known, int how, int ends, uint32_t maxgap, void* stream)
	{
	gdsp_batch_item item;
	item.d_in = NULL;  item.d_out = d_v;  item.n = n;
	return fg_run (&item, 1, T, tiesAbove, known, how, ends, maxgap, stream);
	}

void gdsp_fillgaps_times (double ms[3]) { for (int k=0 ; k<3 ; k++) ms[k] = fgTimes[k]; }

} // extern "C"
