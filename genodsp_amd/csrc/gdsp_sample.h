// gdsp_sample.h -- the sample of the genome, as the kernels that only read it walk it (gdsp_xsum.hip: stats, normalize;
// gdsp_histogram.hip: histogram).  A source (gdsp_xsum_source, include/genodsp_hip.h) is d_v[0 .. n), 8-byte aligned, whose
// first value is base `first` of its chromosome.  Its sampled values are those whose chromosome position is a multiple
// of the window -- every window-th base counted from the chromosome's first, whatever stretch the source is.  Which of
// the sampled values count (min / max, finite values only) is each kernel's own test, next to its own arithmetic.
#pragma once

#include "gdsp_common.h"

// one launch's table (the batch convention of gdsp_common.h): source s is base[s][lead[s] .. lead[s]+n[s]), base 16-byte
// aligned (lead: the one value in front of a source that is not); its sampled values are those of index i >= phase[s]
// with (i - phase[s]) % window == 0 (phase: the first index whose chromosome position is a multiple of the window); it
// owns the tiles [tile0[s], tile0[s+1]) of the frame that starts at base
struct GdspSample
	{
	const double* base[GDSP_BATCH_MAX];
	uint32_t      n[GDSP_BATCH_MAX];
	uint32_t      lead[GDSP_BATCH_MAX];
	uint32_t      phase[GDSP_BATCH_MAX];
	uint32_t      tile0[GDSP_BATCH_MAX + 1];
	uint32_t      nvec;
	};

// host: the next launch's table from sources[*i ..], for tiles of tileValues values and at most maxTiles of them in a
// launch (one source may exceed that on its own); *i moves past what was taken or skipped (empty sources, and those
// with nothing sampled).  -> how many sources the table holds (0: none were left), or -1 for a source that is not
// 8-byte aligned.  taken (when given): which source each entry of the table is
static inline int gdsp_sample_next (GdspSample& B, const gdsp_xsum_source* sources, int nsources, int* i, uint32_t window,
                                    uint32_t tileValues, uint64_t maxTiles, int* taken = NULL)
	{
	int k = 0;
	B.tile0[0] = 0;
	for ( ; (*i<nsources) && (k<GDSP_BATCH_MAX) ; (*i)++)
		{
		const gdsp_xsum_source& src = sources[*i];
		if (src.n == 0) continue;
		if (!((src.d_v != NULL) && ((((uintptr_t) src.d_v) & 7) == 0))) return -1;
		const uint32_t lead  = gdsp_frame_lead (src.d_v);
		const uint32_t phase = (uint32_t) ((window - src.first % window) % window);
		if (phase >= src.n) continue;                                  // nothing of it is sampled
		const uint64_t t = (uint64_t) B.tile0[k] + gdsp_frame_tiles (src.n, lead, tileValues);
		if ((t > maxTiles) && (k > 0)) break;                          // the rest goes into the next launch
		if (taken != NULL) taken[k] = *i;
		B.base[k] = src.d_v - lead;  B.n[k] = src.n;  B.lead[k] = lead;  B.phase[k] = phase;
		B.tile0[++k] = (uint32_t) t;
		}
	for (int j=k ; j<GDSP_BATCH_MAX ; j++) { B.base[j] = NULL;  B.n[j] = 0;  B.lead[j] = 0;  B.phase[j] = 0;  B.tile0[j+1] = B.tile0[k]; }
	B.nvec = (uint32_t) k;
	return k;
	}

// device: tile g of the table, a frame of m values from base of which this tile starts at frame index j0
struct GdspSampleTile { const double* base;  uint32_t v, lead, phase;  uint64_t m, j0; };

// v: the source of the caller's previous tile (0 at first), t.v: this tile's; a workgroup's tiles ascend, so the search
// only moves on
template <uint32_t TILE>
__device__ __forceinline__ GdspSampleTile gdsp_sample_tile (const GdspSample& B, uint32_t g, uint32_t v)
	{
	while (B.tile0[v + 1] <= g) v++;
	GdspSampleTile t;
	t.v     = v;
	t.base  = B.base[v];
	t.lead  = B.lead[v];  t.phase = B.phase[v];
	t.m     = (uint64_t) B.n[v] + t.lead;                           // values of the frame
	t.j0    = (uint64_t) (g - B.tile0[v]) * TILE;
	return t;
	}

// is frame index j (source index j - lead) sampled?  WINDOWED: the window is above 1
template <bool WINDOWED>
__device__ __forceinline__ bool gdsp_sampled (const GdspSampleTile& t, uint32_t window, uint64_t j)
	{
	bool in = (j >= t.lead);
	if (WINDOWED)
		{
		const uint32_t i = (uint32_t) (j - t.lead);
		in = in && (i >= t.phase) && ((i - t.phase) % window == 0);
		}
	return in;
	}

// ---- the pair form (gdsp_xsum_pair.hip: correlate): two signals walked together ----
// A pair (gdsp_xsum_pair, include/genodsp_hip.h) is x = d_x[0 .. n) and y = d_y[0 .. n), both 8-byte aligned.  The table
// and the frame are x's: y[i] goes with x[i], at frame index i + lead.  ybase[s] is d_y - lead[s] (frame index 0; when
// lead is 1 that address is never read unless y shares x's alignment); bit s of `same` says that y is congruent to x
// modulo 16 bytes, so that ybase[s] is 16-byte aligned like base[s] and both streams take 16-byte loads.
struct GdspSamplePair
	{
	GdspSample    x;
	const double* ybase[GDSP_BATCH_MAX];
	uint32_t      same;
	};

// host: as gdsp_sample_next over the pairs' x (xs: the pairs as sources of their x, made once by the caller); -1 also for
// a y that is not 8-byte aligned
static inline int gdsp_sample_pair_next (GdspSamplePair& P, const gdsp_xsum_pair* pairs, const gdsp_xsum_source* xs, int npairs,
                                         int* i, uint32_t window, uint32_t tileValues, uint64_t maxTiles)
	{
	int taken[GDSP_BATCH_MAX];
	const int k = gdsp_sample_next (P.x, xs, npairs, i, window, tileValues, maxTiles, taken);
	P.same = 0;
	for (int j=0 ; j<GDSP_BATCH_MAX ; j++) P.ybase[j] = NULL;
	for (int j=0 ; j<k ; j++)
		{
		const double* y = pairs[taken[j]].d_y;
		if (!((y != NULL) && ((((uintptr_t) y) & 7) == 0))) return -1;
		P.ybase[j] = y - P.x.lead[j];
		if (gdsp_aligned16 (P.ybase[j])) P.same |= 1u << j;
		}
	return k;
	}

struct GdspSamplePairTile { GdspSampleTile x;  const double* ybase;  bool same; };

template <uint32_t TILE>
__device__ __forceinline__ GdspSamplePairTile gdsp_sample_pair_tile (const GdspSamplePair& P, uint32_t g, uint32_t v)
	{
	GdspSamplePairTile t;
	t.x     = gdsp_sample_tile<TILE> (P.x, g, v);
	t.ybase = P.ybase[t.x.v];
	t.same  = ((P.same >> t.x.v) & 1u) != 0;
	return t;
	}
