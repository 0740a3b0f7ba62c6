// gdsp_segments.hip -- segments (not in the reference): the signal's own thresholded regions, each with statsover's exact
// figures: one counting read of the signal, then one pass that finds and reduces the runs (include/genodsp_hip.h).
//
// Device half.  A vector is cut into tiles of SG_TILE values of the 16-byte aligned frame it lies in, and every maximal
// stretch of members inside a tile becomes one record (a PIECE): where it lies and a gdsp_interval_piece for its finite
// members.  Two kernels:
//   sg_count_kernel   per tile, how many pieces it holds (the run starts in it): a streaming read, ballots and popcounts.
//                     The host reads the counts back (4 bytes per 32 KiB of signal), gives every tile that has pieces its
//                     place in the record array and cuts the tiles into launches whose records fit the bound.
//   sg_piece_kernel   a workgroup per tile THAT HAS PIECES (a work list: tiles without a member are not read again, so a
//                     sparse call -- a threshold at the 99th percentile -- reads the signal once and a few tiles twice).
//                     The tile comes into LDS with 16-byte non-temporal loads, lanes covering whole lines; thread t then
//                     owns the 16 consecutive values of strip t (pitch 17: conflict-free) and walks them once with a
//                     two-term TwoSum expansion (gdsp_xsum_dev.h: unchecked, a residual or an overflow sets `flag`), the
//                     count, the least value, and the greatest with its lowest position.  A stretch that closes inside
//                     the strip it began in is written at once; the stretch open at a strip's right edge goes through a
//                     segmented scan over the 256 strips (shuffles inside a wave, four records in LDS across waves), and
//                     the strip a stretch ends in -- or the tile's last strip -- writes it.  A record's place is the
//                     tile's base plus the number of run starts before it in the tile (an integer scan of popcounts),
//                     so the records are in position order whatever the dispatch order.
// No workgroup reads what another wrote, there is no atomic on global memory, and the counting pass and the piece pass
// evaluate the same predicate on the same values, so the counts are the pieces' places (a place beyond its tile's
// count is never written).
//
// The counts come from a pass of their own because a workgroup cannot know its place without them: fixed places of the
// worst case (SG_TILE / 2 records of 64 bytes per tile, four times the signal) would have to be compacted before they
// cross PCIe, and a look-back between workgroups reads what another wrote.  The counting pass runs at the speed of a
// read; with the work list the second read is of the tiles that hold members only.
//
// Host half (no GPU): gdsp_segments_feed joins touching pieces into runs and runs within mergeGap into segments, folds
// the pieces of a long segment as they come (into two TwoSum terms while that is exact, else into a 72-word integer
// image: its memory does not grow with the segment), applies the filters and hands the kept segments on, their figures
// from gdsp_interval_stats_combine.  A flagged piece is summed again by gdsp_xsum_accumulate_batch with that piece as its
// one source, as statsover does: adversarial data stays exact and gets slower.  That second sum, the arithmetic that folds
// pieces, the staging buffers and the timing events are gdsp_pieces.h's, shared with statsover and keepsegments.

#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "gdsp_common.h"
#include "gdsp_xsum_dev.h"
#include "gdsp_pieces.h"

#define SG_THREADS      256
#define SG_WAVES        (SG_THREADS / 64)
#define SG_STRIP        16                            // consecutive values a thread owns
#define SG_PITCH        (SG_STRIP + 1)                // LDS pitch of a strip
#define SG_TILE         (SG_THREADS * SG_STRIP)       // 4096 values: 34 KiB of LDS, four workgroups on a CU
#define SG_PAIRS        (SG_TILE / 2 / SG_THREADS)    // 16-byte words a thread stages
#define SG_TILE_PIECES  (SG_TILE / 2)                 // what one tile can hold: an alternating signal
#define SG_CHUNK_PIECES (1u << 21)                    // records of one launch (128 MiB)
#define SG_FOLD_PIECES  4096                          // pieces of an open segment the builder keeps before it folds them

static_assert (sizeof(gdsp_run_piece) == 64 && sizeof(gdsp_segment) == 64, "the records of the header");
static_assert (SG_STRIP == 16 && SG_PAIRS == 8, "16-bit strip masks, 8-bit pair masks");
static_assert (GDSP_BATCH_MAX == 32, "the work list keeps the vector in 5 bits above a 20-bit tile");

__device__ __forceinline__ bool sg_member (double x, double T, int ties) { return ties? (x >= T) : (x > T); }   // binarize's test

// tile `t` of the vector base[lead .. lead+n), as the 16-byte words SG_THREADS lanes cover together; a value outside
// the vector comes as NaN, which is no member
__device__ __forceinline__ void sg_load_tile (const double* __restrict__ base, uint32_t lead, uint32_t n, uint32_t t, double2 (&r)[SG_PAIRS])
	{
	const uint64_t f0 = (uint64_t) t * SG_TILE, end = (uint64_t) lead + n;
	if ((f0 >= lead) && (f0 + SG_TILE <= end))
		{
		const double2* src = reinterpret_cast<const double2*> (base + f0);
#pragma unroll
		for (int u=0 ; u<SG_PAIRS ; u++) r[u] = gdsp_ld2 (&src[u*SG_THREADS + threadIdx.x]);
		}
	else
		{
#pragma unroll
		for (int u=0 ; u<SG_PAIRS ; u++)
			{
			const uint64_t f = f0 + 2u * (u*SG_THREADS + threadIdx.x);
			r[u].x = ((f   >= lead) && (f   < end))? base[f]   : (double) NAN;
			r[u].y = ((f+1 >= lead) && (f+1 < end))? base[f+1] : (double) NAN;
			}
		}
	}

// counts[g] = the run starts in tile g of the table: members whose left neighbour in the tile is none
__global__ __launch_bounds__(SG_THREADS)
void sg_count_kernel (GdspBatch B, double T, int ties, uint32_t* __restrict__ counts)
	{
	__shared__ uint32_t lastY[SG_WAVES], wsum[SG_WAVES];
	const double* in;  double* unused;  uint32_t n;
	const uint32_t g    = gdsp_xcd_tile (blockIdx.x, B.tile0[GDSP_BATCH_MAX]);
	const uint32_t t    = gdsp_batch_tile (B, in, unused, n);
	const uint32_t lead = gdsp_aligned16 (in)? 0 : 1;
	double2 r[SG_PAIRS];
	sg_load_tile (in - lead, lead, n, t, r);

	// bit u: pair u*SG_THREADS + threadIdx.x
	uint32_t mx = 0, my = 0;
#pragma unroll
	for (int u=0 ; u<SG_PAIRS ; u++) { mx |= (sg_member (r[u].x, T, ties)? 1u : 0u) << u;  my |= (sg_member (r[u].y, T, ties)? 1u : 0u) << u; }
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	uint32_t before = __shfl_up (my, 1, 64);                   // the y of the pair before each of mine
	if (lane == 63) lastY[wave] = my;
	__syncthreads ();
	if (lane == 0) before = (wave > 0)? lastY[wave-1] : ((lastY[SG_WAVES-1] << 1) & 0xFFu);     // (nothing before the tile's first value)
	uint32_t starts = __popc (my & ~mx) + __popc (mx & ~before & 0xFFu);
	for (int off=32 ; off>0 ; off>>=1) starts += __shfl_down (starts, off, 64);
	if (lane == 0) wsum[wave] = starts;
	__syncthreads ();
	if (threadIdx.x == 0) counts[g] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
	}

// a stretch of members being reduced; positions are indices into the tile; start == UINT32_MAX: none
struct SgState { double a[XS_K], mn, mx;  uint32_t cnt, pos, flag, start; };

__device__ __forceinline__ void sg_clear (SgState& s)
	{
#pragma unroll
	for (int j=0 ; j<XS_K ; j++) s.a[j] = 0.0;
	s.mn = HUGE_VAL;  s.mx = -HUGE_VAL;  s.cnt = 0;  s.pos = UINT32_MAX;  s.flag = 0;  s.start = UINT32_MAX;
	}

// r = l ++ r when `take` (l lies left of r: of equal maxima l's position stays), else r as it is.  No branch.
__device__ __forceinline__ void sg_join (const SgState& l, SgState& r, bool take)
	{
#pragma unroll
	for (int j=0 ; j<XS_K ; j++) xs_grow_or_flag (r.a, take? l.a[j] : 0.0, r.flag);
	r.flag |= take? l.flag : 0u;
	r.cnt  += take? l.cnt : 0u;
	r.mn    = (take && (l.mn < r.mn))? l.mn : r.mn;
	const bool left = take && !(r.mx > l.mx);
	r.mx    = left? l.mx : r.mx;
	r.pos   = left? l.pos : r.pos;
	r.start = (take && (l.start < r.start))? l.start : r.start;
	}

__device__ __forceinline__ SgState sg_shfl_up (const SgState& s, int off)
	{
	SgState o;
#pragma unroll
	for (int j=0 ; j<XS_K ; j++) o.a[j] = __shfl_up (s.a[j], off, 64);
	o.mn  = __shfl_up (s.mn, off, 64);   o.mx  = __shfl_up (s.mx, off, 64);
	o.cnt = __shfl_up (s.cnt, off, 64);  o.pos = __shfl_up (s.pos, off, 64);
	o.flag = __shfl_up (s.flag, off, 64);  o.start = __shfl_up (s.start, off, 64);
	return o;
	}

// the stretch [s.start, end) of the tile whose first value is position pos0 of vector vec -> record `idx` of the tile's `cap`
__device__ __forceinline__ void sg_emit (gdsp_run_piece* __restrict__ out, uint32_t idx, uint32_t cap, uint32_t vec, uint32_t pos0,
                                         const SgState& s, uint32_t end)
	{
	if (idx >= cap) return;
	gdsp_run_piece r;
	r.vec = vec;  r.start = pos0 + s.start;  r.end = pos0 + end;  r.reserved = 0;
	r.piece.a0 = s.a[0];  r.piece.a1 = s.a[1];  r.piece.min = s.mn;  r.piece.max = s.mx;
	r.piece.count = s.cnt;  r.piece.maxpos = (s.cnt != 0)? pos0 + s.pos : UINT32_MAX;  r.piece.flag = s.flag;  r.piece.reserved = 0;
	out[idx] = r;
	}

// one launch's vectors: vector s is in[s][0 .. n[s]), 8-byte aligned
struct SgTable { const double* in[GDSP_BATCH_MAX];  uint32_t n[GDSP_BATCH_MAX]; };

// work[b] = { vector << 20 | tile of the vector, the tile's first record, its records, - }
__global__ __launch_bounds__(SG_THREADS)
void sg_piece_kernel (SgTable B, const uint4* __restrict__ work, double T, int ties, uint32_t vecBase, gdsp_run_piece* __restrict__ out)
	{
	__shared__ double   tile[SG_THREADS * SG_PITCH];
	__shared__ uint32_t masks[SG_THREADS], wcount[SG_WAVES], wopen[SG_WAVES];
	__shared__ SgState  wstate[SG_WAVES];
	const uint4    raw  = work[blockIdx.x];
	const uint32_t vt   = __builtin_amdgcn_readfirstlane (raw.x);
	const uint32_t base = __builtin_amdgcn_readfirstlane (raw.y);
	const uint32_t cap  = __builtin_amdgcn_readfirstlane (raw.z);
	const uint32_t vec  = vt >> 20, t = vt & 0xFFFFFu;
	const double*  in   = B.in[vec];
	const uint32_t lead = gdsp_aligned16 (in)? 0 : 1;
	const uint32_t pos0 = t * SG_TILE - lead;                  // the vector position of the tile's first value (tile 0 behind a lead: that value is no member)
	gdsp_run_piece* rec = out + base;

		{
		double2 r[SG_PAIRS];
		sg_load_tile (in - lead, lead, B.n[vec], t, r);
#pragma unroll
		for (int u=0 ; u<SG_PAIRS ; u++)
			{
			const uint32_t i = 2u * (u*SG_THREADS + threadIdx.x);
			tile[i + (i >> 4)] = r[u].x;  tile[i + (i >> 4) + 1] = r[u].y;
			}
		}
	__syncthreads ();

	const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i0 = tid * SG_STRIP;
	double   x[SG_STRIP];
	uint32_t m = 0;
#pragma unroll
	for (int j=0 ; j<SG_STRIP ; j++) { x[j] = tile[tid*SG_PITCH + j];  m |= (sg_member (x[j], T, ties)? 1u : 0u) << j; }
	masks[tid] = m;
	__syncthreads ();
	const bool entered = ((m & 1u) != 0) && (tid > 0) && ((masks[tid-1] >> (SG_STRIP-1)) != 0);      // my first value goes on a stretch of the strip before
	const bool goesOn  = ((m >> (SG_STRIP-1)) != 0) && (tid+1 < SG_THREADS) && ((masks[tid+1] & 1u) != 0);
	const bool through = (m == 0xFFFFu);

	// the run starts of the tile before my strip
	const uint32_t ns = __popc (m & ~((m << 1) | (entered? 1u : 0u)) & 0xFFFFu);
	uint32_t incl = ns;
	for (int off=1 ; off<64 ; off<<=1) { const uint32_t o = __shfl_up (incl, off, 64);  incl += (lane >= (uint32_t) off)? o : 0u; }
	if (lane == 63) wcount[wave] = incl;
	__syncthreads ();
	uint32_t excl = incl - ns;
	for (uint32_t w=0 ; w<wave ; w++) excl += wcount[w];

	// the strip: a stretch that began behind its first value and closes in it is written here; the one that began AT its
	// first value waits in `head` for what the strips before bring; the one open at the end stays in `acc`
	SgState  acc, head;
	uint32_t k = 0, headEnd = 0;
	bool     prev = false;
	sg_clear (acc);  sg_clear (head);
#pragma unroll
	for (int j=0 ; j<SG_STRIP ; j++)
		{
		const bool mem = ((m >> j) & 1u) != 0;
		if (!mem && prev)
			{
			if (acc.start == i0) { head = acc;  headEnd = i0 + j; }
			else                 sg_emit (rec, excl + k - 1, cap, vecBase + vec, pos0, acc, i0 + j);
			sg_clear (acc);
			}
		if (mem && !prev) { acc.start = i0 + j;  k += ((j > 0) || !entered)? 1u : 0u; }
		const bool in = mem && xs_finite (x[j]);               // the sample: finite members
		acc.cnt += in;
		xs_grow_or_flag (acc.a, in? x[j] : 0.0, acc.flag);
		acc.mn = (in && (x[j] < acc.mn))? x[j] : acc.mn;
		if (in && (x[j] > acc.mx)) { acc.mx = x[j];  acc.pos = i0 + j; }       // (ascending: the first of equals stays)
		prev = mem;
		}

	// open[t] = the stretch open at the right edge of strip t, with all of it that lies in the strips before: a strip of
	// members only goes on what its left neighbour has open, any other starts afresh
	bool fresh = !through;
	for (int off=1 ; off<64 ; off<<=1)
		{
		const SgState  l  = sg_shfl_up (acc, off);
		const uint32_t lf = __shfl_up (fresh? 1u : 0u, off, 64);
		const bool     on = (lane >= (uint32_t) off);
		sg_join (l, acc, on && !fresh);
		fresh = fresh || (on && (lf != 0));
		}
	if (lane == 63) { wstate[wave] = acc;  wopen[wave] = fresh? 0u : 1u; }
	__syncthreads ();
	SgState carry;                                             // what the last strip of the wave before has open
	sg_clear (carry);
	for (uint32_t w=0 ; w<wave ; w++)
		{
		SgState s = wstate[w];
		sg_join (carry, s, wopen[w] != 0);
		carry = s;
		}
	sg_join (carry, acc, !fresh);
	SgState before = sg_shfl_up (acc, 1);
	if (lane == 0) before = carry;

	if (((m & 1u) != 0) && !through)                           // the stretch that began at my first value closed in my strip
		{
		sg_join (before, head, entered);
		sg_emit (rec, excl + (entered? 0u : 1u) - 1, cap, vecBase + vec, pos0, head, headEnd);
		}
	if (((m >> (SG_STRIP-1)) != 0) && !goesOn)                 // the stretch open at my right edge ends there
		sg_emit (rec, excl + ns - 1, cap, vecBase + vec, pos0, acc, i0 + SG_STRIP);
	}

// ---------------------------------------------------------------------------------------------- host ----
// per device: staging and result buffers, grown on demand and kept
struct SgBuffers
	{
	GdspStaged<uint32_t> counts;
	GdspStaged<uint4>    work;
	GdspStaged<gdsp_run_piece> rec;
	GdspStaged<uint64_t> img;
	};
static SgBuffers sgBuffers[64];
static uint64_t  sgLast[4];
static double    sgTimes[4];

// records one launch may hold: SG_CHUNK_PIECES, or what GDSP_SEGMENTS_RECORDS says when that is less, never below what
// one tile can give.  Read at every call, so a test can make every tile its own launch.
static uint32_t sg_record_bound (void)
	{
	const char* e = getenv ("GDSP_SEGMENTS_RECORDS");
	if ((e == NULL) || (e[0] == 0)) return SG_CHUNK_PIECES;
	char* endp = NULL;
	const unsigned long long v = strtoull (e, &endp, 10);
	if ((endp == e) || (*endp != 0) || (v >= SG_CHUNK_PIECES)) return SG_CHUNK_PIECES;
	return (v < SG_TILE_PIECES)? SG_TILE_PIECES : (uint32_t) v;
	}

static int sg_feed_hook (void* ctx, const gdsp_run_piece* pieces, uint32_t count, const uint64_t* images);    // gdsp_segments_batch's consumer

// the `nwork` tiles of W.work.h, `P` records in all: reduce, read back, sum the flagged pieces again, hand them on
static int sg_launch (SgBuffers& W, const SgTable& B, const gdsp_batch_item* items, int vecBase, uint32_t nwork, uint32_t P,
                      double T, int tiesAbove, gdsp_run_pieces_fn emit, void* ctx, int dev, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1)
	{
	const GdspTimer tDev;
	int rc = W.rec.grow (P, "gdsp_run_pieces");
	if (rc != GDSP_OK) return rc;
	GDSP_HIP_TRY (hipMemcpyAsync (W.work.d, W.work.h, (size_t) nwork * sizeof(uint4), hipMemcpyHostToDevice, s));
	GDSP_HIP_TRY (hipEventRecord (ev0, s));
	hipLaunchKernelGGL (sg_piece_kernel, dim3(nwork), dim3(SG_THREADS), 0, s, B, W.work.d, T, tiesAbove, (uint32_t) vecBase, W.rec.d);
	GDSP_LAUNCH_CHECK ();
	GDSP_HIP_TRY (hipEventRecord (ev1, s));
	GDSP_HIP_TRY (hipMemcpyAsync (W.rec.h, W.rec.d, (size_t) P * sizeof(gdsp_run_piece), hipMemcpyDeviceToHost, s));
	GDSP_HIP_TRY (hipStreamSynchronize (s));
	float kernelMs = 0;
	GDSP_HIP_TRY (hipEventElapsedTime (&kernelMs, ev0, ev1));

	std::vector<uint32_t> flagged;
	std::vector<uint64_t> images;
	auto stretchOf = [&] (uint32_t p) { const gdsp_run_piece& r = W.rec.h[p];  return std::make_pair (items[r.vec].d_in + r.start, r.end - r.start); };
	rc = gdsp_flagged_images ("gdsp_run_pieces", P, [&] (uint32_t p) { return W.rec.h[p].piece.flag != 0; }, stretchOf, -DBL_MAX, DBL_MAX,
	                          W.img, dev, s, flagged, images);
	if (rc != GDSP_OK) return rc;
	sgTimes[1] += kernelMs;
	sgTimes[2] += tDev.ms () - kernelMs;

	const GdspTimer tEmit;
	const int stop = emit (ctx, W.rec.h, P, images.empty ()? NULL : images.data ());
	sgTimes[3] += tEmit.ms ();
	if (stop != 0)
		{
		if (emit != sg_feed_hook) gdsp_set_error ("gdsp_run_pieces_batch: the consumer of the pieces failed");     // (the builder has said why)
		return GDSP_EINVAL;
		}
	return GDSP_OK;
	}

// ------------------------------------------------------------------------------------------ host half ----
struct gdsp_segments_builder
	{
	uint32_t mergeGap, minLength;  int haveMinHeight;  double minHeight;
	gdsp_segments_fn emit;  void* ctx;
	bool     open;
	uint32_t vec, start, end;                              // the open segment
	std::vector<gdsp_interval_piece> pieces;               // its pieces, the older ones folded into the first
	std::vector<uint64_t> images;                          // one image per flagged piece of `pieces`, in order
	std::vector<gdsp_segment> kept;                        // of the feed in hand
	uint64_t counts[4];
	};

// the open segment's pieces into one: two TwoSum terms while that is exact, else an image
static void sg_fold (gdsp_segments_builder* b)
	{
	const GdspPiecesMerge m = gdsp_pieces_merge (b->pieces.data (), b->pieces.size ());
	gdsp_interval_piece f;
	memset (&f, 0, sizeof(f));
	f.count = (uint32_t) m.count;  f.min = m.min;  f.max = m.max;  f.maxpos = m.maxpos;
	double a[2];
	if (!m.anyFlag && gdsp_pieces_two_terms (b->pieces.data (), b->pieces.size (), a)) { f.a0 = a[0];  f.a1 = a[1];  b->images.clear (); }
	else
		{
		uint64_t img[GDSP_XSUM_WORDS];
		gdsp_pieces_image (b->pieces.data (), b->pieces.size (), b->images.data (), img);
		for (int w=GDSP_XSUM_DIGITS ; w<GDSP_XSUM_WORDS ; w++) img[w] = 0;
		f.flag = 1;
		b->images.assign (img, img + GDSP_XSUM_WORDS);
		}
	b->pieces.assign (1, f);
	}

// the open segment is complete: filter it, and keep it with its figures
static int sg_close (gdsp_segments_builder* b)
	{
	if (!b->open) return GDSP_OK;
	b->open = false;
	gdsp_segment g;
	memset (&g, 0, sizeof(g));
	g.vec = b->vec;  g.start = b->start;  g.end = b->end;
	bool keep = (g.end - g.start >= b->minLength);
	if (keep)
		{
		const int rc = gdsp_interval_stats_combine (b->pieces.data (), (uint32_t) b->pieces.size (), b->images.empty ()? NULL : b->images.data (), &g.stat);
		if (rc != GDSP_OK) return rc;
		if (b->haveMinHeight && ((g.stat.count == 0) || (g.stat.max < b->minHeight))) keep = false;
		}
	b->pieces.clear ();  b->images.clear ();
	if (keep) { b->kept.push_back (g);  b->counts[3]++; }
	return GDSP_OK;
	}

extern "C" {

uint32_t gdsp_segments_tile (void) { return SG_TILE; }

int gdsp_segments_create (gdsp_segments_builder** builder, uint32_t mergeGap, uint32_t minLength, int haveMinHeight,
                          double minHeight, gdsp_segments_fn emit, void* ctx)
	{
	GDSP_REQUIRE (builder != NULL, "NULL builder");
	GDSP_REQUIRE (emit != NULL, "NULL callback");
	GDSP_REQUIRE (!haveMinHeight || (minHeight == minHeight), "the minimum height is NaN");
	gdsp_segments_builder* b = new gdsp_segments_builder ();
	b->mergeGap = mergeGap;  b->minLength = minLength;  b->haveMinHeight = haveMinHeight;  b->minHeight = minHeight;
	b->emit = emit;  b->ctx = ctx;  b->open = false;  b->vec = b->start = b->end = 0;
	memset (b->counts, 0, sizeof(b->counts));
	*builder = b;
	return GDSP_OK;
	}

void gdsp_segments_destroy (gdsp_segments_builder* builder) { delete builder; }

void gdsp_segments_counts (const gdsp_segments_builder* builder, uint64_t out[4]) { memcpy (out, builder->counts, sizeof(builder->counts)); }

static int sg_hand_on (gdsp_segments_builder* b)
	{
	if (b->kept.empty ()) return GDSP_OK;
	const int stop = b->emit (b->ctx, b->kept.data (), (uint32_t) b->kept.size ());
	b->kept.clear ();
	if (stop != 0) { gdsp_set_error ("gdsp_segments: the consumer of the segments failed");  return GDSP_EINVAL; }
	return GDSP_OK;
	}

int gdsp_segments_feed (gdsp_segments_builder* b, const gdsp_run_piece* pieces, uint32_t count, const uint64_t* images)
	{
	GDSP_REQUIRE (b != NULL, "NULL builder");
	GDSP_REQUIRE ((count == 0) || (pieces != NULL), "NULL pieces");
	for (uint32_t k=0 ; k<count ; k++)
		{
		const gdsp_run_piece& r = pieces[k];
		GDSP_REQUIRE (r.start < r.end, "a piece must have start < end");
		GDSP_REQUIRE ((r.piece.flag == 0) || (images != NULL), "a flagged piece without its image");
		if (b->open)
			{
			GDSP_REQUIRE ((r.vec > b->vec) || ((r.vec == b->vec) && (r.start >= b->end)), "the pieces are not in (vector, position) order");
			if ((r.vec != b->vec) || (r.start - b->end > b->mergeGap))
				{
				const int rc = sg_close (b);
				if (rc != GDSP_OK) return rc;
				}
			}
		if (!b->open) { b->open = true;  b->vec = r.vec;  b->start = r.start;  b->counts[0]++; }
		else if (r.start != b->end) b->counts[0]++;            // (a piece that touches the one before goes on its run)
		b->end = r.end;
		b->counts[1]++;
		b->pieces.push_back (r.piece);
		if (r.piece.flag != 0)
			{
			b->counts[2]++;
			b->images.insert (b->images.end (), images, images + GDSP_XSUM_WORDS);
			images += GDSP_XSUM_WORDS;
			}
		if (b->pieces.size () >= SG_FOLD_PIECES) sg_fold (b);
		}
	return sg_hand_on (b);
	}

int gdsp_segments_finish (gdsp_segments_builder* b)
	{
	GDSP_REQUIRE (b != NULL, "NULL builder");
	const int rc = sg_close (b);
	if (rc != GDSP_OK) return rc;
	return sg_hand_on (b);
	}

int gdsp_run_pieces_batch (const gdsp_batch_item* items, int nitems, double T, int tiesAbove, gdsp_run_pieces_fn emit, void* ctx,
                           void* stream)
	{
	for (int k=0 ; k<4 ; k++) sgTimes[k] = 0;
	GDSP_REQUIRE (emit != NULL, "NULL callback");
	GDSP_REQUIRE (T == T, "the threshold is NaN");
	if (nitems <= 0) return GDSP_OK;
	GDSP_REQUIRE (items != NULL, "no vectors");
	for (int k=0 ; k<nitems ; k++)
		GDSP_REQUIRE ((items[k].n == 0) || ((items[k].d_in != NULL) && ((((uintptr_t) items[k].d_in) & 7) == 0)), "a vector must be 8-byte aligned");
	int dev = 0, rc = gdsp_device_slot (&dev);
	if (rc != GDSP_OK) return rc;
	SgBuffers& W = sgBuffers[dev];
	hipStream_t s = gdsp_stream (stream);
	const uint32_t bound = sg_record_bound ();
	GdspEventPair ev;
	rc = ev.create ("gdsp_run_pieces_batch");
	if (rc != GDSP_OK) return rc;

	for (int v0=0 ; v0<nitems ; v0+=GDSP_BATCH_MAX)                  // a table of vectors at a time
		{
		const int nvec = std::min (GDSP_BATCH_MAX, nitems - v0);
		GdspBatch C;
		SgTable   B;
		C.tile0[0] = 0;
		for (int k=0 ; k<GDSP_BATCH_MAX ; k++)
			{
			const bool     have = (k < nvec) && (items[v0+k].n != 0);
			const uint32_t lead = have? gdsp_frame_lead (items[v0+k].d_in) : 0;
			C.in[k]  = have? items[v0+k].d_in : NULL;  C.out[k] = NULL;  C.n[k] = have? items[v0+k].n : 0;
			B.in[k]  = C.in[k];  B.n[k] = C.n[k];
			C.tile0[k+1] = C.tile0[k] + (uint32_t) gdsp_frame_tiles (C.n[k], lead, SG_TILE);
			}
		C.nvec = (uint32_t) nvec;
		const uint32_t tiles = C.tile0[GDSP_BATCH_MAX];
		if (tiles == 0) continue;

		const GdspTimer tCount;
		rc = W.counts.grow (tiles, "gdsp_run_pieces");
		if (rc != GDSP_OK) return rc;
		hipLaunchKernelGGL (sg_count_kernel, dim3(tiles), dim3(SG_THREADS), 0, s, C, T, tiesAbove, W.counts.d);
		GDSP_LAUNCH_CHECK ();
		GDSP_HIP_TRY (hipMemcpyAsync (W.counts.h, W.counts.d, (size_t) tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
		GDSP_HIP_TRY (hipStreamSynchronize (s));
		sgTimes[0] += tCount.ms ();

		// the tiles that have pieces, in order, cut where a launch is full
		uint32_t nwork = 0, P = 0;
		int v = 0;
		for (uint32_t g=0 ; g<=tiles ; g++)
			{
			const uint32_t c = (g < tiles)? W.counts.h[g] : 0;
			if ((g < tiles) && (c == 0)) continue;
			GDSP_REQUIRE (c <= SG_TILE_PIECES, "a tile with more pieces than it can hold");
			if ((nwork != 0) && ((g == tiles) || (P + c > bound)))
				{
				rc = sg_launch (W, B, items, v0, nwork, P, T, tiesAbove, emit, ctx, dev, s, ev.ev0, ev.ev1);
				if (rc != GDSP_OK) return rc;
				nwork = 0;  P = 0;
				}
			if (g == tiles) break;
			while (C.tile0[v+1] <= g) v++;
			rc = W.work.grow ((size_t) nwork + 1, "gdsp_run_pieces", nwork, 1024);      // (between launches only: what is pending moves to the new buffer)
			if (rc != GDSP_OK) return rc;
			W.work.h[nwork++] = make_uint4 (((uint32_t) v << 20) | (g - C.tile0[v]), P, c, 0);
			P += c;
			}
		}
	return GDSP_OK;
	}

static int sg_feed_hook (void* ctx, const gdsp_run_piece* pieces, uint32_t count, const uint64_t* images)
	{ return gdsp_segments_feed ((gdsp_segments_builder*) ctx, pieces, count, images); }

int gdsp_segments_batch (const gdsp_batch_item* items, int nitems, double T, int tiesAbove, uint32_t mergeGap, uint32_t minLength,
                         int haveMinHeight, double minHeight, gdsp_segments_fn emit, void* ctx, void* stream)
	{
	memset (sgLast, 0, sizeof(sgLast));
	gdsp_segments_builder* b = NULL;
	int rc = gdsp_segments_create (&b, mergeGap, minLength, haveMinHeight, minHeight, emit, ctx);
	if (rc != GDSP_OK) return rc;
	rc = gdsp_run_pieces_batch (items, nitems, T, tiesAbove, sg_feed_hook, b, stream);
	if (rc == GDSP_OK) rc = gdsp_segments_finish (b);
	gdsp_segments_counts (b, sgLast);
	gdsp_segments_destroy (b);
	return rc;
	}

void gdsp_segments_last  (uint64_t out[4]) { memcpy (out, sgLast, sizeof(sgLast)); }
void gdsp_segments_times (double ms[4])    { memcpy (ms, sgTimes, sizeof(sgTimes)); }

} // extern "C"
