// gdsp_intervalstats.hip -- statsover (not in the reference): count, exact sum and mean, min, max and summit of one
// signal over millions of arbitrary intervals -- short and long, overlapping, in any order (include/genodsp_hip.h).
//
// Work is cut into PIECES: an interval intersected with a tile of IS_TILE values of the 16-byte aligned frame its vector
// lies in.  The host sorts the pieces of a call by tile (a counting sort, the caller's order kept inside a tile) and cuts
// every tile's list into ITEMS of at most IC_ITEM_PIECES pieces; a workgroup takes one item, so one 249 Mbp interval and
// a million intervals inside one tile both fill the device, and a tile no interval touches is never read.  The workgroup
// brings the part of the tile its pieces cover into LDS with 16-byte loads, and its four waves take the pieces in turn:
// a lane walks its piece with stride 64, keeps two 2-term TwoSum expansions (gdsp_xsum_dev.h: unchecked, a residual or
// an overflow sets `flag`), the count, the least value, and the greatest value with its lowest position; a shuffle tree
// folds the lanes and lane 0 writes the piece's record.  A workgroup reads the signal and writes its own records: there
// is no atomic, no workgroup reads what another wrote, and nothing depends on the dispatch order.
//
// The host then combines an interval's pieces exactly (gdsp_interval_stats_combine, no GPU): the terms of unflagged
// pieces are added with TwoSum into two terms; when nothing is left over and their sum is one double, that double is the
// sum and one IEEE division gives the mean (always so on integer read depth); when two doubles s + e hold it, s is the
// sum and a 128-bit division gives the mean.  Otherwise the terms go into a 72-word
// integer image (gdsp_xsum_add_host) and gdsp_xsum_round / gdsp_xsum_div_round round it once.  A flagged piece (huge
// cancelling values, residuals across hundreds of binades) is summed again by gdsp_xsum_accumulate_batch with that piece
// as its one source: adversarial data stays exact and gets slower.
//
// The staging buffers, the timing events, that second sum and the arithmetic on pieces are gdsp_pieces.h's, shared with
// segments and keepsegments; the cut into pieces and items, the staging of an item's hull and everything a call and a
// launch do around the kernel (ic_run) are gdsp_interval_cut.h's, shared with breadthover: this file keeps the kernel, its
// start, the flagged pieces' second sum and the combine.

#include <float.h>
#include <math.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "gdsp_common.h"
#include "gdsp_xsum_dev.h"
#include "gdsp_pieces.h"
#include "gdsp_interval_cut.h"

#define IS_THREADS      IC_THREADS
#define IS_WAVES        IC_WAVES
#define IS_TILE         IC_TILE                       // (a launch's IC_LAUNCH_PIECES records: 192 MiB)

static_assert (sizeof(gdsp_interval_piece) == 48 && sizeof(gdsp_interval_stat) == 48, "the records of the header");

__global__ __launch_bounds__(IS_THREADS)
void interval_stats_kernel (IcBatch B, const uint4* __restrict__ items, const uint32_t* __restrict__ pieces, double lo, double hi,
                            gdsp_interval_piece* __restrict__ out)
	{
	__shared__ double tile[IS_TILE];
	uint32_t first, count, pos0;
	ic_stage_item (B, items, tile, first, count, pos0);

	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	for (uint32_t k=wave ; k<count ; k+=IS_WAVES)
		{
		const uint32_t d = __builtin_amdgcn_readfirstlane (pieces[first + k]);
		const uint32_t a = d & 0xFFFF, b = (d >> 16) + 1;
		double   ax[XS_K], ay[XS_K], mn = HUGE_VAL, mx = -HUGE_VAL;
		uint32_t cnt = 0, flag = 0, pos = UINT32_MAX;
#pragma unroll
		for (int j=0 ; j<XS_K ; j++) { ax[j] = 0.0;  ay[j] = 0.0; }
		auto take = [&] (double (&acc)[XS_K], uint32_t i)
			{
			const double x  = tile[i];
			const bool   in = !(x < lo) && !(x > hi) && xs_finite (x);    // stats' tests; NaN and +-inf never
			cnt += in;
			xs_grow_or_flag (acc, in? x : 0.0, flag);
			mn = (in && (x < mn))? x : mn;
			if (in && (x > mx)) { mx = x;  pos = i; }                   // (i ascends: the first of equals stays)
			};
		uint32_t i = a + lane;
		for ( ; i+64<b ; i+=128) { take (ax, i);  take (ay, i+64); }
		if (i < b) take (ax, i);

		// the lane's two expansions, then the wave's 64 as a tree: lane l takes lane l+off's terms when l % 2off == 0
#pragma unroll
		for (int j=0 ; j<XS_K ; j++) xs_grow_or_flag (ax, ay[j], flag);
		for (int off=1 ; off<64 ; off<<=1)
			{
			double tt[XS_K];
#pragma unroll
			for (int j=0 ; j<XS_K ; j++) tt[j] = __shfl_down (ax[j], off, 64);
			const bool mine = (lane & (2*off - 1)) == 0;
#pragma unroll
			for (int j=0 ; j<XS_K ; j++) xs_grow_or_flag (ax, mine? tt[j] : 0.0, flag);
			}
		for (int off=32 ; off>0 ; off>>=1)
			{
			cnt  += __shfl_down (cnt, off, 64);
			flag |= __shfl_down (flag, off, 64);
			const double   omn = __shfl_down (mn, off, 64), omx = __shfl_down (mx, off, 64);
			const uint32_t opos = __shfl_down (pos, off, 64);
			mn = (omn < mn)? omn : mn;
			if ((omx > mx) || ((omx == mx) && (opos < pos))) { mx = omx;  pos = opos; }
			}
		if (lane == 0)
			{
			gdsp_interval_piece r;
			r.a0 = ax[0];  r.a1 = ax[1];  r.min = mn;  r.max = mx;
			r.count = cnt;  r.maxpos = (cnt != 0)? pos0 + pos : UINT32_MAX;  r.flag = flag;  r.reserved = 0;
			out[first + k] = r;
			}
		}
	}

// ---------------------------------------------------------------------------------------------- host ----
// per device: the launch's buffers (gdsp_interval_cut.h) and the staging of the flagged pieces' second sum
struct IsBuffers : IcBuffers<gdsp_interval_piece> { GdspStaged<uint64_t> img; };
static IsBuffers isBuffers[64];
static IcReport  isReport;                            // last: intervals, pieces, flagged pieces, intervals rounded from the image

// behind the records: each flagged piece is summed again as the one source of an exact pass
static int is_flagged (IsBuffers& W, const IcLaunch& L, double lo, double hi, std::vector<uint32_t>& flagged, std::vector<uint64_t>& images)
	{
	auto stretchOf = [&] (uint32_t p)
		{
		const uint32_t g = (uint32_t) (std::upper_bound (L.cut.tileFirst.begin (), L.cut.tileFirst.end (), p) - L.cut.tileFirst.begin ()) - 1;
		int v = 0;
		while ((v+1 < L.nvec) && (L.vecs[v+1].tile0 <= g)) v++;
		const uint32_t a = W.pieces.h[p] & 0xFFFF, b = (W.pieces.h[p] >> 16) + 1;
		return std::make_pair (L.B.base[v] + (uint64_t) (g - L.vecs[v].tile0) * IS_TILE + a, b - a);
		};
	return gdsp_flagged_images ("gdsp_interval_stats", L.cut.P, [&] (uint32_t p) { return W.out.h[p].flag != 0; }, stretchOf, lo, hi,
	                            W.img, L.dev, L.s, flagged, images);
	}

// the figures of the launch's intervals from their pieces' records
static int is_combine (IsBuffers& W, const IcLaunch& L, const std::vector<uint32_t>& flagged, const std::vector<uint64_t>& images,
                       gdsp_interval_stat* h_out)
	{
	const std::vector<uint32_t> &ivFirst = L.cut.ivFirst, &ivPiece = L.cut.ivPiece;
	std::vector<gdsp_interval_piece> mine;
	std::vector<uint64_t> mineImages;
	for (uint32_t j=0 ; j<L.nsel ; j++)
		{
		const uint32_t np = ivFirst[j+1] - ivFirst[j];
		const gdsp_interval_piece* pc = &W.out.h[ivPiece[ivFirst[j]]];
		const uint64_t* im = NULL;
		if ((np > 1) || (pc->flag != 0))
			{
			mine.clear ();  mineImages.clear ();
			for (uint32_t k=0 ; k<np ; k++)
				{
				const uint32_t p = ivPiece[ivFirst[j] + k];
				mine.push_back (W.out.h[p]);
				if (W.out.h[p].flag == 0) continue;
				const size_t f = (size_t) (std::lower_bound (flagged.begin (), flagged.end (), p) - flagged.begin ());
				mineImages.insert (mineImages.end (), &images[f * GDSP_XSUM_WORDS], &images[(f+1) * GDSP_XSUM_WORDS]);
				}
			pc = mine.data ();
			im = mineImages.empty ()? NULL : mineImages.data ();
			}
		const int rc = gdsp_interval_stats_combine (pc, np, im, &h_out[L.sel[j]]);
		if (rc != GDSP_OK) return rc;
		isReport.last[3] += h_out[L.sel[j]].image;
		}
	isReport.last[2] += flagged.size ();
	return GDSP_OK;
	}

// x = (-1)^neg * m * 2^e with m an integer below 2^53 (x finite and not zero)
static inline void is_decompose (double x, uint64_t& m, int& e, bool& neg)
	{
	union { double d; uint64_t u; } b;
	b.d = x;
	const int be = (int) ((b.u >> 52) & 0x7FF);
	m   = b.u & 0xFFFFFFFFFFFFFull;
	neg = (b.u >> 63) != 0;
	if (be != 0) { m |= 1ull << 52;  e = be - 1075; }
	else         e = -1074;
	}

// (s + e) / n rounded once, for s = fl(s + e), e != 0, n >= 1: the sum as one integer M * 2^ee of at most 115 bits, a
// 128-bit division that leaves the quotient 56 bits or more, and the image's rounding (xs_round_limbs) of quotient and
// remainder.  False when e lies more than 60 bits below s's last place (the caller takes the integer image).
static bool is_mean_of_two (double s, double e, uint64_t n, double* mean)
	{
	uint64_t ms, me;  int es, ee;  bool ns, ne;
	if ((s == 0.0) || (n == 0) || (n >> 32) > 1) return false;
	is_decompose (s, ms, es, ns);
	is_decompose (e, me, ee, ne);
	const int z = __builtin_ctzll (me);
	me >>= z;  ee += z;
	const int d = es - ee;
	if ((d < 0) || (d > 60)) return false;
	__int128 M = (__int128) ms << d;
	if (ns) M = -M;
	M += ne? -(__int128) me : (__int128) me;
	const bool neg = M < 0;
	unsigned __int128 A = neg? (unsigned __int128) (-M) : (unsigned __int128) M;
	const int k = (d < 37)? 37 - d : 0;                      // |M| has 52 + d bits or more: the quotient at least 56
	A <<= k;
	const unsigned __int128 q = A / n, r = A % n;
	std::vector<uint32_t> L (4);
	for (int w=0 ; w<4 ; w++) L[w] = (uint32_t) (q >> (32*w));
	*mean = xs_round_limbs (L, r != 0, ee - k, neg);
	return true;
	}

extern "C" {

uint32_t gdsp_interval_stats_tile (void) { return IS_TILE; }

int gdsp_interval_stats_combine (const gdsp_interval_piece* pieces, uint32_t npieces, const uint64_t* images, gdsp_interval_stat* out)
	{
	GDSP_REQUIRE (out != NULL, "NULL result");
	GDSP_REQUIRE ((npieces == 0) || (pieces != NULL), "NULL pieces");
	const GdspPiecesMerge m = gdsp_pieces_merge (pieces, npieces);
	GDSP_REQUIRE (!m.anyFlag || (images != NULL), "a flagged piece without its image");
	out->count = m.count;  out->image = 0;
	if (m.count == 0) { out->sum = 0.0;  out->mean = out->min = out->max = NAN;  out->maxpos = UINT32_MAX;  return GDSP_OK; }
	out->min = m.min + 0.0;  out->max = m.max + 0.0;  out->maxpos = m.maxpos;         // (-0.0 + 0.0 is +0.0)
	double a[2];
	if (!m.anyFlag && gdsp_pieces_two_terms (pieces, npieces, a))
		{
		const double s  = a[0] + a[1];
		const double bp = s - a[0];
		const double e  = (a[0] - (s - bp)) + (a[1] - bp);
		// the exact sum is s + e and s is it rounded once; the mean is one IEEE division when e is zero, else a
		// 128-bit one (is_mean_of_two) unless e lies too far below s for that
		if (xs_finite (s) && ((e == 0.0) || is_mean_of_two (s, e, m.count, &out->mean)))
			{
			out->sum = s + 0.0;
			if (e == 0.0) out->mean = s / (double) m.count;
			return GDSP_OK;
			}
		}
	uint64_t img[GDSP_XSUM_WORDS];
	gdsp_pieces_image (pieces, npieces, images, img);
	img[GDSP_XSUM_WORD_INF] = 0;
	out->sum  = gdsp_xsum_round (img);
	out->mean = gdsp_xsum_div_round (img, m.count);
	out->image = 1;
	return GDSP_OK;
	}

int gdsp_interval_stats_batch (const gdsp_batch_item* items, int nitems, const uint32_t* h_vec, const uint32_t* h_start,
                               const uint32_t* h_end, uint32_t count, double lo, double hi, gdsp_interval_stat* h_out, void* stream)
	{
	GDSP_REQUIRE ((count == 0) || (h_out != NULL), "NULL result array");
	std::vector<uint32_t> flagged;                    // the running launch's flagged pieces, and their images
	std::vector<uint64_t> images;
	return ic_run (__func__, "gdsp_interval_stats", isReport, isBuffers, items, nitems, h_vec, h_start, h_end, count, 1, stream,
		[&] (IsBuffers& W, const IcLaunch& L)
			{
			hipLaunchKernelGGL (interval_stats_kernel, dim3(L.cut.nitems), dim3(IS_THREADS), 0, L.s, L.B, reinterpret_cast<const uint4*> (W.items.d),
			                    W.pieces.d, lo, hi, W.out.d);
			},
		[&] (IsBuffers& W, const IcLaunch& L) { return is_flagged (W, L, lo, hi, flagged, images); },
		[&] (IsBuffers& W, const IcLaunch& L) { return is_combine (W, L, flagged, images, h_out); });
	}

int gdsp_interval_stats_set_launch_pieces (uint32_t pieces)
	{ GDSP_REQUIRE (pieces <= IC_LAUNCH_PIECES, "more pieces than a launch takes");  isReport.launchPieces = pieces;  return GDSP_OK; }

int gdsp_interval_stats (const double* d_v, uint32_t n, const uint32_t* h_start, const uint32_t* h_end, uint32_t count,
                         double lo, double hi, gdsp_interval_stat* h_out, void* stream)
	{
	gdsp_batch_item item;
	item.d_in = d_v;  item.d_out = NULL;  item.n = n;
	return gdsp_interval_stats_batch (&item, 1, NULL, h_start, h_end, count, lo, hi, h_out, stream);
	}

void gdsp_interval_stats_last  (uint64_t out[4]) { memcpy (out, isReport.last, sizeof(isReport.last)); }
void gdsp_interval_stats_times (double ms[4])    { memcpy (ms, isReport.ms, sizeof(isReport.ms)); }

} // extern "C"
