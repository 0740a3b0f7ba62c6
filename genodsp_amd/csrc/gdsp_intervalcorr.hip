// gdsp_intervalcorr.hip -- correlateover (not in the reference): for every interval of a call, correlate's figures of the
// signal against a second track over the interval's pair sample -- count, both means and standard deviations, the
// covariance, the correlation, slope and intercept, each exact and rounded once or derived from such
// (include/genodsp_hip.h; the definition is gdsp_genome_correlation's, per interval).
//
// The work is cut as statsover cuts it (gdsp_interval_cut.h): intervals into pieces at the tiles of the signal's 16-byte
// frame, the pieces sorted by tile, a workgroup per item of at most 64 pieces of one tile, the hull of the item's pieces
// staged into LDS with 16-byte loads, the four waves taking the pieces in turn.  What is this file's own is a wave that
// walks two streams per piece, in two passes over the same items:
//   pass 1  per piece the size of its pair sample and a two-term expansion each for the sums of x and of y: statsover's
//           record without min, max and maxpos, and statsover's walk -- 64 lanes at stride 64, two expansions per sum and
//           lane (gdsp_xsum_dev.h: unchecked, a residual or an overflow sets the record's flag), a shuffle tree, lane 0
//           writes;
//   means   the host combines an interval's pieces exactly (gdsp_interval_stats_combine: one division where TwoSum left
//           nothing over, else the 128-bit or the image route) and uploads one (meanx, meany) per PIECE -- overlapping
//           intervals have different means over the same bases;
//   pass 2  per pair dx = fl(x - meanx), dy = fl(y - meany), qxx = fl(dx dx), qyy = fl(dy dy), qxy = fl(dx dy) (__dsub_rn,
//           __dmul_rn: never contracted, as xsum_pair_kernel<2>), per piece three two-term expansions, a count of the
//           products that are not finite each (left out of the sums, as correlate leaves them) and a flag.
// A piece flagged in either pass is summed again exactly with that piece as the one pair of correlate's exact pass
// (gdsp_xsum_pair_accumulate_batch / _dev_batch, integer images): adversarial data stays exact and gets slower.  The host
// then rounds every sum over the count once (gdsp_interval_stats_combine again, with the pieces' terms) and derives the
// rest as correlate does (gdsp_corr_derive.h).  No atomics, no workgroup reads what another wrote, and every figure is a
// function of the interval's sample alone: nothing depends on the cut, the grid, the launches or the dispatch order.
//
// The second track: x's hull is staged; y is read by the walk itself, straight from global memory, each wave load 64
// consecutive values (512 B), the next round's on their way while this round is added -- so a track of either 16-byte
// parity is read the same way.  Staging y's hull too (64 KiB of LDS, two workgroups a CU; a y congruent to x modulo 16
// bytes staged with x's 16-byte loads, any other value by value) was built and measured against it on the genome: its
// two passes took 1.8 to 2.1 times as long (profiles/correlateover.txt), and it is not kept.
//
// Everything a call and a launch do around pass 1 is gdsp_interval_cut.h's (ic_run); the means, pass 2 and the second sums
// run in its `device` hook, and their kernel and host time is moved to the timers where it belongs.

#include <float.h>
#include <math.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "gdsp_common.h"
#include "gdsp_xsum_dev.h"
#include "gdsp_pieces.h"
#include "gdsp_interval_cut.h"
#include "gdsp_corr_derive.h"

static_assert (sizeof(gdsp_interval_corr) == 72, "the record of the header");

// the second tracks of a launch's vectors: y[s][j] is the track's value under frame value j of vector s (y[s] is the
// track's pointer less the frame's lead; frame value 0 behind a lead is in no piece and never read)
struct IcrTracks { const double* y[GDSP_BATCH_MAX]; };

// a piece's records: pass 1, the sums of x (s[0]) and y (s[1]); pass 2, those of qxx, qyy and qxy, and how many of each
// were not finite
struct IcrSums     { double s[2][XS_K];  uint32_t count, flag; };
struct IcrProducts { double q[3][XS_K];  uint32_t inf[3], flag; };
static_assert (XS_K == 2 && sizeof(IcrSums) == 40 && sizeof(IcrProducts) == 64, "records of two-term expansions");

// PASS 1: out is IcrSums[pieces], means is not read; PASS 2: out is IcrProducts[pieces], means[p] the means of piece p's interval
template <int PASS>
__global__ __launch_bounds__(IC_THREADS)
void interval_corr_kernel (IcBatch B, IcrTracks Y, const uint4* __restrict__ items, const uint32_t* __restrict__ pieces,
                           double lo, double hi, double ylo, double yhi, const double2* __restrict__ means, void* __restrict__ out)
	{
	constexpr int NS = (PASS == 1)? 2 : 3;                // sums
	__shared__ double tile[IC_TILE];
	// the track's tile: the item's vector and tile once more (ic_stage_item keeps them to itself)
	const uint4    raw  = items[blockIdx.x];
	const uint32_t vec  = __builtin_amdgcn_readfirstlane (raw.z) >> 16;
	const double* __restrict__ yv = Y.y[vec] + (uint64_t) __builtin_amdgcn_readfirstlane (raw.y) * IC_TILE;
	uint32_t first, count, pos0;
	ic_stage_item (B, items, tile, first, count, pos0);

	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	for (uint32_t k=wave ; k<count ; k+=IC_WAVES)
		{
		const uint32_t d = __builtin_amdgcn_readfirstlane (pieces[first + k]);
		const uint32_t a = d & 0xFFFF, b = (d >> 16) + 1;
		double meanx = 0.0, meany = 0.0;
		if constexpr (PASS == 2) { const double2 m = means[first + k];  meanx = m.x;  meany = m.y; }
		double   acc[NS][2][XS_K];                          // per sum, one expansion for each half of the walk's round
		uint32_t cnt = 0, flag = 0, infs[NS];
#pragma unroll
		for (int s=0 ; s<NS ; s++)
			{
			infs[s] = 0;
#pragma unroll
			for (int h=0 ; h<2 ; h++)
#pragma unroll
				for (int j=0 ; j<XS_K ; j++) acc[s][h][j] = 0.0;
			}
		auto take = [&] (const int h, uint32_t i, double y)
			{
			const double x = tile[i];
			const bool   in = !(x < lo) && !(x > hi) && xs_finite (x) && !(y < ylo) && !(y > yhi) && xs_finite (y);   // correlate's tests
			cnt += in;
			double t[NS];
			if constexpr (PASS == 1) { t[0] = x;  t[1] = y; }
			else
				{
				const double dx = __dsub_rn (x, meanx), dy = __dsub_rn (y, meany);
				t[0] = __dmul_rn (dx, dx);  t[1] = __dmul_rn (dy, dy);  t[2] = __dmul_rn (dx, dy);
				}
#pragma unroll
			for (int s=0 ; s<NS ; s++)
				{
				const bool big = (PASS == 2) && in && !xs_finite (t[s]);      // q = +-inf or NaN: counted, not added
				infs[s] += big;
				xs_grow_or_flag (acc[s][h], (in && !big)? t[s] : 0.0, flag);
				}
			};
		// the round's two values of y are on their way while the round before is added (a lane beyond the piece's end
		// rereads its last value, which is then not taken)
		uint32_t i = a + lane;
		double y0 = yv[min (i, b - 1)], y1 = yv[min (i + 64, b - 1)];
		for ( ; i+64<b ; i+=128)
			{
			const double n0 = yv[min (i + 128, b - 1)], n1 = yv[min (i + 192, b - 1)];
			take (0, i, y0);  take (1, i+64, y1);
			y0 = n0;  y1 = n1;
			}
		if (i < b) take (0, i, y0);

		// per sum: the lane's two expansions, then the wave's 64 as a tree: lane l takes lane l+off's terms when l % 2off == 0
#pragma unroll
		for (int s=0 ; s<NS ; s++)
			{
#pragma unroll
			for (int j=0 ; j<XS_K ; j++) xs_grow_or_flag (acc[s][0], acc[s][1][j], flag);
			for (int off=1 ; off<64 ; off<<=1)
				{
				double tt[XS_K];
#pragma unroll
				for (int j=0 ; j<XS_K ; j++) tt[j] = __shfl_down (acc[s][0][j], off, 64);
				const bool mine = (lane & (2*off - 1)) == 0;
#pragma unroll
				for (int j=0 ; j<XS_K ; j++) xs_grow_or_flag (acc[s][0], mine? tt[j] : 0.0, flag);
				}
			}
		for (int off=32 ; off>0 ; off>>=1)
			{
			cnt  += __shfl_down (cnt, off, 64);
			flag |= __shfl_down (flag, off, 64);
#pragma unroll
			for (int s=0 ; s<NS ; s++) infs[s] += __shfl_down (infs[s], off, 64);
			}
		if (lane == 0)
			{
			if constexpr (PASS == 1)
				{
				IcrSums r;
#pragma unroll
				for (int s=0 ; s<2 ; s++) { r.s[s][0] = acc[s][0][0];  r.s[s][1] = acc[s][0][1]; }
				r.count = cnt;  r.flag = flag;
				static_cast<IcrSums*> (out)[first + k] = r;
				}
			else
				{
				IcrProducts r;
#pragma unroll
				for (int s=0 ; s<3 ; s++) { r.q[s][0] = acc[s][0][0];  r.q[s][1] = acc[s][0][1];  r.inf[s] = infs[s]; }
				r.flag = flag;
				static_cast<IcrProducts*> (out)[first + k] = r;
				}
			}
		}
	}

// ---------------------------------------------------------------------------------------------- host ----
// per device: the launch's buffers (gdsp_interval_cut.h; `out` holds pass 1's records), pass 2's records, the pieces' means
// and the staging of the flagged pieces' second sums
struct IcrBuffers : IcBuffers<IcrSums>
	{
	GdspStaged<IcrProducts> products;
	GdspStaged<double2>     means;
	GdspStaged<uint64_t>    img;
	};
static IcrBuffers icrBuffers[64];
static IcReport   icrReport;                          // last: intervals, pieces, pieces flagged in pass 1, in pass 2

#define ICR_FLAG_BATCH 256                            // flagged pieces summed again per read-back (two or three images each)

// what a call keeps from hook to hook of the running launch
struct IcrCall
	{
	double lo, hi, ylo, yhi;
	const gdsp_batch_item* items;                     // the caller's table
	gdsp_interval_corr*    h_out;
	GdspEventPair ev;                                 // pass 2's, made when the first launch gets there
	IcrTracks Y;
	std::vector<gdsp_interval_stat> sums;             // [nsel][2]: count and mean of x and of y
	std::vector<uint32_t> flagged[2];                 // the pieces flagged in pass 1, in pass 2, ascending
	std::vector<uint64_t> images[2];                  // their images: two each, three each
	};

// the pieces flagOf names, each summed again as the one pair of correlate's exact pass -- pass 1's two images, or with
// means pass 2's three -- ICR_FLAG_BATCH pieces per read-back
template <typename FlagOf>
static int icr_flagged (IcrCall& c, IcrBuffers& W, const IcLaunch& L, int pass, FlagOf flagOf, std::vector<uint32_t>& flagged,
                        std::vector<uint64_t>& images)
	{
	const size_t per = (size_t) ((pass == 1)? 2 : 3) * GDSP_XSUM_WORDS, words = ICR_FLAG_BATCH * per;
	flagged.clear ();
	for (uint32_t p=0 ; p<L.cut.P ; p++) { if (flagOf (p)) flagged.push_back (p); }
	images.assign (flagged.size () * per, 0);
	if (flagged.empty ()) return GDSP_OK;
	int rc = W.img.grow (words, "gdsp_interval_correlation", 0, words);
	if (rc != GDSP_OK) return rc;
	for (size_t f0=0 ; f0<flagged.size () ; f0+=ICR_FLAG_BATCH)
		{
		const size_t m = std::min<size_t> (ICR_FLAG_BATCH, flagged.size () - f0);
		GDSP_HIP_TRY (hipMemsetAsync (W.img.d, 0, m * per * sizeof(uint64_t), L.s));
		for (size_t f=0 ; f<m ; f++)
			{
			const uint32_t p = flagged[f0 + f];
			const uint32_t g = (uint32_t) (std::upper_bound (L.cut.tileFirst.begin (), L.cut.tileFirst.end (), p) - L.cut.tileFirst.begin ()) - 1;
			int v = 0;
			while ((v+1 < L.nvec) && (L.vecs[v+1].tile0 <= g)) v++;
			const uint32_t a = W.pieces.h[p] & 0xFFFF, b = (W.pieces.h[p] >> 16) + 1;
			const uint64_t at = (uint64_t) (g - L.vecs[v].tile0) * IC_TILE + a;
			gdsp_xsum_pair pair;
			pair.d_x = L.B.base[v] + at;  pair.d_y = c.Y.y[v] + at;  pair.n = b - a;  pair.first = 0;
			pair.device = L.dev;  pair.stream = (void*) L.s;
			if (pass == 1) rc = gdsp_xsum_pair_accumulate_batch (&pair, 1, 1, c.lo, c.hi, c.ylo, c.yhi, W.img.d + f * per, (void*) L.s);
			else           rc = gdsp_xsum_pair_accumulate_dev_batch (&pair, 1, 1, c.lo, c.hi, c.ylo, c.yhi, W.means.h[p].x, W.means.h[p].y,
			                                                          W.img.d + f * per, (void*) L.s);
			if (rc != GDSP_OK) return rc;
			}
		GDSP_HIP_TRY (hipMemcpyAsync (W.img.h, W.img.d, m * per * sizeof(uint64_t), hipMemcpyDeviceToHost, L.s));
		GDSP_HIP_TRY (hipStreamSynchronize (L.s));
		memcpy (&images[f0 * per], W.img.h, m * per * sizeof(uint64_t));
		}
	return GDSP_OK;
	}

// interval j's sum number `which` of a pass over its sample's size, exact and rounded once, in st->mean (and the size in
// st->count): its pieces' terms as statsover's records, the images of the flagged among them, gdsp_interval_stats_combine
struct IcrGather { std::vector<gdsp_interval_piece> pieces;  std::vector<uint64_t> images; };
static int icr_ratio (const IcrCall& c, const IcrBuffers& W, const IcLaunch& L, uint32_t j, int pass, int which, IcrGather& G, gdsp_interval_stat* st)
	{
	const size_t per = (size_t) ((pass == 1)? 2 : 3) * GDSP_XSUM_WORDS;
	const std::vector<uint32_t>& flagged = c.flagged[pass-1];
	G.pieces.clear ();  G.images.clear ();
	for (uint32_t k=L.cut.ivFirst[j] ; k<L.cut.ivFirst[j+1] ; k++)
		{
		const uint32_t p = L.cut.ivPiece[k];
		gdsp_interval_piece r;
		memset (&r, 0, sizeof(r));
		const double* terms = (pass == 1)? W.out.h[p].s[which] : W.products.h[p].q[which];
		r.a0 = terms[0];  r.a1 = terms[1];  r.count = W.out.h[p].count;
		r.flag = (pass == 1)? W.out.h[p].flag : W.products.h[p].flag;
		G.pieces.push_back (r);
		if (r.flag == 0) continue;
		const size_t f = (size_t) (std::lower_bound (flagged.begin (), flagged.end (), p) - flagged.begin ());
		const uint64_t* img = &c.images[pass-1][f * per + (size_t) which * GDSP_XSUM_WORDS];
		G.images.insert (G.images.end (), img, img + GDSP_XSUM_WORDS);
		}
	return gdsp_interval_stats_combine (G.pieces.data (), (uint32_t) G.pieces.size (), G.images.empty ()? NULL : G.images.data (), st);
	}

static void icr_start (const IcrCall& c, IcrBuffers& W, const IcLaunch& L, int pass)
	{
	const uint4* items = reinterpret_cast<const uint4*> (W.items.d);
	if (pass == 1) hipLaunchKernelGGL (interval_corr_kernel<1>, dim3(L.cut.nitems), dim3(IC_THREADS), 0, L.s, L.B, c.Y, items, W.pieces.d,
	                                   c.lo, c.hi, c.ylo, c.yhi, (const double2*) NULL, (void*) W.out.d);
	else           hipLaunchKernelGGL (interval_corr_kernel<2>, dim3(L.cut.nitems), dim3(IC_THREADS), 0, L.s, L.B, c.Y, items, W.pieces.d,
	                                   c.lo, c.hi, c.ylo, c.yhi, W.means.d, (void*) W.products.d);
	}

// before pass 1: the launch's tracks
static void icr_tracks (IcrCall& c, const IcLaunch& L)
	{
	for (int k=0 ; k<GDSP_BATCH_MAX ; k++)
		{
		const double* y = (k < L.nvec)? c.items[L.vecBase + k].d_out : NULL;
		c.Y.y[k] = (y != NULL)? y - L.vecs[k].lead : NULL;
		}
	}

// behind pass 1's records: its flagged pieces' second sums, every interval's means, pass 2 and its flagged pieces'
static int icr_second_pass (IcrCall& c, IcrBuffers& W, const IcLaunch& L)
	{
	int rc = icr_flagged (c, W, L, 1, [&] (uint32_t p) { return W.out.h[p].flag != 0; }, c.flagged[0], c.images[0]);
	if (rc == GDSP_OK) rc = W.products.grow (L.cut.P, "gdsp_interval_correlation");
	if (rc == GDSP_OK) rc = W.means.grow (L.cut.P, "gdsp_interval_correlation");
	if (rc != GDSP_OK) return rc;

	const GdspTimer tMeans;
	IcrGather G;
	c.sums.resize ((size_t) L.nsel * 2);
	for (uint32_t j=0 ; j<L.nsel ; j++)
		{
		for (int which=0 ; which<2 ; which++)
			{
			rc = icr_ratio (c, W, L, j, 1, which, G, &c.sums[(size_t) j*2 + which]);
			if (rc != GDSP_OK) return rc;
			}
		const double2 m = { c.sums[(size_t) j*2].mean, c.sums[(size_t) j*2 + 1].mean };      // (NaN of an empty sample: nothing is multiplied)
		for (uint32_t k=L.cut.ivFirst[j] ; k<L.cut.ivFirst[j+1] ; k++) W.means.h[L.cut.ivPiece[k]] = m;
		}
	const double meansMs = tMeans.ms ();

	if (c.ev.ev0 == NULL) rc = c.ev.create ("gdsp_interval_correlation");
	if (rc != GDSP_OK) return rc;
	GDSP_HIP_TRY (hipMemcpyAsync (W.means.d, W.means.h, (size_t) L.cut.P * sizeof(double2), hipMemcpyHostToDevice, L.s));
	GDSP_HIP_TRY (hipEventRecord (c.ev.ev0, L.s));
	icr_start (c, W, L, 2);
	GDSP_LAUNCH_CHECK ();
	GDSP_HIP_TRY (hipEventRecord (c.ev.ev1, L.s));
	GDSP_HIP_TRY (hipMemcpyAsync (W.products.h, W.products.d, (size_t) L.cut.P * sizeof(IcrProducts), hipMemcpyDeviceToHost, L.s));
	GDSP_HIP_TRY (hipStreamSynchronize (L.s));
	float kernelMs = 0;
	GDSP_HIP_TRY (hipEventElapsedTime (&kernelMs, c.ev.ev0, c.ev.ev1));
	rc = icr_flagged (c, W, L, 2, [&] (uint32_t p) { return W.products.h[p].flag != 0; }, c.flagged[1], c.images[1]);
	if (rc != GDSP_OK) return rc;
	// ic_run books this hook as copying and waiting: pass 2's kernel and the means belong to the kernel and to combining
	icrReport.ms[1] += kernelMs;  icrReport.ms[3] += meansMs;  icrReport.ms[2] -= kernelMs + meansMs;
	icrReport.last[2] += c.flagged[0].size ();  icrReport.last[3] += c.flagged[1].size ();
	return GDSP_OK;
	}

// the records of the launch's intervals
static int icr_combine (IcrCall& c, IcrBuffers& W, const IcLaunch& L)
	{
	IcrGather G;
	for (uint32_t j=0 ; j<L.nsel ; j++)
		{
		gdsp_interval_corr& o = c.h_out[L.sel[j]];
		const gdsp_interval_stat &sx = c.sums[(size_t) j*2], &sy = c.sums[(size_t) j*2 + 1];
		o.count = (uint32_t) sx.count;  o.reserved = 0;
		o.mean = o.filemean = o.stddev = o.filestddev = o.covariance = o.correlation = o.slope = o.intercept = NAN;
		if (sx.count == 0) continue;
		uint64_t infs[3] = { 0, 0, 0 };
		for (uint32_t k=L.cut.ivFirst[j] ; k<L.cut.ivFirst[j+1] ; k++)
			{ for (int s=0 ; s<3 ; s++) infs[s] += W.products.h[L.cut.ivPiece[k]].inf[s]; }
		double fig[GDSP_CORR_FIGURES];
		for (int k=0 ; k<GDSP_CORR_FIGURES ; k++) fig[k] = NAN;
		fig[GDSP_CORR_MEANX] = sx.mean;  fig[GDSP_CORR_MEANY] = sy.mean;
		static const int where[3] = { GDSP_CORR_VARX, GDSP_CORR_VARY, GDSP_CORR_COV };
		for (int s=0 ; s<3 ; s++)
			{
			gdsp_interval_stat st;
			if (infs[s] != 0) { fig[where[s]] = (s < 2)? HUGE_VAL : NAN;  continue; }      // correlate's rule for products that are not finite
			const int rc = icr_ratio (c, W, L, j, 2, s, G, &st);
			if (rc != GDSP_OK) return rc;
			fig[where[s]] = st.mean;
			}
		gdsp_corr_derive (fig);
		o.mean = fig[GDSP_CORR_MEANX];  o.filemean = fig[GDSP_CORR_MEANY];  o.stddev = fig[GDSP_CORR_SDX];  o.filestddev = fig[GDSP_CORR_SDY];
		o.covariance = fig[GDSP_CORR_COV];  o.correlation = fig[GDSP_CORR_CORRELATION];  o.slope = fig[GDSP_CORR_SLOPE];
		o.intercept = fig[GDSP_CORR_INTERCEPT];
		}
	return GDSP_OK;
	}

extern "C" {

uint32_t gdsp_interval_correlation_tile (void) { return IC_TILE; }

int gdsp_interval_correlation_set_launch_pieces (uint32_t pieces)
	{ GDSP_REQUIRE (pieces <= IC_LAUNCH_PIECES, "more pieces than a launch takes");  icrReport.launchPieces = pieces;  return GDSP_OK; }

int gdsp_interval_correlation_batch (const gdsp_batch_item* items, int nitems, const uint32_t* h_vec, const uint32_t* h_start,
                                     const uint32_t* h_end, uint32_t count, double lo, double hi, double ylo, double yhi,
                                     gdsp_interval_corr* h_out, void* stream)
	{
	GDSP_REQUIRE ((count == 0) || (h_out != NULL), "NULL result array");
	for (int k=0 ; (count != 0) && (items != NULL) && (k<nitems) ; k++)
		GDSP_REQUIRE ((items[k].n == 0) || ((items[k].d_out != NULL) && ((((uintptr_t) items[k].d_out) & 7) == 0)), "a track is NULL or not 8-byte aligned");
	IcrCall c;
	c.lo = lo;  c.hi = hi;  c.ylo = ylo;  c.yhi = yhi;  c.items = items;  c.h_out = h_out;
	return ic_run (__func__, "gdsp_interval_correlation", icrReport, icrBuffers, items, nitems, h_vec, h_start, h_end, count, 1, stream,
		[&] (IcrBuffers& W, const IcLaunch& L) { icr_tracks (c, L);  icr_start (c, W, L, 1); },
		[&] (IcrBuffers& W, const IcLaunch& L) { return icr_second_pass (c, W, L); },
		[&] (IcrBuffers& W, const IcLaunch& L) { return icr_combine (c, W, L); });
	}

int gdsp_interval_correlation (const double* d_x, const double* d_y, uint32_t n, const uint32_t* h_start, const uint32_t* h_end,
                               uint32_t count, double lo, double hi, double ylo, double yhi, gdsp_interval_corr* h_out, void* stream)
	{
	gdsp_batch_item item;
	item.d_in = d_x;  item.d_out = const_cast<double*> (d_y);  item.n = n;
	return gdsp_interval_correlation_batch (&item, 1, NULL, h_start, h_end, count, lo, hi, ylo, yhi, h_out, stream);
	}

void gdsp_interval_correlation_last  (uint64_t out[4]) { memcpy (out, icrReport.last, sizeof(icrReport.last)); }
void gdsp_interval_correlation_times (double ms[4])    { memcpy (ms, icrReport.ms, sizeof(icrReport.ms)); }

} // extern "C"
