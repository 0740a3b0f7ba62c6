// gdsp_intervalbreadth.hip -- breadthover (not in the reference): for every interval of a call, the size of its sample
// and, for up to 16 thresholds, how many sampled bases are at or above (or above) each (include/genodsp_hip.h).
//
// The work is cut as statsover cuts it (gdsp_interval_cut.h): intervals into pieces at the tiles of the vector's 16-byte
// frame, the pieces sorted by tile, a workgroup per item of at most 64 pieces of one tile, the hull of the item's pieces
// staged into LDS with 16-byte loads, the four waves taking the pieces in turn.  What is this file's own is what a wave
// does with 64 staged values: the sample test, which turns a value outside the sample into a NaN, and one comparison per
// threshold, each taken as the wave's 64-bit lane mask (ballot), counted with a population count and added to a counter
// that is uniform over the wave -- so the counters live in scalar registers, 32 bits and unsigned (a piece has at most
// IC_TILE bases), there is no shuffle tree at the end, and lane 0 writes the piece's record: the count and one figure per
// threshold.  (Measured against two other forms on the genome at 16 thresholds, whole chromosomes / a million peaks: the
// masks ANDed with the sample's mask instead of the NaN 15.5 / 5.4 ms, this form 14.4 / 5.1, per-lane counters fed by
// the compare bit and folded with shuffles per piece 15.5 / 6.2 -- no scalar work at all and no faster: the sixteen
// 64-bit compares are the cost.)  The thresholds
// are kernel arguments, sorted ascending by the host, and the kernel is compiled for 1, 2, 4, 8 and 16 of them (a call's
// list is padded with +inf, which no sampled value reaches), every loop over them unrolled: no register array is
// indexed at run time.  Behind every fourth threshold a wave whose mask is empty leaves the rest of the list alone,
// since no later, greater threshold can be met.  No atomics, no workgroup reads what another wrote, and every figure is an
// integer: nothing depends on the cut, the grid or the dispatch order.
//
// The host adds an interval's pieces in 64-bit integers and gives the columns back in the caller's order of thresholds.
// Everything a call and a launch do around the kernel is gdsp_interval_cut.h's (ic_run), shared with statsover.

#include <float.h>
#include <math.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "gdsp_common.h"
#include "gdsp_xsum_dev.h"
#include "gdsp_pieces.h"
#include "gdsp_interval_cut.h"

struct IbThresholds { double t[GDSP_INTERVAL_THRESHOLDS_MAX]; };

// a piece's record: out[piece * (Q+1)] = its sample's size, then Q counts in the kernel's (ascending) order of thresholds
template <int Q, bool STRICT>
__global__ __launch_bounds__(IC_THREADS)
void interval_breadth_kernel (IcBatch B, const uint4* __restrict__ items, const uint32_t* __restrict__ pieces, double lo, double hi,
                              IbThresholds T, uint32_t* __restrict__ out)
	{
	__shared__ double tile[IC_TILE];
	uint32_t first, count, pos0;
	ic_stage_item (B, items, tile, first, count, pos0);

	const uint32_t wave = __builtin_amdgcn_readfirstlane (threadIdx.x >> 6), lane = threadIdx.x & 63;
	for (uint32_t k=wave ; k<count ; k+=IC_WAVES)
		{
		const uint32_t d = __builtin_amdgcn_readfirstlane (pieces[first + k]);
		const uint32_t a = d & 0xFFFF, b = (d >> 16) + 1;
		uint32_t cnt = 0, acc[Q];                                   // uniform over the wave
#pragma unroll
		for (int j=0 ; j<Q ; j++) acc[j] = 0;
		// all 64 lanes walk the piece together; a lane beyond the piece's end rereads the last value and is masked out
		double x = tile[min (a + lane, b - 1)];
		for (uint32_t i0=a ; i0<b ; i0+=64)
			{
			const double xn = tile[min (i0 + 64 + lane, b - 1)];    // (the next round's, on its way while this one counts)
			const bool   in = (i0 + lane < b) && !(x < lo) && !(x > hi) && xs_finite (x);      // stats' tests; NaN and +-inf never
			cnt += (uint32_t) __builtin_popcountll (__builtin_amdgcn_ballot_w64 (in));
			const double xe = in? x : __builtin_nan ("");           // outside the sample: no comparison holds, so no mask needs the sample's
			bool met = true;                                        // (uniform) the last threshold looked at was met by some lane
#pragma unroll
			for (int g=0 ; g<Q ; g+=4)                              // four thresholds, then a look whether the rest can be met
				{
				if (!met) continue;
				uint64_t m = 0;
#pragma unroll
				for (int j=g ; (j<g+4) && (j<Q) ; j++)
					{
					m = __builtin_amdgcn_ballot_w64 (STRICT? (xe > T.t[j]) : (xe >= T.t[j]));
					acc[j] += (uint32_t) __builtin_popcountll (m);
					}
				met = (m != 0);
				}
			x = xn;
			}
		if (lane == 0)
			{
			uint32_t* r = out + (size_t) (first + k) * (Q + 1);
			r[0] = cnt;
#pragma unroll
			for (int j=0 ; j<Q ; j++) r[1+j] = acc[j];
			}
		}
	}

// ---------------------------------------------------------------------------------------------- host ----
typedef IcBuffers<uint32_t> IbBuffers;                // a piece's record: Q + 1 words (a launch's IC_LAUNCH_PIECES: at most 272 MiB)
static IbBuffers ibBuffers[64];
static IcReport  ibReport;                            // last: intervals, pieces, launches, workgroups

// what a call asks of every launch: the thresholds as the kernel takes them and where each goes in the caller's order
struct IbQuery
	{
	IbThresholds T;
	int nt, Q, strict;                                // Q: the kernel's list, nt rounded up to 1, 2, 4, 8 or 16
	int column[GDSP_INTERVAL_THRESHOLDS_MAX];         // the kernel's figure j is the caller's column[j] (j < nt)
	double lo, hi;
	};

template <int Q>
static void ib_start (const IbQuery& q, uint32_t nitems, hipStream_t s, const IcBatch& B, const uint4* items, const uint32_t* pieces, uint32_t* out)
	{
	if (q.strict != 0) hipLaunchKernelGGL ((interval_breadth_kernel<Q, true>),  dim3(nitems), dim3(IC_THREADS), 0, s, B, items, pieces, q.lo, q.hi, q.T, out);
	else               hipLaunchKernelGGL ((interval_breadth_kernel<Q, false>), dim3(nitems), dim3(IC_THREADS), 0, s, B, items, pieces, q.lo, q.hi, q.T, out);
	}

static void ib_start_launch (const IbQuery& q, IbBuffers& W, const IcLaunch& L)
	{
	const uint4* items = reinterpret_cast<const uint4*> (W.items.d);
	switch (q.Q)
		{
		case 1:  ib_start<1>  (q, L.cut.nitems, L.s, L.B, items, W.pieces.d, W.out.d);  break;
		case 2:  ib_start<2>  (q, L.cut.nitems, L.s, L.B, items, W.pieces.d, W.out.d);  break;
		case 4:  ib_start<4>  (q, L.cut.nitems, L.s, L.B, items, W.pieces.d, W.out.d);  break;
		case 8:  ib_start<8>  (q, L.cut.nitems, L.s, L.B, items, W.pieces.d, W.out.d);  break;
		default: ib_start<16> (q, L.cut.nitems, L.s, L.B, items, W.pieces.d, W.out.d);  break;
		}
	}

// an interval's pieces, added in 64 bits (e - s <= 2^32 - 1 bounds every sum), into the caller's columns
static int ib_combine (const IbQuery& q, IbBuffers& W, const IcLaunch& L, uint32_t* h_count, uint32_t* h_atleast)
	{
	const size_t rec = (size_t) q.Q + 1;
	for (uint32_t j=0 ; j<L.nsel ; j++)
		{
		uint64_t sum[GDSP_INTERVAL_THRESHOLDS_MAX + 1] = { 0 };
		for (uint32_t k=L.cut.ivFirst[j] ; k<L.cut.ivFirst[j+1] ; k++)
			{
			const uint32_t* r = &W.out.h[(size_t) L.cut.ivPiece[k] * rec];
			for (int c=0 ; c<=q.nt ; c++) sum[c] += r[c];
			}
		const uint32_t i = L.sel[j];
		h_count[i] = (uint32_t) sum[0];
		for (int c=0 ; c<q.nt ; c++) h_atleast[(size_t) i * q.nt + q.column[c]] = (uint32_t) sum[1+c];
		}
	ibReport.last[2] += 1;  ibReport.last[3] += L.cut.nitems;
	return GDSP_OK;
	}

extern "C" {

uint32_t gdsp_interval_breadth_tile (void) { return IC_TILE; }

int gdsp_interval_breadth_set_launch_pieces (uint32_t pieces)
	{ GDSP_REQUIRE (pieces <= IC_LAUNCH_PIECES, "more pieces than a launch takes");  ibReport.launchPieces = pieces;  return GDSP_OK; }

int gdsp_interval_breadth_batch (const gdsp_batch_item* items, int nitems, const uint32_t* h_vec, const uint32_t* h_start,
                                 const uint32_t* h_end, uint32_t count, const double* thresholds, int nt, int strict,
                                 double lo, double hi, uint32_t* h_count, uint32_t* h_atleast, void* stream)
	{
	GDSP_REQUIRE ((nt >= 1) && (nt <= GDSP_INTERVAL_THRESHOLDS_MAX), "the number of thresholds must be in 1..16");
	GDSP_REQUIRE (thresholds != NULL, "NULL thresholds");
	for (int j=0 ; j<nt ; j++) GDSP_REQUIRE (thresholds[j] == thresholds[j], "a threshold is NaN");
	GDSP_REQUIRE ((count == 0) || ((h_count != NULL) && (h_atleast != NULL)), "NULL result arrays");

	// ascending for the kernel (equal thresholds in the order given), padded with +inf; the caller's order kept
	IbQuery q;
	q.nt = nt;  q.strict = strict;  q.lo = lo;  q.hi = hi;
	q.Q = 1;
	while (q.Q < nt) q.Q *= 2;
	for (int j=0 ; j<nt ; j++) q.column[j] = j;
	std::stable_sort (q.column, q.column + nt, [&] (int x, int y) { return thresholds[x] < thresholds[y]; });
	for (int j=0 ; j<GDSP_INTERVAL_THRESHOLDS_MAX ; j++) q.T.t[j] = (j < nt)? thresholds[q.column[j]] : HUGE_VAL;

	return ic_run (__func__, "gdsp_interval_breadth", ibReport, ibBuffers, items, nitems, h_vec, h_start, h_end, count, (size_t) q.Q + 1, stream,
		[&] (IbBuffers& W, const IcLaunch& L) { ib_start_launch (q, W, L); },
		[] (IbBuffers&, const IcLaunch&) { return GDSP_OK; },
		[&] (IbBuffers& W, const IcLaunch& L) { return ib_combine (q, W, L, h_count, h_atleast); });
	}

int gdsp_interval_breadth (const double* d_v, uint32_t n, const uint32_t* h_start, const uint32_t* h_end, uint32_t count,
                           const double* thresholds, int nt, int strict, double lo, double hi,
                           uint32_t* h_count, uint32_t* h_atleast, void* stream)
	{
	gdsp_batch_item item;
	item.d_in = d_v;  item.d_out = NULL;  item.n = n;
	return gdsp_interval_breadth_batch (&item, 1, NULL, h_start, h_end, count, thresholds, nt, strict, lo, hi, h_count, h_atleast, stream);
	}

void gdsp_interval_breadth_last  (uint64_t out[4]) { memcpy (out, ibReport.last, sizeof(ibReport.last)); }
void gdsp_interval_breadth_times (double ms[4])    { memcpy (ms, ibReport.ms, sizeof(ibReport.ms)); }

} // extern "C"
