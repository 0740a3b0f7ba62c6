// gdsp_matrixover.hip -- matrixover (not in the reference): the signal around every anchor of a list, one row per anchor
// and one double per cell of `bin` offsets (include/genodsp_hip.h has the definitions) -- profileover's picture before the
// anchors are added up.  A cell is one interval of its chromosome, and its figure is statsover's for that interval.
//
// A wave takes whole anchors, by stride over the launch's rows, and walks each window in ascending base order whatever
// the strand: the strand only decides which column a cell lands in (a minus anchor's ascending cell c is column
// ncols - 1 - c).  Every base of a window is read from HBM once with plain 8-byte loads, the lanes of the wave on
// consecutive doubles, which is right at any 8-byte alignment of the vector.  Three routes, by the bin width b:
//   b == 1       a clipped, strand-ordered copy: lane l reads base g0 + t and writes column t (or noffsets - 1 - t).
//   2 <= b < 256 the wave stages a stretch of 64 / G cells in its own piece of LDS with coalesced loads, eight in flight
//                per lane (a base outside the chromosome is staged as NaN, which nothing samples), and a group of G lanes
//                owns a whole cell: G = 1 below 16 bases, 4 below 64, else 16, so that a stretch is at most MX_STAGE
//                doubles and all 64 lanes work.  The stretch is stored with one double of padding per 32 (index i lives
//                at i + i / 32): lanes a power of two of doubles apart would otherwise meet on one bank.  A group folds
//                its lanes with log2 G steps of the shuffle tree.
//   b >= 256     the wave strides over the cell, two expansions per lane, and folds its 64 lanes with the shuffle tree of
//                interval_stats_kernel.
// The kernel is a template on the figure: min, max and count carry no expansions.  A sum is a lane's two-term expansion
// grown with xs_grow_or_flag; an unflagged cell's a0 + a1 is its exact sum, so fl(a0 + a1) is the sum rounded once.  The
// mean is finished here where the exact sum is one double (TwoSum of a0 and a1 leaves no error term, as it always does on
// read depth): one IEEE division of two exact values is the exact quotient rounded once; and where the sum takes two
// doubles, when a candidate quotient can be PROVEN to be the exact quotient rounded once from its exact remainder
// (mx_finish has the argument: all but ties, near-ties within 2^-40, powers of two and extreme exponents).  Every other
// cell -- flagged, overflowing, or a mean that cannot be proven -- is appended to the launch's to-do list, one atomic per
// wave and stretch, and computed by the host half through gdsp_interval_stats_batch.  One double is written per cell, by one lane; no
// atomics on cells, no wave or workgroup waits for another (the LDS piece is a wave's own), no scratch.
// What concerns the anchors rather than the figures -- their code word, the table of vectors a launch takes, the checks, the
// gather of a device's sources, the walk over the devices, the holder of its allocations -- is gdsp_anchors.h's, shared with
// profileover; the host half of a device's rows -- launches, copies back, the to-do list -- is gdsp_matrix_rows.h's, shared
// with regionsover.

#include <float.h>
#include <math.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "gdsp_common.h"
#include "gdsp_anchors.h"
#include "gdsp_xsum_dev.h"
#include "gdsp_matrix_cell.h"
#include "gdsp_matrix_rows.h"

enum { MX_ROUTE_COPY = 0, MX_ROUTE_NARROW = 1, MX_ROUTE_WIDE = 2 };

template <int WHAT, int ROUTE>
__global__ __launch_bounds__(MX_THREADS)
void matrix_kernel (GdspAnchorTable P, const uint32_t* __restrict__ d_pos, const uint32_t* __restrict__ d_code, uint32_t count,
                    int32_t offLo, uint32_t noffsets, uint32_t bin, uint32_t group, double lo, double hi,
                    double* __restrict__ out, uint32_t* __restrict__ todo, uint32_t* __restrict__ ntodo)
	{
	__shared__ double stage[(ROUTE == MX_ROUTE_NARROW)? MX_WAVES * MX_STAGE_PAD : 1];
	const uint32_t lane  = threadIdx.x & 63;
	const uint32_t wave  = threadIdx.x >> 6;
	const uint32_t ncols = noffsets / bin;
	const uint32_t nwave = gridDim.x * MX_WAVES;

	for (uint32_t row=blockIdx.x*MX_WAVES+wave ; row<count ; row+=nwave)
		{
		const uint32_t code = __builtin_amdgcn_readfirstlane (d_code[row]);
		const uint32_t vec  = gdsp_anchor_vec (code) - P.vec0;
		if (vec >= P.nvec) continue;                                  // (a vector of another launch sequence)
		const double* __restrict__ v = P.v[vec];
		const int64_t n     = (int64_t) P.n[vec];
		const int64_t p     = (int64_t) (uint32_t) __builtin_amdgcn_readfirstlane (d_pos[row]);   // (the builtin returns int: unsigned again before it widens, or a position from 2^31 on turns negative)
		const bool    minus = gdsp_anchor_minus (code);
		// the window is the bases g0 .. g0 + noffsets - 1; ascending cell c is column c, or ncols - 1 - c on the minus strand
		const int64_t g0    = minus? p - (int64_t) offLo - (int64_t) (noffsets - 1) : p + (int64_t) offLo;
		const uint32_t cell0 = row * ncols;                           // (the call's cells fit 32 bits: the host half sees to it)
		double* __restrict__ rowOut = out + (size_t) row * ncols;
		if (n == 0) continue;                                         // (no anchor lies in an empty vector)

		if (ROUTE == MX_ROUTE_COPY)
			{
			for (uint32_t t=lane ; t<noffsets ; t+=64)
				{
				const int64_t g  = g0 + t;
				const bool    in = (g >= 0) && (g < n);
				const double  x  = in? v[g] : NAN;
				const bool    take = !(x < lo) && !(x > hi) && xs_finite (x);
				const uint32_t j = minus? noffsets - 1 - t : t;
				double y;
				if      (WHAT == GDSP_MATRIX_COUNT) y = take? 1.0 : 0.0;
				else if (WHAT == GDSP_MATRIX_SUM)   y = take? __dadd_rn (x, 0.0) : 0.0;
				else                                y = take? __dadd_rn (x, 0.0) : NAN;     // (one value is its own mean, min and max)
				rowOut[j] = y;
				}
			}

		if (ROUTE == MX_ROUTE_NARROW)
			{
			double* __restrict__ mine = stage + wave * MX_STAGE_PAD;
			const uint32_t perPass = 64 / group;                           // cells of a stretch
			const uint32_t cell = lane / group, r = lane % group;
			for (uint32_t c0=0 ; c0<ncols ; c0+=perPass)
				{
				const uint32_t cells = (ncols - c0 < perPass)? ncols - c0 : perPass;
				const uint32_t len   = cells * bin;                        // <= MX_STAGE
				const int64_t  gc    = g0 + (int64_t) c0 * bin;
				const bool     live  = cell < cells;
				const uint32_t j     = minus? ncols - 1 - (c0 + cell) : c0 + cell;
				if ((gc + len <= 0) || (gc >= n))                       // nothing of the stretch lies in the chromosome
					{
					if (live && (r == 0)) rowOut[j] = mx_empty<WHAT> ();
					continue;
					}
				for (uint32_t i0=0 ; i0<len ; i0+=64*MX_STAGE_DEPTH)
					{
					double x[MX_STAGE_DEPTH];
#pragma unroll
					for (int u=0 ; u<MX_STAGE_DEPTH ; u++)                 // (every lane loads, index clamped: see gdsp_stage_f64)
						{
						const int64_t g  = gc + i0 + u*64 + lane;
						const int64_t gi = (g < 0)? 0 : ((g >= n)? n - 1 : g);
						const double  y  = v[gi];
						x[u] = (g == gi)? y : NAN;
						}
#pragma unroll
					for (int u=0 ; u<MX_STAGE_DEPTH ; u++)
						{
						const uint32_t i = i0 + u*64 + lane;
						if (i < len) mine[i + (i >> 5)] = x[u];
						}
					}
				__builtin_amdgcn_fence (__ATOMIC_RELEASE, "wavefront");     // the wave's stores, then the wave's loads
				__builtin_amdgcn_wave_barrier ();
				__builtin_amdgcn_fence (__ATOMIC_ACQUIRE, "wavefront");

				MxAcc c;
				mx_clear<WHAT> (c);
				const uint32_t base = live? cell * bin : 0;
				for (uint32_t u=r ; u<bin ; u+=group)
					{
					const uint32_t i = base + u;
					mx_take<WHAT> (c, mine[i + (i >> 5)], lo, hi);
					}
				for (uint32_t off=1 ; off<group ; off<<=1)
					mx_fold<WHAT> (c, (int) off, (r & (2*off - 1)) == 0);
				bool later;
				const double y     = mx_finish<WHAT> (c, later);
				const bool   owner = live && (r == 0);
				if (owner) rowOut[j] = y;
				if ((WHAT == GDSP_MATRIX_SUM) || (WHAT == GDSP_MATRIX_MEAN)) mx_later_wave (todo, ntodo, owner && later, cell0 + j);
				__builtin_amdgcn_fence (__ATOMIC_RELEASE, "wavefront");     // the wave's loads, then the next stretch's stores
				__builtin_amdgcn_wave_barrier ();
				__builtin_amdgcn_fence (__ATOMIC_ACQUIRE, "wavefront");
				}
			}

		if (ROUTE == MX_ROUTE_WIDE)
			{
			for (uint32_t c0=0 ; c0<ncols ; c0++)
				{
				// offsets [tLo, tHi) of the window, cut to the chromosome
				int64_t tLo = (int64_t) c0 * bin, tHi = tLo + bin;
				if (tLo < -g0)    tLo = -g0;
				if (tHi > n - g0) tHi = n - g0;
				const uint32_t j = minus? ncols - 1 - c0 : c0;
				if (tLo >= tHi)
					{
					if (lane == 0) rowOut[j] = mx_empty<WHAT> ();
					continue;
					}
				MxAcc c, d;
				mx_clear<WHAT> (c);
				mx_clear<WHAT> (d);
				int64_t i = tLo + lane;
				for ( ; i+192<tHi ; i+=256)
					{
					const double x0 = v[g0+i], x1 = v[g0+i+64], x2 = v[g0+i+128], x3 = v[g0+i+192];
					mx_take<WHAT> (c, x0, lo, hi);  mx_take<WHAT> (d, x1, lo, hi);
					mx_take<WHAT> (c, x2, lo, hi);  mx_take<WHAT> (d, x3, lo, hi);
					}
				for ( ; i+64<tHi ; i+=128)
					{
					const double x0 = v[g0+i], x1 = v[g0+i+64];
					mx_take<WHAT> (c, x0, lo, hi);  mx_take<WHAT> (d, x1, lo, hi);
					}
				if (i < tHi) mx_take<WHAT> (c, v[g0+i], lo, hi);
				// the lane's two shares, then the wave's 64 as a tree
				if ((WHAT == GDSP_MATRIX_SUM) || (WHAT == GDSP_MATRIX_MEAN))
					{
#pragma unroll
					for (int k=0 ; k<XS_K ; k++) xs_grow_or_flag (c.a, d.a[k], c.flag);
					c.flag |= d.flag;
					}
				c.cnt += d.cnt;
				if (WHAT == GDSP_MATRIX_MIN) c.m = (d.m < c.m)? d.m : c.m;
				if (WHAT == GDSP_MATRIX_MAX) c.m = (d.m > c.m)? d.m : c.m;
				for (int off=1 ; off<64 ; off<<=1)
					mx_fold<WHAT> (c, off, (lane & (2*off - 1)) == 0);
				if (lane == 0)
					{
					bool later;
					rowOut[j] = mx_finish<WHAT> (c, later);
					if (later) mx_later (todo, ntodo, cell0 + j);
					}
				}
			}
		}
	}

// ---------------------------------------------------------------------------------------------- host ----
static uint32_t mxLaunchRows = 0;                            // see gdsp_matrix_set_launch_rows
static uint64_t mxLast[4];                                   // see gdsp_genome_matrix_last

static int mx_check_shape (int32_t offLo, uint32_t noffsets, uint32_t bin, int what, const char* who = __builtin_FUNCTION ())
	{
	const int rc = gdsp_anchor_check_offsets (offLo, noffsets, who);
	if (rc != GDSP_OK) return rc;
	if ((bin < 1) || (noffsets % bin != 0)) return gdsp_anchor_refuse (who, "the bin must divide the number of offsets");
	if ((what < GDSP_MATRIX_MEAN) || (what > GDSP_MATRIX_MAX)) return gdsp_anchor_refuse (who, "the figure is one of GDSP_MATRIX_*");
	return GDSP_OK;
	}

template <int WHAT>
static void mx_launch_route (const GdspAnchorTable& B, dim3 grid, hipStream_t s, const uint32_t* d_pos, const uint32_t* d_code, uint32_t count,
                             int32_t offLo, uint32_t noffsets, uint32_t bin, double lo, double hi, double* d_out, uint32_t* d_todo,
                             uint32_t* d_ntodo)
	{
	const uint32_t group = (bin < 16)? 1u : ((bin < 64)? 4u : 16u);
	if (bin == 1)
		hipLaunchKernelGGL ((matrix_kernel<WHAT, MX_ROUTE_COPY>), grid, dim3 (MX_THREADS), 0, s, B, d_pos, d_code, count, offLo, noffsets,
		                    bin, group, lo, hi, d_out, d_todo, d_ntodo);
	else if (bin < MX_NARROW_BELOW)
		hipLaunchKernelGGL ((matrix_kernel<WHAT, MX_ROUTE_NARROW>), grid, dim3 (MX_THREADS), 0, s, B, d_pos, d_code, count, offLo, noffsets,
		                    bin, group, lo, hi, d_out, d_todo, d_ntodo);
	else
		hipLaunchKernelGGL ((matrix_kernel<WHAT, MX_ROUTE_WIDE>), grid, dim3 (MX_THREADS), 0, s, B, d_pos, d_code, count, offLo, noffsets,
		                    bin, group, lo, hi, d_out, d_todo, d_ntodo);
	}

// the launch sequences of one call (arguments checked, every anchor inside its vector); *launches counts them
static int mx_launch (const gdsp_batch_item* items, int nitems, const uint32_t* d_pos, const uint32_t* d_code, uint32_t count,
                      int32_t offLo, uint32_t noffsets, uint32_t bin, int what, double lo, double hi, double* d_out,
                      uint32_t* d_todo, uint32_t* d_ntodo, hipStream_t s, uint64_t* launches)
	{
	static_assert ((MX_STAGE % 32 == 0) && (64 * 15 <= MX_STAGE) && (16 * 63 <= MX_STAGE) && (4 * (MX_NARROW_BELOW - 1) <= MX_STAGE), "a stretch holds 64 / G cells");
	const dim3 grid (std::min<uint32_t> ((count + MX_WAVES - 1) / MX_WAVES, MX_WG_TARGET));
	return gdsp_anchor_tables (items, nitems, [&] (const GdspAnchorTable& B) -> int
		{
		mx_with_figure (what, [&] (auto W)
			{ mx_launch_route<decltype (W)::value> (B, grid, s, d_pos, d_code, count, offLo, noffsets, bin, lo, hi, d_out, d_todo, d_ntodo); });
		GDSP_LAUNCH_CHECK ();
		if (launches != NULL) (*launches)++;
		return GDSP_OK;
		});
	}

extern "C" {

int gdsp_matrix_set_launch_rows (uint32_t rows) { mxLaunchRows = rows;  return GDSP_OK; }

void gdsp_genome_matrix_last (uint64_t out[4]) { memcpy (out, mxLast, sizeof(mxLast)); }

int gdsp_matrix_rows_batch (const gdsp_batch_item* items, int nitems, const uint32_t* d_pos, const uint32_t* d_code, uint32_t count,
                            int32_t offLo, uint32_t noffsets, uint32_t bin, int what, double lo, double hi, double* d_out,
                            uint32_t* d_todo, uint32_t* d_ntodo, void* stream)
	{
	int rc = mx_check_shape (offLo, noffsets, bin, what);
	if (rc != GDSP_OK) return rc;
	GDSP_REQUIRE (nitems >= 0, "a negative number of vectors");
	GDSP_REQUIRE ((nitems == 0) || (items != NULL), "NULL items");
	rc = gdsp_anchor_check_aligned (items, nitems);
	if (rc != GDSP_OK) return rc;
	GDSP_REQUIRE ((count == 0) || ((d_pos != NULL) && (d_code != NULL)), "NULL anchors");
	GDSP_REQUIRE ((count == 0) || (nitems > 0), "anchors without a vector");
	GDSP_REQUIRE ((count == 0) || ((d_out != NULL) && (d_todo != NULL) && (d_ntodo != NULL)), "NULL rows or to-do list");
	GDSP_REQUIRE ((uint64_t) count * (noffsets / bin) <= UINT32_MAX, "more than 2^32 - 1 cells in one call");
	hipStream_t s = gdsp_stream (stream);
	if (count == 0) return GDSP_OK;

	rc = gdsp_anchor_check (items, nitems, d_pos, d_code, count, s, __func__);     // on the device, where the anchors are
	if (rc != GDSP_OK) return rc;
	return mx_launch (items, nitems, d_pos, d_code, count, offLo, noffsets, bin, what, lo, hi, d_out, d_todo, d_ntodo, s, NULL);
	}

} // extern "C"

// ------------------------------------------------------------------------------------------- end to end ----
namespace {

// the current device's sources mine[0 .. nmine) (indices into `sources`, the caller's order) and all their rows
int mx_on_device (const gdsp_profile_source* sources, const int* mine, int nmine, int32_t offLo, uint32_t noffsets, uint32_t bin,
                  int what, double lo, double hi, double* const* h_rows)
	{
	std::vector<gdsp_batch_item> items;
	std::vector<uint64_t> first (nmine + 1, 0);                   // the device's rows: source k owns first[k] .. first[k+1]
	std::vector<uint32_t> cols[2];                                // the positions, the code words
	const std::vector<uint32_t> &pos = cols[0], &code = cols[1];
	gdsp_anchor_gather (sources, mine, nmine, items, cols[0], cols[1], first.data ());
	if (first[nmine] == 0) return GDSP_OK;
	GDSP_REQUIRE (first[nmine] <= UINT32_MAX, "more than 2^32 - 1 anchors on a device");
	return mx_rows_on_device (items, first, mine, cols, noffsets / bin, what, lo, hi, h_rows, mxLaunchRows, mxLast,
	                          sources[mine[0]].stream, "gdsp_genome_matrix", "anchors",
		[&] (const uint32_t* d_rows, uint64_t na, uint32_t nr, double* d_out, uint32_t* d_todo, uint32_t* d_ntodo, hipStream_t s, uint64_t* launches) -> int
			{ return mx_launch (items.data (), nmine, d_rows, d_rows + na, nr, offLo, noffsets, bin, what, lo, hi, d_out, d_todo, d_ntodo, s, launches); },
		[&] (uint64_t a, uint32_t j, int64_t n, int64_t* gLo, int64_t* gHi)
			{
			// the offsets kLo .. kHi of column j, from the anchor in its own direction, cut to the chromosome
			const int64_t p = pos[a], kLo = (int64_t) offLo + (int64_t) j * bin, kHi = kLo + bin - 1;
			*gLo = std::max<int64_t> (gdsp_anchor_minus (code[a])? p - kHi : p + kLo, 0);
			*gHi = std::min<int64_t> (gdsp_anchor_minus (code[a])? p - kLo : p + kHi, n - 1) + 1;
			});
	}

} // namespace

extern "C" {

int gdsp_genome_matrix (const gdsp_profile_source* sources, int nsources, int32_t offLo, uint32_t noffsets, uint32_t bin, int what,
                        double lo, double hi, double* const* h_rows)
	{
	GDSP_REQUIRE (nsources >= 0, "a negative number of sources");
	GDSP_REQUIRE ((nsources == 0) || ((sources != NULL) && (h_rows != NULL)), "NULL sources or rows");
	int rc = mx_check_shape (offLo, noffsets, bin, what);
	if (rc != GDSP_OK) return rc;
	memset (mxLast, 0, sizeof(mxLast));
	const uint32_t ncols = noffsets / bin;
	rc = gdsp_anchor_check_sources (sources, nsources, [&, who = __func__] (int i) -> int
		{
		if ((sources[i].nanchors != 0) && ((sources[i].h_pos == NULL) || (h_rows[i] == NULL))) return gdsp_anchor_refuse (who, "NULL anchors or rows");
		if ((sources[i].n != 0) && ((sources[i].d_v == NULL) || ((((uintptr_t) sources[i].d_v) & 7) != 0))) return gdsp_anchor_refuse (who, "a vector must be 8-byte aligned");
		return GDSP_OK;
		}, &mxLast[0]);
	if (rc != GDSP_OK) return rc;
	mxLast[1] = mxLast[0] * ncols;
	return gdsp_anchor_per_device (sources, nsources, __func__, [&] (const int* mine, int nmine) -> int
		{ return mx_on_device (sources, mine, nmine, offLo, noffsets, bin, what, lo, hi, h_rows); });
	}

} // extern "C"
