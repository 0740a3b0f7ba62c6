// gdsp_regionsover.hip -- regionsover (not in the reference): every region of a list scaled to the same columns, one row
// per region (include/genodsp_hip.h has the definitions): U / b columns of unscaled flank upstream, B columns over the
// region's own L bases, D / b columns of flank downstream -- deepTools' computeMatrix scale-regions.  A cell is one interval
// of its chromosome and its figure is statsover's for that interval, as in matrixover; what is new is that the width of a
// body cell, floor (L / B) or ceil (L / B), changes from row to row.
//
// A wave takes whole regions, by stride over the launch's rows.  In ascending base order a row is three segments -- the low
// flank, the body, the high flank -- whatever the strand: the strand only decides which flank is which and which column a
// cell lands in (a minus region's ascending cell c is column ncols - 1 - c).  rg_bound gives the ascending bound of cell c
// of a segment, on the device and for the host's to-do cells alike.  It divides nothing in 64 bits: with L = qL B + rL,
// floor (c L / B) = c qL + floor (c rL / B), and for c <= B <= 16384 the first product is at most L < 2^32 and the second
// below 2^28 -- two 32-bit multiplications and one 32-bit division per bound, and bounds are asked for per cell, never per base.
// Each segment takes one of matrixover's three routes, uniform over the wave, by its widest cell w (b, or ceil (L / B)):
//   w == 1     a copy: lane l looks at cell l, which has one base or (a body with L < B) none.
//   w < 256    the wave stages a stretch of 64 / G cells -- the bases between the first cell's lower bound and the last
//              cell's upper bound -- in its own padded piece of LDS, and a group of G lanes (1 below 16 bases, 4 below 64,
//              else 16) owns a cell, whose [lo, hi) inside the stretch each group reads from rg_bound.
//   otherwise  the wave strides over the cell and folds its 64 lanes with the shuffle tree.
// The cell -- MxAcc, mx_take, mx_fold, mx_finish with its proof, the to-do list -- is gdsp_matrix_cell.h's, shared with
// matrixover, as are the sizes of a stretch; the host half of a device's rows is gdsp_matrix_rows.h's and the check on the
// device that every region lies inside its vector gdsp_anchors.hip's.  One double is written per cell, by one lane; no
// atomics on cells; one atomic per wave and stretch for the to-do list; no wave or workgroup waits for another (the LDS
// piece is a wave's own); no scratch.

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

// ---------------------------------------------------------------------------------- the geometry of a row ----
struct RgShape { uint32_t B, b, nUp, nDown, ncols; };       // body columns, bases of a flank column, flank columns

// a region [s, e) of L bases: L = qL B + rL; nLow flank cells from base lowBase below it, nHigh from e above it
struct RgRow { int64_t s, e, lowBase;  uint32_t L, qL, rL, nLow, nHigh;  bool minus; };

enum { RG_LOW = 0, RG_BODY = 1, RG_HIGH = 2 };

__host__ __device__ __forceinline__ RgShape rg_shape (uint32_t B, uint32_t U, uint32_t D, uint32_t b)
	{
	RgShape S;
	S.B = B;  S.b = b;  S.nUp = U / b;  S.nDown = D / b;  S.ncols = S.nUp + B + S.nDown;
	return S;
	}

__host__ __device__ __forceinline__ RgRow rg_row (const RgShape& S, int64_t s, int64_t e, bool minus)
	{
	RgRow R;
	R.s = s;  R.e = e;  R.minus = minus;
	R.L  = (uint32_t) (e - s);                                // (s < e <= n < 2^32)
	R.qL = R.L / S.B;  R.rL = R.L % S.B;
	R.nLow  = minus? S.nDown : S.nUp;                         // a minus region has its downstream flank below it
	R.nHigh = minus? S.nUp : S.nDown;
	R.lowBase = s - (int64_t) R.nLow * S.b;
	return R;
	}

__host__ __device__ __forceinline__ uint32_t rg_cells (const RgShape& S, const RgRow& R, int seg)
	{ return (seg == RG_BODY)? S.B : ((seg == RG_LOW)? R.nLow : R.nHigh); }

// floor (c L / B), 0 <= c <= B
__host__ __device__ __forceinline__ uint32_t rg_scaled (const RgShape& S, const RgRow& R, uint32_t c)
	{ return c * R.qL + (c * R.rL) / S.B; }

// the ascending lower bound of cell c of a segment (c = the segment's cells: the last cell's upper bound), before any
// cut to the chromosome.  Body, plus strand: s + floor (c L / B); minus strand, the mirror image: e - floor ((B - c) L / B)
__host__ __device__ __forceinline__ int64_t rg_bound (const RgShape& S, const RgRow& R, int seg, uint32_t c)
	{
	if (seg == RG_LOW)  return R.lowBase + (int64_t) c * S.b;
	if (seg == RG_HIGH) return R.e + (int64_t) c * S.b;
	return R.minus? R.e - (int64_t) rg_scaled (S, R, S.B - c) : R.s + (int64_t) rg_scaled (S, R, c);
	}

// ascending cell c of the whole row -> its segment and its index there
__host__ __device__ __forceinline__ int rg_segment_of (const RgShape& S, const RgRow& R, uint32_t c, uint32_t* within)
	{
	if (c < R.nLow) { *within = c;  return RG_LOW; }
	if (c < R.nLow + S.B) { *within = c - R.nLow;  return RG_BODY; }
	*within = c - R.nLow - S.B;
	return RG_HIGH;
	}

// column j of the row as the bases [*lo, *hi) of a chromosome of n bases (lo >= hi: none)
__host__ __device__ __forceinline__ void rg_column (const RgShape& S, const RgRow& R, int64_t n, uint32_t j, int64_t* lo, int64_t* hi)
	{
	uint32_t within;
	const int seg = rg_segment_of (S, R, R.minus? S.ncols - 1 - j : j, &within);
	const int64_t a = rg_bound (S, R, seg, within), z = rg_bound (S, R, seg, within + 1);
	*lo = (a < 0)? 0 : a;
	*hi = (z > n)? n : z;
	}

// ---------------------------------------------------------------------------------------------- the kernel ----
// one segment of one row, by the whole wave.  c0Row: the ascending index of the segment's first cell in the row
template <int WHAT>
__device__ __forceinline__ void rg_segment (const double* __restrict__ v, int64_t n, const RgShape& S, const RgRow& R, int seg,
                                            uint32_t c0Row, uint32_t w, double lo, double hi, double* __restrict__ rowOut,
                                            uint32_t cell0, double* __restrict__ mine, uint32_t* __restrict__ todo,
                                            uint32_t* __restrict__ ntodo)
	{
	const uint32_t lane   = threadIdx.x & 63;
	const uint32_t ncells = rg_cells (S, R, seg);
	if (ncells == 0) return;

	if (w == 1)                                                       // ---- the copy: a cell is one base or none
		{
		for (uint32_t t=lane ; t<ncells ; t+=64)
			{
			const int64_t g  = rg_bound (S, R, seg, t);
			const bool    in = (rg_bound (S, R, seg, t + 1) > g) && (g >= 0) && (g < n);
			const double  x  = in? v[g] : NAN;
			const bool    take = !(x < lo) && !(x > hi) && xs_finite (x);
			const uint32_t c = c0Row + t;
			const uint32_t j = R.minus? S.ncols - 1 - c : c;
			double y;
			if      (WHAT == GDSP_MATRIX_COUNT) y = take? 1.0 : 0.0;
			else if (WHAT == GDSP_MATRIX_SUM)   y = take? __dadd_rn (x, 0.0) : 0.0;
			else                                y = take? __dadd_rn (x, 0.0) : NAN;     // (one value is its own mean, min and max)
			rowOut[j] = y;
			}
		return;
		}

	if (w < MX_NARROW_BELOW)                                          // ---- the wave's own stretch of LDS
		{
		// A stretch of c cells is the bases between two bounds c cells apart: at most c w of them, w the widest cell of the
		// segment (b, or ceil (L / B)).  With 64 / G cells of at most 15, 63 and 255 bases, MX_STAGE holds it, as it does
		// matrixover's stretch of 64 / G cells of exactly b bases.
		static_assert ((MX_STAGE % 32 == 0) && (64 * 15 <= MX_STAGE) && (16 * 63 <= MX_STAGE) && (4 * (MX_NARROW_BELOW - 1) <= MX_STAGE), "a stretch holds 64 / G cells");
		const uint32_t group   = (w < 16)? 1u : ((w < 64)? 4u : 16u);
		const uint32_t perPass = 64 / group;
		const uint32_t cell = lane / group, r = lane % group;
		for (uint32_t c0=0 ; c0<ncells ; c0+=perPass)
			{
			const uint32_t cells = (ncells - c0 < perPass)? ncells - c0 : perPass;
			const int64_t  gc    = rg_bound (S, R, seg, c0);
			const uint32_t len   = (uint32_t) (rg_bound (S, R, seg, c0 + cells) - gc);      // <= cells * w <= MX_STAGE
			const bool     live  = cell < cells;
			const uint32_t c     = c0Row + c0 + cell;
			const uint32_t j     = R.minus? S.ncols - 1 - c : c;
			if ((gc + len <= 0) || (gc >= n) || (len == 0))             // nothing of the stretch lies in the chromosome
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

			// the group's own cell, as offsets [base, base + width) into the stretch
			const uint32_t cc    = live? c0 + cell : c0;
			const uint32_t base  = (uint32_t) (rg_bound (S, R, seg, cc) - gc);
			const uint32_t width = live? (uint32_t) (rg_bound (S, R, seg, cc + 1) - gc) - base : 0;
			MxAcc a;
			mx_clear<WHAT> (a);
			for (uint32_t u=r ; u<width ; u+=group)
				{
				const uint32_t i = base + u;
				mx_take<WHAT> (a, mine[i + (i >> 5)], lo, hi);
				}
			for (uint32_t off=1 ; off<group ; off<<=1)
				mx_fold<WHAT> (a, (int) off, (r & (2*off - 1)) == 0);
			bool later;
			const double y     = mx_finish<WHAT> (a, later);
			const bool   owner = live && (r == 0);
			if (owner) rowOut[j] = y;
			if ((WHAT == GDSP_MATRIX_SUM) || (WHAT == GDSP_MATRIX_MEAN)) mx_later_wave (todo, ntodo, owner && later, cell0 + j);
			__builtin_amdgcn_fence (__ATOMIC_RELEASE, "wavefront");     // the wave's loads, then the next stretch's stores
			__builtin_amdgcn_wave_barrier ();
			__builtin_amdgcn_fence (__ATOMIC_ACQUIRE, "wavefront");
			}
		return;
		}

	for (uint32_t c0=0 ; c0<ncells ; c0++)                            // ---- the wave strides over the cell
		{
		int64_t tLo = rg_bound (S, R, seg, c0), tHi = rg_bound (S, R, seg, c0 + 1);
		if (tLo < 0) tLo = 0;
		if (tHi > n) tHi = n;
		const uint32_t c = c0Row + c0;
		const uint32_t j = R.minus? S.ncols - 1 - c : c;
		if (tLo >= tHi)
			{
			if (lane == 0) rowOut[j] = mx_empty<WHAT> ();
			continue;
			}
		MxAcc a, d;
		mx_clear<WHAT> (a);
		mx_clear<WHAT> (d);
		int64_t i = tLo + lane;
		for ( ; i+192<tHi ; i+=256)
			{
			const double x0 = v[i], x1 = v[i+64], x2 = v[i+128], x3 = v[i+192];
			mx_take<WHAT> (a, x0, lo, hi);  mx_take<WHAT> (d, x1, lo, hi);
			mx_take<WHAT> (a, x2, lo, hi);  mx_take<WHAT> (d, x3, lo, hi);
			}
		for ( ; i+64<tHi ; i+=128)
			{
			const double x0 = v[i], x1 = v[i+64];
			mx_take<WHAT> (a, x0, lo, hi);  mx_take<WHAT> (d, x1, lo, hi);
			}
		if (i < tHi) mx_take<WHAT> (a, v[i], lo, hi);
		// the lane's two shares, then the wave's 64 as a tree
		if ((WHAT == GDSP_MATRIX_SUM) || (WHAT == GDSP_MATRIX_MEAN))
			{
#pragma unroll
			for (int k=0 ; k<XS_K ; k++) xs_grow_or_flag (a.a, d.a[k], a.flag);
			a.flag |= d.flag;
			}
		a.cnt += d.cnt;
		if (WHAT == GDSP_MATRIX_MIN) a.m = (d.m < a.m)? d.m : a.m;
		if (WHAT == GDSP_MATRIX_MAX) a.m = (d.m > a.m)? d.m : a.m;
		for (int off=1 ; off<64 ; off<<=1)
			mx_fold<WHAT> (a, off, (lane & (2*off - 1)) == 0);
		if (lane == 0)
			{
			bool later;
			rowOut[j] = mx_finish<WHAT> (a, later);
			if (later) mx_later (todo, ntodo, cell0 + j);
			}
		}
	}

template <int WHAT>
__global__ __launch_bounds__(MX_THREADS)
void regions_kernel (GdspAnchorTable P, const uint32_t* __restrict__ d_start, const uint32_t* __restrict__ d_end,
                     const uint32_t* __restrict__ d_code, uint32_t count, RgShape S, double lo, double hi,
                     double* __restrict__ out, uint32_t* __restrict__ todo, uint32_t* __restrict__ ntodo)
	{
	__shared__ double stage[MX_WAVES * MX_STAGE_PAD];
	const uint32_t wave  = threadIdx.x >> 6;
	const uint32_t nwave = gridDim.x * MX_WAVES;
	double* __restrict__ mine = stage + wave * MX_STAGE_PAD;

	for (uint32_t row=blockIdx.x*MX_WAVES+wave ; row<count ; row+=nwave)
		{
		const uint32_t code = __builtin_amdgcn_readfirstlane (d_code[row]);
		const uint32_t vec  = gdsp_anchor_vec (code) - P.vec0;
		if (vec >= P.nvec) continue;                                  // (a vector of another launch sequence)
		const double* __restrict__ v = P.v[vec];
		const int64_t n = (int64_t) P.n[vec];
		// (the builtin returns int: unsigned again before it widens, or a position from 2^31 on turns negative)
		const int64_t s = (int64_t) (uint32_t) __builtin_amdgcn_readfirstlane (d_start[row]);
		const int64_t e = (int64_t) (uint32_t) __builtin_amdgcn_readfirstlane (d_end[row]);
		const RgRow   R = rg_row (S, s, e, gdsp_anchor_minus (code));
		const uint32_t cell0 = row * S.ncols;                         // (the call's cells fit 32 bits: the host half sees to it)
		double* __restrict__ rowOut = out + (size_t) row * S.ncols;
		const uint32_t wBody = R.qL + ((R.rL != 0)? 1u : 0u);         // ceil (L / B): the widest body cell
#pragma unroll 1
		for (int seg=RG_LOW ; seg<=RG_HIGH ; seg++)                    // (one copy of the three routes, not three)
			{
			const uint32_t c0Row = (seg == RG_LOW)? 0 : ((seg == RG_BODY)? R.nLow : R.nLow + S.B);
			rg_segment<WHAT> (v, n, S, R, seg, c0Row, (seg == RG_BODY)? wBody : S.b, lo, hi, rowOut, cell0, mine, todo, ntodo);
			}
		}
	}

// ---------------------------------------------------------------------------------------------- host ----
static uint32_t rgLaunchRows = 0;                            // see gdsp_regions_set_launch_rows
static uint64_t rgLast[4];                                   // see gdsp_genome_regions_last

static int rg_check_shape (uint32_t B, uint32_t U, uint32_t D, uint32_t b, int what, const char* who = __builtin_FUNCTION ())
	{
	if ((B < 1) || (B > GDSP_REGIONS_MAX_COLUMNS)) return gdsp_anchor_refuse (who, "the body must have 1 .. 16384 columns");
	if ((U > GDSP_REGIONS_MAX_COLUMNS) || (D > GDSP_REGIONS_MAX_COLUMNS)) return gdsp_anchor_refuse (who, "a flank must be at most 16384 bases");
	if ((b < 1) || (U % b != 0) || (D % b != 0)) return gdsp_anchor_refuse (who, "the bin must divide both flanks");
	if ((uint64_t) U / b + B + (uint64_t) D / b > GDSP_REGIONS_MAX_COLUMNS) return gdsp_anchor_refuse (who, "a row must have at most 16384 columns");
	if ((what < GDSP_MATRIX_MEAN) || (what > GDSP_MATRIX_MAX)) return gdsp_anchor_refuse (who, "the figure is one of GDSP_MATRIX_*");
	return GDSP_OK;
	}

// the launch sequences of one call (arguments checked, every region inside its vector); *launches counts them
static int rg_launch (const gdsp_batch_item* items, int nitems, const uint32_t* d_start, const uint32_t* d_end, const uint32_t* d_code,
                      uint32_t count, const RgShape& S, int what, double lo, double hi, double* d_out, uint32_t* d_todo,
                      uint32_t* d_ntodo, hipStream_t s, uint64_t* launches)
	{
	const dim3 grid (std::min<uint32_t> ((count + MX_WAVES - 1) / MX_WAVES, MX_WG_TARGET)), block (MX_THREADS);
	return gdsp_anchor_tables (items, nitems, [&] (const GdspAnchorTable& T) -> int
		{
		mx_with_figure (what, [&] (auto W)
			{ hipLaunchKernelGGL (regions_kernel<decltype (W)::value>, grid, block, 0, s, T, d_start, d_end, d_code, count, S, lo, hi, d_out, d_todo, d_ntodo); });
		GDSP_LAUNCH_CHECK ();
		if (launches != NULL) (*launches)++;
		return GDSP_OK;
		});
	}

extern "C" {

int gdsp_regions_set_launch_rows (uint32_t rows) { rgLaunchRows = rows;  return GDSP_OK; }

void gdsp_genome_regions_last (uint64_t out[4]) { memcpy (out, rgLast, sizeof(rgLast)); }

int gdsp_region_cell_bounds (uint32_t n, uint32_t start, uint32_t end, int minus, uint32_t B, uint32_t U, uint32_t D, uint32_t b,
                             uint32_t column, int64_t* lo, int64_t* hi)
	{
	const int rc = rg_check_shape (B, U, D, b, GDSP_MATRIX_MEAN);
	if (rc != GDSP_OK) return rc;
	GDSP_REQUIRE ((lo != NULL) && (hi != NULL), "NULL bounds");
	GDSP_REQUIRE ((start < end) && (end <= n), "a region is empty or lies outside its vector");
	const RgShape S = rg_shape (B, U, D, b);
	GDSP_REQUIRE (column < S.ncols, "no such column");
	rg_column (S, rg_row (S, start, end, minus != 0), n, column, lo, hi);
	return GDSP_OK;
	}

int gdsp_region_rows_batch (const gdsp_batch_item* items, int nitems, const uint32_t* d_start, const uint32_t* d_end,
                            const uint32_t* d_code, uint32_t count, uint32_t B, uint32_t U, uint32_t D, uint32_t b, int what,
                            double lo, double hi, double* d_out, uint32_t* d_todo, uint32_t* d_ntodo, void* stream)
	{
	int rc = rg_check_shape (B, U, D, b, what);
	if (rc != GDSP_OK) return rc;
	GDSP_REQUIRE (nitems >= 0, "a negative number of vectors");
	GDSP_REQUIRE ((nitems == 0) || (items != NULL), "NULL items");
	rc = gdsp_anchor_check_aligned (items, nitems);
	if (rc != GDSP_OK) return rc;
	GDSP_REQUIRE ((count == 0) || ((d_start != NULL) && (d_end != NULL) && (d_code != NULL)), "NULL regions");
	GDSP_REQUIRE ((count == 0) || (nitems > 0), "regions without a vector");
	GDSP_REQUIRE ((count == 0) || ((d_out != NULL) && (d_todo != NULL) && (d_ntodo != NULL)), "NULL rows or to-do list");
	const RgShape S = rg_shape (B, U, D, b);
	GDSP_REQUIRE ((uint64_t) count * S.ncols <= UINT32_MAX, "more than 2^32 - 1 cells in one call");
	hipStream_t s = gdsp_stream (stream);
	if (count == 0) return GDSP_OK;

	rc = gdsp_region_check (items, nitems, d_start, d_end, d_code, count, s, __func__);     // on the device, where the regions are
	if (rc != GDSP_OK) return rc;
	return rg_launch (items, nitems, d_start, d_end, d_code, count, S, what, lo, hi, d_out, d_todo, d_ntodo, s, NULL);
	}

} // extern "C"

// ------------------------------------------------------------------------------------------- end to end ----
namespace {

// the current device's sources mine[0 .. nmine) (indices into `sources`, the caller's order) and all their rows
int rg_on_device (const gdsp_region_source* sources, const int* mine, int nmine, const RgShape& S, int what, double lo, double hi,
                  double* const* h_rows)
	{
	std::vector<gdsp_batch_item> items;
	std::vector<uint64_t> first (nmine + 1, 0);                   // the device's rows: source k owns first[k] .. first[k+1]
	std::vector<uint32_t> cols[3];                                // the starts, the ends, the code words
	std::vector<uint32_t> &start = cols[0], &end = cols[1], &code = cols[2];
	for (int k=0 ; k<nmine ; k++)
		{
		const gdsp_region_source& Q = sources[mine[k]];
		items.push_back (gdsp_batch_item ());                    // (all zero)
		items.back ().d_in = Q.d_v;  items.back ().n = Q.n;
		for (uint32_t a=0 ; a<Q.nregions ; a++)
			{
			start.push_back (Q.h_start[a]);  end.push_back (Q.h_end[a]);
			code.push_back (gdsp_anchor_code ((uint32_t) k, (Q.h_minus != NULL) && (Q.h_minus[a] != 0)));
			}
		first[k+1] = first[k] + Q.nregions;
		}
	if (first[nmine] == 0) return GDSP_OK;
	GDSP_REQUIRE (first[nmine] <= UINT32_MAX, "more than 2^32 - 1 regions on a device");
	return mx_rows_on_device (items, first, mine, cols, S.ncols, what, lo, hi, h_rows, rgLaunchRows, rgLast,
	                          sources[mine[0]].stream, "gdsp_genome_regions", "regions",
		[&] (const uint32_t* d_rows, uint64_t na, uint32_t nr, double* d_out, uint32_t* d_todo, uint32_t* d_ntodo, hipStream_t s, uint64_t* launches) -> int
			{ return rg_launch (items.data (), nmine, d_rows, d_rows + na, d_rows + 2 * na, nr, S, what, lo, hi, d_out, d_todo, d_ntodo, s, launches); },
		[&] (uint64_t a, uint32_t j, int64_t n, int64_t* gLo, int64_t* gHi)       // (by the kernel's own rg_bound)
			{ rg_column (S, rg_row (S, start[a], end[a], gdsp_anchor_minus (code[a])), n, j, gLo, gHi); });
	}

} // namespace

extern "C" {

int gdsp_genome_regions (const gdsp_region_source* sources, int nsources, uint32_t B, uint32_t U, uint32_t D, uint32_t b, int what,
                         double lo, double hi, double* const* h_rows)
	{
	GDSP_REQUIRE (nsources >= 0, "a negative number of sources");
	GDSP_REQUIRE ((nsources == 0) || ((sources != NULL) && (h_rows != NULL)), "NULL sources or rows");
	int rc = rg_check_shape (B, U, D, b, what);
	if (rc != GDSP_OK) return rc;
	memset (rgLast, 0, sizeof(rgLast));
	const RgShape S = rg_shape (B, U, D, b);
	for (int i=0 ; i<nsources ; i++)
		{
		const gdsp_region_source& Q = sources[i];
		if ((Q.nregions != 0) && ((Q.h_start == NULL) || (Q.h_end == NULL) || (h_rows[i] == NULL))) return gdsp_anchor_refuse (__func__, "NULL regions or rows");
		if ((Q.n != 0) && ((Q.d_v == NULL) || ((((uintptr_t) Q.d_v) & 7) != 0))) return gdsp_anchor_refuse (__func__, "a vector must be 8-byte aligned");
		for (uint32_t k=0 ; k<Q.nregions ; k++)
			if (!((Q.h_start[k] < Q.h_end[k]) && (Q.h_end[k] <= Q.n))) return gdsp_anchor_refuse (__func__, "a region is empty or lies outside its vector");
		rgLast[0] += Q.nregions;
		}
	rgLast[1] = rgLast[0] * S.ncols;
	return gdsp_anchor_per_device (sources, nsources, __func__, [&] (const int* mine, int nmine) -> int
		{ return rg_on_device (sources, mine, nmine, S, what, lo, hi, h_rows); });
	}

} // extern "C"
