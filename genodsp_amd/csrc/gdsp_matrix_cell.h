// gdsp_matrix_cell.h -- the cell of the matrix operators (gdsp_matrixover.hip: matrixover, cells of one bin width around
// anchors; gdsp_regionsover.hip: regionsover, cells whose width changes with the row): what a lane knows of its sample,
// how lanes fold their shares, and how a cell's figure is finished exactly and rounded once -- or handed to the host, by
// its index on the launch's to-do list.  The routes that feed a cell stay with the kernels; what the host does with the
// rows and the list is gdsp_matrix_rows.h's.
#pragma once
#include <math.h>
#include "gdsp_common.h"
#include "gdsp_xsum_dev.h"

// the shape of a launch and of a wave's stretch of LDS, the same for both kernels
#define MX_THREADS      256
#define MX_WAVES        (MX_THREADS / 64)
#define MX_STAGE        1024                          // doubles of a wave's stretch: 64 cells of up to 15, 16 of up to 63, 4 of up to 255
#define MX_STAGE_PAD    (MX_STAGE + MX_STAGE / 32)
#define MX_STAGE_DEPTH  8                             // loads a lane issues before its first LDS store
#define MX_WG_TARGET    2048                          // workgroups of a launch (33 KiB of LDS each: four on a CU)
#define MX_LAUNCH_CELLS (1u << 25)                    // cells of one launch of the host half (256 MiB of rows)

#define MX_NARROW_BELOW 256                           // bins from here on take the wide route

// what a lane (then a group, then a cell) knows of its sample
struct MxAcc { double a[XS_K];  double m;  uint32_t cnt, flag; };

template <int WHAT>
__device__ __forceinline__ void mx_clear (MxAcc& c)
	{
	c.a[0] = c.a[1] = 0.0;  c.cnt = 0;  c.flag = 0;
	c.m = (WHAT == GDSP_MATRIX_MIN)? HUGE_VAL : -HUGE_VAL;
	}

template <int WHAT>
__device__ __forceinline__ void mx_take (MxAcc& c, double x, double lo, double hi)
	{
	const bool in = !(x < lo) && !(x > hi) && xs_finite (x);          // stats' tests; NaN and +-inf never
	if ((WHAT == GDSP_MATRIX_SUM) || (WHAT == GDSP_MATRIX_MEAN)) xs_grow_or_flag (c.a, in? x : 0.0, c.flag);
	if ((WHAT == GDSP_MATRIX_COUNT) || (WHAT == GDSP_MATRIX_MEAN)) c.cnt += in? 1u : 0u;
	if (WHAT == GDSP_MATRIX_MIN) c.m = (in && (x < c.m))? x : c.m;
	if (WHAT == GDSP_MATRIX_MAX) c.m = (in && (x > c.m))? x : c.m;
	}

// lane l takes lane l + off's share when `mine`
template <int WHAT>
__device__ __forceinline__ void mx_fold (MxAcc& c, int off, bool mine)
	{
	if ((WHAT == GDSP_MATRIX_SUM) || (WHAT == GDSP_MATRIX_MEAN))
		{
		double tt[XS_K];
#pragma unroll
		for (int j=0 ; j<XS_K ; j++) tt[j] = __shfl_down (c.a[j], off, 64);
#pragma unroll
		for (int j=0 ; j<XS_K ; j++) xs_grow_or_flag (c.a, mine? tt[j] : 0.0, c.flag);
		const uint32_t of = __shfl_down (c.flag, off, 64);
		c.flag |= mine? of : 0u;
		}
	if ((WHAT == GDSP_MATRIX_COUNT) || (WHAT == GDSP_MATRIX_MEAN))
		{
		const uint32_t oc = __shfl_down (c.cnt, off, 64);
		c.cnt += mine? oc : 0u;
		}
	if ((WHAT == GDSP_MATRIX_MIN) || (WHAT == GDSP_MATRIX_MAX))
		{
		const double om = __shfl_down (c.m, off, 64);
		const bool better = (WHAT == GDSP_MATRIX_MIN)? (om < c.m) : (om > c.m);
		c.m = (mine && better)? om : c.m;
		}
	}

// the cell's figure; `later` when the host has to compute it
template <int WHAT>
__device__ __forceinline__ double mx_finish (const MxAcc& c, bool& later)
	{
	later = false;
	if (WHAT == GDSP_MATRIX_COUNT) return (double) c.cnt;
	if (WHAT == GDSP_MATRIX_MIN) return (c.m ==  HUGE_VAL)? NAN : __dadd_rn (c.m, 0.0);     // (-0.0 + 0.0 is +0.0)
	if (WHAT == GDSP_MATRIX_MAX) return (c.m == -HUGE_VAL)? NAN : __dadd_rn (c.m, 0.0);
	// a0 + a1 is the exact sum: s is it rounded once, e what the rounding left
	const double s  = __dadd_rn (c.a[0], c.a[1]);
	const double bp = __dsub_rn (s, c.a[0]);
	const double e  = __dadd_rn (__dsub_rn (c.a[0], __dsub_rn (s, bp)), __dsub_rn (c.a[1], bp));
	if (WHAT == GDSP_MATRIX_SUM)
		{
		later = (c.flag != 0) || !xs_finite (s);
		return later? NAN : __dadd_rn (s, 0.0);
		}
	if (c.cnt == 0) return NAN;                                          // (only +0.0 was added: nothing is flagged)
	later = (c.flag != 0) || !xs_finite (s);
	const double n = (double) c.cnt;                                     // an integer below 2^32: exact
	const double q = __ddiv_rn (s, n);
	// e == 0: the exact sum is the double s, so the division's operands are exact and q is the exact quotient rounded once
	if (later || (e == 0.0)) return later? NAN : q;
	// a count that is a power of two: dividing by it moves the exponent alone (s is far from the subnormals), so rounding
	// and dividing commute and S / n rounded once is s / n.  (Half of these are ties the test below would give away.)
	const uint32_t sExp = (uint32_t) ((unsigned long long) __double_as_longlong (s) >> 52) & 0x7FF;
	if (((c.cnt & (c.cnt - 1)) == 0) && (sExp >= 128)) return q;
	// The exact sum is S = s + e with e != 0, |e| <= ulp(s)/2, and the mean is S / n.  Take a candidate q1 -- q moved by
	// the remainder it left, fl(fl(r + e) / n) with r = s - q n from one fma; how good that step is decides only how
	// often the test below passes, not what it proves -- and test the candidate itself:
	//   r1 = fma (-q1, n, s) is s - q1 n EXACTLY.  q1 lies within three ulps of s / n, so |s - q1 n| <= 3 ulp(q1) n, and
	//   the value is a multiple of ulp(q1): q1 n is one, and s is a multiple of ulp(s) >= ulp(q1) because |q1| <= |s|
	//   up to that rounding.  A multiple of ulp(q1) below 2^34 ulp(q1) is a double (everything here is far from the
	//   subnormals and from overflow: the exponents of s and q1 are held to 128 .. 1900 of 2047), so the fma rounds nothing.
	//   (An fma that did round would have met a remainder of 2^53 ulp(q1) or more, which fails the test below: nothing
	//   is accepted on the strength of the candidate being close.)
	//   Then S / n - q1 = (r1 + e) / n, and q1 is S / n rounded to nearest iff |r1 + e| < h n, h = ulp(q1)/2, provided q1
	//   is not a power of two (below one the doubles lie twice as dense, and the bound on that side would be h/2).
	//   h n is exact (a power of two times an integer below 2^32).  t = fl(r1 + e) is off by at most 2^-53 of itself, and
	//   so is the product with 1 - 2^-40: t < fl(h n (1 - 2^-40)) implies |r1 + e| < h n strictly.  A tie, |r1 + e| = h n,
	//   and everything within 2^-40 of one fails the test and goes to the host, as does a power of two.
	const double r  = __fma_rn (-q, n, s);
	const double q1 = __dadd_rn (q, __ddiv_rn (__dadd_rn (r, e), n));
	const double r1 = __fma_rn (-q1, n, s);
	const double t  = fabs (__dadd_rn (r1, e));
	const unsigned long long qb = (unsigned long long) __double_as_longlong (q1), sb = (unsigned long long) __double_as_longlong (s);
	const uint32_t qe = (uint32_t) (qb >> 52) & 0x7FF, se = (uint32_t) (sb >> 52) & 0x7FF;
	const bool inRange = (qe >= 128) && (qe <= 1900) && (se >= 128) && (se <= 1900) && ((qb & 0xFFFFFFFFFFFFFull) != 0);
	const double h = __longlong_as_double ((long long) ((unsigned long long) ((qe >= 128)? qe - 53 : 75) << 52));   // 2^(qe - 1076) = ulp(q1)/2
	later = !(inRange && (t < __dmul_rn (__dmul_rn (h, n), 1.0 - 0x1p-40)));
	return later? NAN : q1;
	}

// the figure of a cell with an empty sample
template <int WHAT>
__device__ __forceinline__ double mx_empty (void)
	{ return ((WHAT == GDSP_MATRIX_COUNT) || (WHAT == GDSP_MATRIX_SUM))? 0.0 : NAN; }

__device__ __forceinline__ void mx_later (uint32_t* __restrict__ todo, uint32_t* __restrict__ ntodo, uint32_t cell)
	{ todo[atomicAdd (ntodo, 1u)] = cell; }                                // (a cell is finished once: at most the launch's cells)

// the same for the cells of a whole wave, which calls it with all its lanes: one atomic for all that are `later`
__device__ __forceinline__ void mx_later_wave (uint32_t* __restrict__ todo, uint32_t* __restrict__ ntodo, bool later, uint32_t cell)
	{
	const unsigned long long mask = __ballot (later);
	if (mask == 0) return;
	const uint32_t lane   = threadIdx.x & 63;
	const uint32_t leader = (uint32_t) __ffsll ((long long) mask) - 1;
	uint32_t base = 0;
	if (lane == leader) base = atomicAdd (ntodo, (uint32_t) __popcll (mask));
	base = __shfl (base, (int) leader, 64);
	if (later) todo[base + (uint32_t) __popcll (mask & ((1ull << lane) - 1))] = cell;
	}
