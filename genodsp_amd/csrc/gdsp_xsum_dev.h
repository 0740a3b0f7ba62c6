// gdsp_xsum_dev.h -- the exact-sum device helpers shared by gdsp_xsum.hip (stats, normalize) and gdsp_intervalstats.hip
// (statsover): a finite double as digits of the integer image, and a lane's floating-point expansion grown with TwoSum.
#pragma once

#include <float.h>
#include <math.h>
#include <vector>
#include "gdsp_common.h"

#define XS_K          2                               // terms of a lane's expansion

// gdsp_xsum.hip, host: (-1)^neg * (L + something in (0,1) when sticky) * 2^scale rounded once to nearest, ties to even
// (L: 32-bit limbs, least significant first; subnormal results and +-inf beyond DBL_MAX included)
double xs_round_limbs (const std::vector<uint32_t>& L, bool sticky, int scale, bool neg);

// a finite double as three signed digits at word w: x = (c0 + c1 2^32 + c2 2^64) 2^(32w-1074), each |c| < 2^32
__host__ __device__ __forceinline__ void xs_split (double x, uint32_t& w, uint64_t& c0, uint64_t& c1, uint64_t& c2)
	{
	union { double d; uint64_t u; } b;
	b.d = x;
	const uint32_t be = (uint32_t) (b.u >> 52) & 0x7FF;
	uint64_t mant = b.u & 0xFFFFFFFFFFFFFull;
	uint32_t shift = 0;                                    // weight of mant's lowest bit: 2^(shift-1074)
	if (be != 0) { mant |= 1ull << 52;  shift = be - 1; }
	w = shift >> 5;
	const uint32_t r  = shift & 31;
	const uint64_t lo = mant << r;
	const uint64_t hi = (r == 0)? 0 : (mant >> (64 - r));
	c0 = lo & 0xFFFFFFFFull;  c1 = lo >> 32;  c2 = hi;
	if (b.u >> 63) { c0 = 0 - c0;  c1 = 0 - c1;  c2 = 0 - c2; }     // two's complement: the words add as signed integers
	}

__device__ __forceinline__ void xs_deposit (unsigned long long* acc, double x)
	{
	uint32_t w;  uint64_t c0, c1, c2;
	xs_split (x, w, c0, c1, c2);
	if (c0 != 0) atomicAdd (&acc[w],     (unsigned long long) c0);
	if (c1 != 0) atomicAdd (&acc[w + 1], (unsigned long long) c1);
	if (c2 != 0) atomicAdd (&acc[w + 2], (unsigned long long) c2);
	}

// an image (LDS or device) in canonical digits, 0 <= digit < 2^32 below the top one, by one lane (68 steps): canonical
// images add word by word with room to spare, and can be compared word for word
__device__ __forceinline__ void xs_carry (unsigned long long* acc)
	{
	long long carry = 0;
	for (int w=0 ; w<GDSP_XSUM_DIGITS-1 ; w++)
		{
		const long long x = (long long) acc[w] + carry;
		carry  = x >> 32;
		acc[w] = (unsigned long long) (x & 0xFFFFFFFFll);
		}
	acc[GDSP_XSUM_DIGITS-1] += (unsigned long long) carry;
	}

__host__ __device__ __forceinline__ bool xs_finite (double x) { return fabs (x) <= DBL_MAX; }

// a[] += x exactly, the careful way: TwoSum through the terms; what is left after the last one (or a summand whose TwoSum
// overflows, which then leaves the term it met unchanged) goes to the LDS image
__device__ __forceinline__ void xs_grow_careful (double (&a)[XS_K], double x, unsigned long long* acc)
	{
	double spill = 0.0;
#pragma unroll
	for (int k=0 ; k<XS_K ; k++)
		{
		const double s  = __dadd_rn (a[k], x);
		const double bp = __dsub_rn (s, a[k]);
		const double e  = __dadd_rn (__dsub_rn (a[k], __dsub_rn (s, bp)), __dsub_rn (x, bp));
		const bool   ok = xs_finite (s) && xs_finite (e);   // an overflow anywhere leaves +-inf or NaN in s or e
		a[k]  = ok? s : a[k];
		spill = ok? spill : x;
		x     = ok? e : 0.0;
		}
	if ((x != 0.0) || (spill != 0.0))
		{
		xs_deposit (acc, x);
		xs_deposit (acc, spill);
		atomicAdd (&acc[GDSP_XSUM_WORD_FLUSHES], 1ull);
		}
	}

// a[] += x exactly.  The fast path runs the TwoSums unchecked: an overflow in any of them leaves NaN in the final
// residual, so a residual that is not exactly zero -- a real one, or that NaN -- sends the lane back to the terms it
// had and through the careful form (rare on real data; a branch the other lanes skip)
__device__ __forceinline__ void xs_grow (double (&a)[XS_K], double x, unsigned long long* acc)
	{
	double keep[XS_K], r = x;
#pragma unroll
	for (int k=0 ; k<XS_K ; k++)
		{
		keep[k] = a[k];
		const double s  = __dadd_rn (a[k], r);
		const double bp = __dsub_rn (s, a[k]);
		r    = __dadd_rn (__dsub_rn (a[k], __dsub_rn (s, bp)), __dsub_rn (r, bp));
		a[k] = s;
		}
	if (r != 0.0)
		{
#pragma unroll
		for (int k=0 ; k<XS_K ; k++) a[k] = keep[k];
		xs_grow_careful (a, x, acc);
		}
	}

// a[] += x exactly, or not at all: the fast path of xs_grow with nowhere to put a residual.  A residual that is not
// exactly zero (a real one, or the NaN an overflowing TwoSum leaves) sets `flag` for good, and a[] means nothing from
// then on: the caller computes that sum again some other way.  No branch.
__device__ __forceinline__ void xs_grow_or_flag (double (&a)[XS_K], double x, uint32_t& flag)
	{
	double r = x;
#pragma unroll
	for (int k=0 ; k<XS_K ; k++)
		{
		const double s  = __dadd_rn (a[k], r);
		const double bp = __dsub_rn (s, a[k]);
		r    = __dadd_rn (__dsub_rn (a[k], __dsub_rn (s, bp)), __dsub_rn (r, bp));
		a[k] = s;
		}
	flag |= (r != 0.0)? 1u : 0u;
	}
