// gdsp_pieces.h -- the host half the piece operators share (gdsp_intervalstats.hip: statsover; gdsp_segments.hip:
// segments; gdsp_paint.hip: keepsegments): staging buffers that grow on demand, the per-device slot, the pair of timing
// events, the second and exact sum of flagged pieces, and the host arithmetic that makes one record of many
// gdsp_interval_piece (include/genodsp_hip.h).  The kernels, and what each operator cuts into pieces, stay in their files.
#pragma once

#include <math.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <utility>
#include <vector>
#include "gdsp_common.h"

#define GDSP_FLAG_BATCH 1024                          // flagged pieces summed again per read-back

// a pinned host array and its device twin, grown on demand and kept: `floor` elements at first, then doubling
template <typename T>
struct GdspStaged
	{
	T *h, *d;  size_t cap;

	// room for `want` elements; the first `keep` host elements survive a regrow, nothing else does.  The device half is
	// gdsp_malloc's (poisoned under GDSP_POISON: the callers write every word before it is read).  cap is 0 after a failure
	int grow (size_t want, const char* who, size_t keep = 0, size_t floor = 65536)
		{
		if (want <= cap) return GDSP_OK;
		size_t n = (cap == 0)? floor : cap;
		while (n < want) n *= 2;
		const std::vector<T> kept (h, h + keep);
		if (h != NULL) { (void) hipHostFree (h);  h = NULL; }
		if (d != NULL) { (void) gdsp_free (d);  d = NULL; }
		cap = 0;
		if (hipHostMalloc ((void**) &h, n * sizeof(T), hipHostMallocDefault) != hipSuccess) { h = NULL;  gdsp_set_error ("%s: no pinned memory", who);  return GDSP_ENOMEM; }
		if (gdsp_malloc ((void**) &d, n * sizeof(T)) != GDSP_OK) { d = NULL;  return GDSP_ENOMEM; }
		if (keep != 0) memcpy (h, kept.data (), keep * sizeof(T));
		cap = n;
		return GDSP_OK;
		}
	};

// host milliseconds since t0; a GdspTimer counts from where it is declared
static inline double gdsp_ms_since (std::chrono::steady_clock::time_point t0)
	{ return std::chrono::duration<double, std::milli> (std::chrono::steady_clock::now () - t0).count (); }
struct GdspTimer { std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now ();  double ms () const { return gdsp_ms_since (t0); } };

// *dev = the current device, which the operators' per-device buffers (64 slots each) have a slot for
static inline int gdsp_device_slot (int* dev, const char* who = __builtin_FUNCTION ())
	{
	GDSP_HIP_TRY (hipGetDevice (dev));
	if ((*dev < 0) || (*dev >= 64)) { gdsp_set_error ("%s: device index beyond 63", who);  return GDSP_EINVAL; }
	return GDSP_OK;
	}

// the two events a call times its kernels with; they go when the call returns, whichever way
struct GdspEventPair
	{
	hipEvent_t ev0 = NULL, ev1 = NULL;
	int create (const char* who)
		{
		GDSP_HIP_TRY (hipEventCreate (&ev0));
		if (hipEventCreate (&ev1) != hipSuccess) { ev1 = NULL;  gdsp_set_error ("%s: no event", who);  return GDSP_EHIP; }
		return GDSP_OK;
		}
	~GdspEventPair ()
		{
		if (ev0 != NULL) (void) hipEventDestroy (ev0);
		if (ev1 != NULL) (void) hipEventDestroy (ev1);
		}
	};

// the flagged records among `count` (flagOf (p): record p is), each summed again as the one source of an exact pass
// (gdsp_xsum_accumulate_batch over stretchOf (p) = { its first value on the device, its length }, limits lo .. hi),
// GDSP_FLAG_BATCH images per read-back through `staging`.  -> flagged: their indices, ascending; images: one
// GDSP_XSUM_WORDS image each, in that order.  who: the entry point, as the complaint about memory names it
template <typename FlagOf, typename StretchOf>
static inline int gdsp_flagged_images (const char* who, uint32_t count, FlagOf flagOf, StretchOf stretchOf, double lo, double hi,
                                       GdspStaged<uint64_t>& staging, int dev, hipStream_t s, std::vector<uint32_t>& flagged,
                                       std::vector<uint64_t>& images)
	{
	const size_t words = (size_t) GDSP_FLAG_BATCH * GDSP_XSUM_WORDS;
	flagged.clear ();
	for (uint32_t p=0 ; p<count ; p++) { if (flagOf (p)) flagged.push_back (p); }
	images.assign (flagged.size () * GDSP_XSUM_WORDS, 0);
	if (flagged.empty ()) return GDSP_OK;
	int rc = staging.grow (words, who, 0, words);
	if (rc != GDSP_OK) return rc;
	for (size_t f0=0 ; f0<flagged.size () ; f0+=GDSP_FLAG_BATCH)
		{
		const size_t m = std::min<size_t> (GDSP_FLAG_BATCH, flagged.size () - f0);
		GDSP_HIP_TRY (hipMemsetAsync (staging.d, 0, m * GDSP_XSUM_WORDS * sizeof(uint64_t), s));
		for (size_t f=0 ; f<m ; f++)
			{
			const std::pair<const double*, uint32_t> stretch = stretchOf (flagged[f0 + f]);
			gdsp_xsum_source src;
			src.d_v = stretch.first;  src.n = stretch.second;  src.first = 0;
			src.device = dev;  src.stream = (void*) s;
			rc = gdsp_xsum_accumulate_batch (&src, 1, 1, lo, hi, staging.d + f * GDSP_XSUM_WORDS, (void*) s);
			if (rc != GDSP_OK) return rc;
			}
		GDSP_HIP_TRY (hipMemcpyAsync (staging.h, staging.d, m * GDSP_XSUM_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
		GDSP_HIP_TRY (hipStreamSynchronize (s));
		memcpy (&images[f0 * GDSP_XSUM_WORDS], staging.h, m * GDSP_XSUM_WORDS * sizeof(uint64_t));
		}
	return GDSP_OK;
	}

// ---- many pieces into one, on the host (no GPU) ----
// count, least and greatest value of all pieces, the lowest position of equal maxima, and whether any piece is flagged.
// (The loop runs on locals: with the struct's members as the running figures the compiler built a longer loop -- compare
// and blend beside the minsd -- and the host half of segments, one call per segment, ran 2-3 % slower.)
struct GdspPiecesMerge { uint64_t count;  double min, max;  uint32_t maxpos;  bool anyFlag; };
static inline GdspPiecesMerge gdsp_pieces_merge (const gdsp_interval_piece* pieces, size_t npieces)
	{
	uint64_t count = 0;
	double   mn = HUGE_VAL, mx = -HUGE_VAL;
	uint32_t pos = UINT32_MAX;
	bool     anyFlag = false;
	for (size_t k=0 ; k<npieces ; k++)
		{
		const gdsp_interval_piece& p = pieces[k];
		anyFlag |= (p.flag != 0);
		if (p.count == 0) continue;
		count += p.count;
		if (p.min < mn) mn = p.min;
		if ((p.max > mx) || ((p.max == mx) && (p.maxpos < pos))) { mx = p.max;  pos = p.maxpos; }
		}
	return { count, mn, mx, pos, anyFlag };
	}

// the terms of (unflagged) pieces into the two terms a[] with TwoSum -> true when that was exact: every residual was
// zero (an overflow leaves a NaN); a[] means nothing otherwise
static inline bool gdsp_pieces_two_terms (const gdsp_interval_piece* pieces, size_t npieces, double (&a)[2])
	{
	double left = 0.0;
	a[0] = a[1] = 0.0;
	for (size_t k=0 ; (k<npieces) && (left == 0.0) ; k++)
		{
		const double term[2] = { pieces[k].a0, pieces[k].a1 };
		for (int j=0 ; (j<2) && (left == 0.0) ; j++)
			{
			double r = term[j];
			for (int i=0 ; i<2 ; i++)
				{
				const double s  = a[i] + r;
				const double bp = s - a[i];
				r    = (a[i] - (s - bp)) + (r - bp);
				a[i] = s;
				}
			left = r;
			}
		}
	return left == 0.0;
	}

// img = the pieces' sum as a 72-word integer image: the terms of unflagged pieces, and the digits of the flagged pieces'
// images (one per flagged piece, in order).  The caller clears the words beyond the digits that it does not want
static inline void gdsp_pieces_image (const gdsp_interval_piece* pieces, size_t npieces, const uint64_t* images, uint64_t (&img)[GDSP_XSUM_WORDS])
	{
	memset (img, 0, sizeof(img));
	for (size_t k=0 ; k<npieces ; k++)
		{
		if (pieces[k].flag == 0) { gdsp_xsum_add_host (img, pieces[k].a0);  gdsp_xsum_add_host (img, pieces[k].a1);  continue; }
		for (int w=0 ; w<GDSP_XSUM_DIGITS ; w++) img[w] += images[w];
		images += GDSP_XSUM_WORDS;
		}
	}
