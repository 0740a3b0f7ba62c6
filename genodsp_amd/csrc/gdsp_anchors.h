// gdsp_anchors.h -- the anchor half the anchor operators share (gdsp_profileover.hip: profileover; gdsp_matrixover.hip:
// matrixover; gdsp_regionsover.hip: regionsover): how an anchor is encoded for the device, the table of read-only vectors a
// launch takes and the walk that fills it, the checks of the arguments they take, the check on the device that every
// anchor lies inside its vector, the gather of a device's sources into items and anchors, the walk over the devices of an
// end-to-end call, and the holder of what a call allocates.  The kernels and the figures stay in their files;
// gdsp_anchors.hip has the checks on the device, compiled once.  A region has a start and an end where an anchor has a
// position: its check on the device is the anchors' host sequence around another kernel, and its gather stays with
// regionsover.  What matrixover and regionsover share beyond this -- the rows of a device -- is gdsp_matrix_rows.h's.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>
#include "gdsp_common.h"

// ---- the encoding: an anchor on the device is its position and a code word, the index of its vector among the call's
// items times two, plus one on the minus strand ----
__host__ __device__ __forceinline__ uint32_t gdsp_anchor_code (uint32_t vec, bool minus) { return vec * 2 + (minus? 1u : 0u); }
__host__ __device__ __forceinline__ uint32_t gdsp_anchor_vec (uint32_t code) { return code >> 1; }
__host__ __device__ __forceinline__ bool gdsp_anchor_minus (uint32_t code) { return (code & 1) != 0; }

// ---- the launch table: an anchor's vector is entry gdsp_anchor_vec (code) - vec0 of it; nvec or more: of another table ----
struct GdspAnchorTable
	{
	const double* v[GDSP_BATCH_MAX];
	uint32_t      n[GDSP_BATCH_MAX];
	uint32_t      vec0;                                   // the table holds the vectors vec0 .. vec0 + nvec - 1 of the call
	uint32_t      nvec;
	};

// host: launch (T) -> GDSP_OK or an error, over tables of GDSP_BATCH_MAX vectors each until every item has been in one
template <typename Launch>
static inline int gdsp_anchor_tables (const gdsp_batch_item* items, int nitems, Launch launch)
	{
	int rc = GDSP_OK;
	for (int i0=0 ; (i0<nitems) && (rc == GDSP_OK) ; i0+=GDSP_BATCH_MAX)
		{
		GdspAnchorTable T;
		T.vec0 = (uint32_t) i0;
		T.nvec = (uint32_t) std::min (nitems - i0, GDSP_BATCH_MAX);
		for (int j=0 ; j<GDSP_BATCH_MAX ; j++)
			{
			const bool have = (uint32_t) j < T.nvec;
			T.v[j] = have? items[i0+j].d_in : NULL;
			T.n[j] = have? items[i0+j].n    : 0;
			}
		rc = launch (T);
		}
	return rc;
	}

// ---- the checks.  who: the entry point, as the message names it ----
static inline int gdsp_anchor_refuse (const char* who, const char* msg) { gdsp_set_error ("%s: %s", who, msg);  return GDSP_EINVAL; }
static inline int gdsp_anchor_check_offsets (int32_t offLo, uint32_t noffsets, const char* who = __builtin_FUNCTION ())
	{
	if ((noffsets < 1) || (noffsets > GDSP_PROFILE_MAX_OFFSETS)) return gdsp_anchor_refuse (who, "the number of offsets must be 1 .. 16384");
	if ((int64_t) offLo + noffsets - 1 > INT32_MAX) return gdsp_anchor_refuse (who, "the last offset is beyond int32");
	return GDSP_OK;
	}

static inline int gdsp_anchor_check_aligned (const gdsp_batch_item* items, int nitems, const char* who = __builtin_FUNCTION ())
	{
	for (int i=0 ; i<nitems ; i++)
		if ((items[i].n != 0) && ((items[i].d_in == NULL) || ((((uintptr_t) items[i].d_in) & 7) != 0))) return gdsp_anchor_refuse (who, "a vector must be 8-byte aligned");
	return GDSP_OK;
	}

// the sources of an end-to-end call, on the host: after also (i) -> GDSP_OK or an error, what else the caller asks of
// source i, its anchors are there and inside its vector, and their number is added to *total
template <typename Also>
static inline int gdsp_anchor_check_sources (const gdsp_profile_source* sources, int nsources, Also also, uint64_t* total,
                                             const char* who = __builtin_FUNCTION ())
	{
	for (int i=0 ; i<nsources ; i++)
		{
		const int rc = also (i);
		if (rc != GDSP_OK) return rc;
		if ((sources[i].nanchors != 0) && (sources[i].h_pos == NULL)) return gdsp_anchor_refuse (who, "NULL anchors");
		for (uint32_t k=0 ; k<sources[i].nanchors ; k++)
			if (!(sources[i].h_pos[k] < sources[i].n)) return gdsp_anchor_refuse (who, "an anchor lies outside its vector");
		*total += sources[i].nanchors;
		}
	return GDSP_OK;
	}

// the same of `count` anchors that are on the device already, decided there: each names one of the items and a position in it
int gdsp_anchor_check (const gdsp_batch_item* items, int nitems, const uint32_t* d_pos, const uint32_t* d_code, uint32_t count,
                       hipStream_t s, const char* who);
// and of `count` regions: each names one of the items and is start < end <= the item's length
int gdsp_region_check (const gdsp_batch_item* items, int nitems, const uint32_t* d_start, const uint32_t* d_end, const uint32_t* d_code,
                       uint32_t count, hipStream_t s, const char* who);

// ---- the gather: the sources mine[0 .. nmine) (indices into `sources`) as the items of one device's calls.  Item k is
// source mine[k]; pos / code get the sources' anchors, one source after the other in that order, source mine[k]'s being
// first[k] .. first[k+1] - 1 of them (first: nmine + 1 entries, or NULL) ----
static inline void gdsp_anchor_gather (const gdsp_profile_source* sources, const int* mine, int nmine, std::vector<gdsp_batch_item>& items,
                                       std::vector<uint32_t>& pos, std::vector<uint32_t>& code, uint64_t* first = NULL)
	{
	items.clear ();  pos.clear ();  code.clear ();
	if (first != NULL) first[0] = 0;
	for (int k=0 ; k<nmine ; k++)
		{
		const gdsp_profile_source& S = sources[mine[k]];
		items.push_back (gdsp_batch_item ());                    // (all zero)
		items.back ().d_in = S.d_v;  items.back ().n = S.n;
		for (uint32_t a=0 ; a<S.nanchors ; a++)
			{
			pos.push_back (S.h_pos[a]);
			code.push_back (gdsp_anchor_code ((uint32_t) k, (S.h_minus != NULL) && (S.h_minus[a] != 0)));
			}
		if (first != NULL) first[k+1] = first[k] + S.nanchors;
		}
	}

// ---- the devices of an end-to-end call, each once in ascending order: on_device (mine, nmine) -> GDSP_OK or an error, with
// that device current and mine[0 .. nmine) its sources (indices into `sources`, the caller's order).  The caller's device
// is current again afterwards.  who: the entry point, as the message names it ----
template <typename Source, typename OnDevice>
static inline int gdsp_anchor_per_device (const Source* sources, int nsources, const char* who, OnDevice on_device)
	{
	int rc = GDSP_OK, home = 0;
	GDSP_HIP_TRY (hipGetDevice (&home));
	std::vector<int> devices;
	for (int i=0 ; i<nsources ; i++) devices.push_back (sources[i].device);
	std::sort (devices.begin (), devices.end ());
	devices.erase (std::unique (devices.begin (), devices.end ()), devices.end ());
	std::vector<int> mine;
	for (size_t d=0 ; (d<devices.size ()) && (rc == GDSP_OK) ; d++)
		{
		mine.clear ();
		for (int i=0 ; i<nsources ; i++) { if (sources[i].device == devices[d]) mine.push_back (i); }
		if (hipSetDevice (devices[d]) != hipSuccess)
			{ gdsp_set_error ("%s: device %d cannot be selected", who, devices[d]);  rc = GDSP_EHIP;  break; }
		rc = on_device (mine.data (), (int) mine.size ());
		}
	(void) hipSetDevice (home);
	return rc;
	}

// ---- what a call allocates on its devices: freed when the call returns, whichever way, each on the device it came from ----
struct GdspAnchorHeld
	{
	std::vector<std::pair<int, void*>> bufs;                 // (device, allocation)
	// *p = `bytes` on the current device; who, what: the entry point and the buffer as the complaint names them
	int alloc (void** p, size_t bytes, const char* who, const char* what)
		{
		int device = 0;
		*p = NULL;
		GDSP_HIP_TRY (hipGetDevice (&device));
		if (hipMalloc (p, bytes) != hipSuccess) { *p = NULL;  gdsp_set_error ("%s: no device memory for the %s", who, what);  return GDSP_ENOMEM; }
		bufs.push_back ({ device, *p });
		return GDSP_OK;
		}
	~GdspAnchorHeld ()
		{
		int home = 0;
		if (bufs.empty () || (hipGetDevice (&home) != hipSuccess)) return;
		for (auto& b : bufs) { (void) hipSetDevice (b.first);  (void) hipFree (b.second); }
		(void) hipSetDevice (home);
		}
	};
