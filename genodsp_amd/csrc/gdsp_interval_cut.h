// gdsp_interval_cut.h -- what the operators that reduce arbitrary intervals of a file piece by piece share
// (gdsp_intervalstats.hip: statsover; gdsp_intervalbreadth.hip: breadthover; gdsp_intervalcorr.hip: correlateover): the refusals of a call (ic_check, which
// percentilesover takes too), the walk over a call's vectors a launch table at a time and over its intervals a launch at
// a time, the cut of a launch's intervals into PIECES -- an interval intersected with a tile of IC_TILE values of the
// 16-byte aligned frame its vector lies in --, their counting sort by tile (the caller's order kept inside a tile), the
// ITEMS of at most IC_ITEM_PIECES pieces of one tile a workgroup takes, their upload, on the device the decoding of an item
// and the staging of the part of the tile its pieces cover, and (ic_run) everything a call and a launch do around the
// kernel: buffers, report, events, copies, the wait, the timers.  What a wave does with a staged piece, the record it
// writes, the start of its kernel and how the host combines an interval's records stay in the operators' files.
#pragma once

#include <string.h>
#include <algorithm>
#include <vector>
#include "gdsp_common.h"
#include "gdsp_pieces.h"

#define IC_THREADS      256
#define IC_WAVES        (IC_THREADS / 64)
#define IC_TILE         4096                          // values: 32 KiB of LDS, five workgroups on a CU
#define IC_ITEM_PIECES  64                            // pieces of one tile a workgroup takes
#define IC_LAUNCH_PIECES (1u << 22)                   // pieces of one launch by default; one interval has at most 2^20 + 1

static_assert (IC_TILE <= 65536 && IC_ITEM_PIECES <= 65535 && GDSP_BATCH_MAX <= 65535, "16-bit fields below");

// one launch's table (the batch convention of gdsp_common.h): vector s is base[s][lead[s] .. lead[s]+n), base 16-byte aligned
struct IcBatch
	{
	const double* base[GDSP_BATCH_MAX];
	uint32_t      lead[GDSP_BATCH_MAX];
	};

// a workgroup's work: pieces [first, first+count) of the launch, all in tile `tile` of vector `vec`; together they cover
// values [h0, h1) of the tile.  A piece is lo | (hi-1) << 16, values [lo, hi) of the tile.
struct IcItem { uint32_t first, tile;  uint16_t count, vec, h0, h1m1; };
static_assert (sizeof(IcItem) == 16, "loaded as one 16-byte word");

// ---------------------------------------------------------------------------------------------- device ----
// the workgroup's item: its pieces [first, first+count), the tile's first value and that value's position in the vector
// (tile 0 behind a lead: tile[0] is in no piece); the values [h0, h1) of the tile are in `tile` when it returns
__device__ __forceinline__ void ic_stage_item (const IcBatch& B, const uint4* __restrict__ items, double* tile,
                                               uint32_t& first, uint32_t& count, uint32_t& pos0)
	{
	const uint4    raw = items[blockIdx.x];
	first = __builtin_amdgcn_readfirstlane (raw.x);
	const uint32_t t   = __builtin_amdgcn_readfirstlane (raw.y);
	const uint32_t cv  = __builtin_amdgcn_readfirstlane (raw.z);
	const uint32_t hh  = __builtin_amdgcn_readfirstlane (raw.w);
	const uint32_t vec = cv >> 16;
	count = cv & 0xFFFF;
	const uint32_t h0    = hh & 0xFFFF, h1 = (hh >> 16) + 1;
	const double*  base  = B.base[vec] + (uint64_t) t * IC_TILE;
	pos0 = t * IC_TILE - B.lead[vec];

	// values [h0, h1) of the tile, whole 16-byte words first; the hull ends inside the vector, so an odd last value is
	// loaded on its own (its word's other half may lie beyond the vector)
	const uint32_t e0 = h0 & ~1u;
	const uint32_t np = (h1 - e0) >> 1;
	const double2* src = reinterpret_cast<const double2*> (base + e0);
	double2*       dst = reinterpret_cast<double2*> (tile + e0);
	for (uint32_t b0=0 ; b0<np ; b0+=GDSP_STAGE_DEPTH*IC_THREADS)
		{
		double2 r[GDSP_STAGE_DEPTH];
#pragma unroll
		for (int u=0 ; u<GDSP_STAGE_DEPTH ; u++)                // (every lane loads, index clamped: see gdsp_stage_f64)
			{ const uint32_t p = b0 + u*IC_THREADS + threadIdx.x;  r[u] = src[(p < np)? p : np-1]; }
#pragma unroll
		for (int u=0 ; u<GDSP_STAGE_DEPTH ; u++)
			{ const uint32_t p = b0 + u*IC_THREADS + threadIdx.x;  if (p < np) dst[p] = r[u]; }
		}
	if ((((h1 - e0) & 1) != 0) && (threadIdx.x == 0)) tile[h1-1] = base[h1-1];
	__syncthreads ();
	}

// ------------------------------------------------------------------------------------------------ host ----
struct IcVector { const double* v;  uint32_t n, lead, tile0; };      // tile0: its first tile in the launch's numbering

// a launch's pieces and items, as ic_cut left them
struct IcCut
	{
	std::vector<uint32_t> tileFirst;      // [tiles + 1]: the first piece of each tile of the launch
	std::vector<uint32_t> ivFirst;        // [nsel + 1]: interval j's pieces are ivPiece[ivFirst[j] .. ivFirst[j+1]), in position order
	std::vector<uint32_t> ivPiece;
	uint32_t P, nitems;
	};

// the refusals of a call, in the caller's name, before the device is touched
static inline int ic_check (const char* who, const gdsp_batch_item* items, int nitems, const uint32_t* h_vec, const uint32_t* h_start,
                            const uint32_t* h_end, uint32_t count)
	{
	const char* msg = NULL;
	if ((h_start == NULL) || (h_end == NULL)) msg = "NULL interval arrays";
	else if ((items == NULL) || (nitems <= 0)) msg = "no vectors";
	for (int k=0 ; (msg == NULL) && (k<nitems) ; k++)
		{ if ((items[k].n != 0) && ((items[k].d_in == NULL) || ((((uintptr_t) items[k].d_in) & 7) != 0))) msg = "a vector must be 8-byte aligned"; }
	for (uint32_t i=0 ; (msg == NULL) && (i<count) ; i++)
		{
		const uint32_t v = (h_vec != NULL)? h_vec[i] : 0;
		if      (v >= (uint32_t) nitems)   msg = "an interval names a vector beyond the table";
		else if (h_start[i] >= h_end[i])   msg = "an interval must have start < end";
		else if (h_end[i] > items[v].n)    msg = "an interval ends beyond its vector";
		}
	if (msg == NULL) return GDSP_OK;
	gdsp_set_error ("%s: %s", who, msg);
	return GDSP_EINVAL;
	}

// the intervals sel[0 .. nsel) (indices into the caller's arrays; all on the vectors vecs[0 .. nvec) of this launch,
// vector `vecBase + k` of the caller being vecs[k]) cut into pieces, sorted by tile and grouped into items, in the host
// halves of `pieces` and `items`
static inline int ic_cut (const char* who, GdspStaged<uint32_t>& pieces, GdspStaged<IcItem>& items, const IcVector* vecs, int nvec,
                          int vecBase, uint32_t tiles, const uint32_t* sel, uint32_t nsel, const uint32_t* h_vec,
                          const uint32_t* h_start, const uint32_t* h_end, IcCut& cut)
	{
	// pieces per tile and per interval
	std::vector<uint32_t>& tileFirst = cut.tileFirst;
	std::vector<uint32_t>& ivFirst   = cut.ivFirst;
	tileFirst.assign ((size_t) tiles + 1, 0);
	ivFirst.assign ((size_t) nsel + 1, 0);
	auto span = [&] (uint32_t i, const IcVector*& V, uint64_t& fs, uint64_t& fe)
		{
		V  = &vecs[((h_vec != NULL)? (int) h_vec[i] : 0) - vecBase];
		fs = (uint64_t) h_start[i] + V->lead;  fe = (uint64_t) h_end[i] + V->lead;       // in the frame
		};
	for (uint32_t j=0 ; j<nsel ; j++)
		{
		const IcVector* V;  uint64_t fs, fe;
		span (sel[j], V, fs, fe);
		const uint32_t ts = (uint32_t) (fs / IC_TILE), te = (uint32_t) ((fe - 1) / IC_TILE);
		for (uint32_t t=ts ; t<=te ; t++) tileFirst[V->tile0 + t + 1]++;
		ivFirst[j+1] = ivFirst[j] + (te - ts + 1);
		}
	const uint32_t P = ivFirst[nsel];
	uint32_t nitems = 0;
	std::vector<uint32_t> itemBase (tiles, 0);
	for (uint32_t g=0 ; g<tiles ; g++)
		{
		itemBase[g] = nitems;
		nitems += (tileFirst[g+1] + IC_ITEM_PIECES - 1) / IC_ITEM_PIECES;
		tileFirst[g+1] += tileFirst[g];
		}
	cut.P = P;  cut.nitems = nitems;
	int rc = pieces.grow (P, who);
	if (rc == GDSP_OK) rc = items.grow (nitems, who);
	if (rc != GDSP_OK) return rc;

	// the items of every tile that has pieces, their hulls still empty
		{
		int v = 0;
		for (uint32_t g=0 ; g<tiles ; g++)
			{
			const uint32_t c = tileFirst[g+1] - tileFirst[g];
			if (c == 0) continue;
			while ((v+1 < nvec) && (vecs[v+1].tile0 <= g)) v++;
			for (uint32_t k=0 ; k<c ; k+=IC_ITEM_PIECES)
				{
				IcItem& it = items.h[itemBase[g] + k / IC_ITEM_PIECES];
				it.first = tileFirst[g] + k;  it.tile = g - vecs[v].tile0;
				it.count = (uint16_t) std::min<uint32_t> (c - k, IC_ITEM_PIECES);  it.vec = (uint16_t) v;
				it.h0 = 0xFFFF;  it.h1m1 = 0;
				}
			}
		}
	// the pieces, sorted by tile (the caller's order inside a tile); where each interval's pieces went
	std::vector<uint32_t> cursor (tileFirst.begin (), tileFirst.end () - 1);
	cut.ivPiece.resize (P);
	for (uint32_t j=0 ; j<nsel ; j++)
		{
		const IcVector* V;  uint64_t fs, fe;
		span (sel[j], V, fs, fe);
		const uint32_t ts = (uint32_t) (fs / IC_TILE), te = (uint32_t) ((fe - 1) / IC_TILE);
		for (uint32_t t=ts ; t<=te ; t++)
			{
			const uint32_t g = V->tile0 + t;
			const uint64_t t0 = (uint64_t) t * IC_TILE;
			const uint32_t a = (uint32_t) (std::max (fs, t0) - t0), b = (uint32_t) (std::min (fe, t0 + IC_TILE) - t0);
			const uint32_t pos = cursor[g]++;
			pieces.h[pos] = a | ((b - 1) << 16);
			cut.ivPiece[ivFirst[j] + (t - ts)] = pos;
			IcItem& it = items.h[itemBase[g] + (pos - tileFirst[g]) / IC_ITEM_PIECES];
			it.h0   = (uint16_t) std::min<uint32_t> (it.h0, a);
			it.h1m1 = (uint16_t) std::max<uint32_t> (it.h1m1, b - 1);
			}
		}
	return GDSP_OK;
	}

// the launch's table of vectors, and its pieces and items on their way to the device
static inline int ic_upload (IcBatch& B, const IcVector* vecs, int nvec, GdspStaged<uint32_t>& pieces, GdspStaged<IcItem>& items,
                             const IcCut& cut, hipStream_t s)
	{
	for (int k=0 ; k<GDSP_BATCH_MAX ; k++)
		{
		B.base[k] = (k < nvec)? vecs[k].v - vecs[k].lead : NULL;
		B.lead[k] = (k < nvec)? vecs[k].lead : 0;
		}
	GDSP_HIP_TRY (hipMemcpyAsync (pieces.d, pieces.h, (size_t) cut.P * sizeof(uint32_t), hipMemcpyHostToDevice, s));
	GDSP_HIP_TRY (hipMemcpyAsync (items.d, items.h, (size_t) cut.nitems * sizeof(IcItem), hipMemcpyHostToDevice, s));
	return GDSP_OK;
	}

// a call's vectors a launch table at a time, and the intervals on a table's vectors in the caller's order, cut where a
// launch would hold more than maxPieces pieces (one interval always fits a launch):
// launch (vecs, nvec, vecBase, tiles, sel, nsel) -> GDSP_OK or what ends the call
template <typename Launch>
static inline int ic_for_each_launch (const gdsp_batch_item* items, int nitems, const uint32_t* h_vec, const uint32_t* h_start,
                                      const uint32_t* h_end, uint32_t count, uint64_t maxPieces, Launch launch)
	{
	int rc = GDSP_OK;
	std::vector<uint32_t> sel;
	for (int v0=0 ; (v0<nitems) && (rc == GDSP_OK) ; v0+=GDSP_BATCH_MAX)         // a table of vectors at a time
		{
		const int nvec = std::min (GDSP_BATCH_MAX, nitems - v0);
		IcVector vecs[GDSP_BATCH_MAX];
		uint32_t tiles = 0;
		for (int k=0 ; k<nvec ; k++)
			{
			vecs[k].v = items[v0+k].d_in;  vecs[k].n = items[v0+k].n;
			vecs[k].lead  = (items[v0+k].n != 0)? gdsp_frame_lead (items[v0+k].d_in) : 0;
			vecs[k].tile0 = tiles;
			tiles += (uint32_t) gdsp_frame_tiles (vecs[k].n, vecs[k].lead, IC_TILE);
			}
		// the caller's order, cut where a launch is full
		uint64_t pieces = 0;
		sel.clear ();
		for (uint32_t i=0 ; (i<=count) && (rc == GDSP_OK) ; i++)
			{
			uint64_t mine = 0;
			if (i < count)
				{
				const int v = (h_vec != NULL)? (int) h_vec[i] : 0;
				if ((v < v0) || (v >= v0 + nvec)) continue;
				const uint64_t fs = (uint64_t) h_start[i] + vecs[v-v0].lead, fe = (uint64_t) h_end[i] + vecs[v-v0].lead;
				mine = (fe - 1) / IC_TILE - fs / IC_TILE + 1;
				}
			if (!sel.empty () && ((i == count) || (pieces + mine > maxPieces)))
				{
				rc = launch (vecs, nvec, v0, tiles, sel.data (), (uint32_t) sel.size ());
				sel.clear ();  pieces = 0;
				}
			if (i < count) { sel.push_back (i);  pieces += mine; }
			}
		}
	return rc;
	}

// ---------------------------------------------------------------------------------------------- launch ----
// per device: staging and result buffers, grown on demand and kept; an operator derives from it what it adds
template <typename Record>
struct IcBuffers
	{
	GdspStaged<uint32_t> pieces;
	GdspStaged<IcItem>   items;
	GdspStaged<Record>   out;
	};

// what an operator's last call did: intervals, pieces and two counters of its own; ms spent cutting, in the kernel (HIP
// events), copying and waiting, combining; and the most pieces of a launch (set by tests; 0: IC_LAUNCH_PIECES)
struct IcReport { uint64_t last[4];  double ms[4];  uint32_t launchPieces; };

// a launch as the operator's hooks see it: its vectors (vecs[k] is the caller's vector vecBase + k) and their table, its
// intervals sel[0 .. nsel), its cut
struct IcLaunch
	{
	const IcVector* vecs;  int nvec, vecBase;  const uint32_t* sel;  uint32_t nsel;
	IcBatch B;  IcCut cut;  int dev;  hipStream_t s;
	};

// a call, in the name of the entry point `entry` (buffers and events in the operator's name `who`): the refusals, then
// launch by launch the cut, `recs` records of W.out per piece, the upload, the kernel between two events, the records'
// way back and the wait.  The operator's hooks, each (W, launch) with W its buffers of this device:
//   start   -> starts the kernel on launch.s (grid launch.cut.nitems);
//   device  -> device work behind the records that counts as copy time, if any; GDSP_OK or what ends the call;
//   combine -> the caller's results of the launch's intervals from the records in W.out.h (the combine timer); likewise
template <typename Buffers, typename Start, typename Device, typename Combine>
static inline int ic_run (const char* entry, const char* who, IcReport& rep, Buffers* perDevice, const gdsp_batch_item* items, int nitems,
                          const uint32_t* h_vec, const uint32_t* h_start, const uint32_t* h_end, uint32_t count, size_t recs,
                          void* stream, Start start, Device device, Combine combine)
	{
	memset (rep.last, 0, sizeof(rep.last));
	for (int k=0 ; k<4 ; k++) rep.ms[k] = 0;
	if (count == 0) return GDSP_OK;
	int rc = ic_check (entry, items, nitems, h_vec, h_start, h_end, count);
	if (rc != GDSP_OK) return rc;
	IcLaunch L;
	L.s = gdsp_stream (stream);
	rc = gdsp_device_slot (&L.dev, entry);
	if (rc != GDSP_OK) return rc;
	GdspEventPair ev;
	rc = ev.create (who);
	if (rc != GDSP_OK) return rc;
	Buffers& W = perDevice[L.dev];
	return ic_for_each_launch (items, nitems, h_vec, h_start, h_end, count, (rep.launchPieces != 0)? rep.launchPieces : IC_LAUNCH_PIECES,
		[&] (const IcVector* vecs, int nvec, int v0, uint32_t tiles, const uint32_t* sel, uint32_t nsel)
			{
			const GdspTimer tCut;
			L.vecs = vecs;  L.nvec = nvec;  L.vecBase = v0;  L.sel = sel;  L.nsel = nsel;
			rc = ic_cut (who, W.pieces, W.items, vecs, nvec, v0, tiles, sel, nsel, h_vec, h_start, h_end, L.cut);
			if (rc == GDSP_OK) rc = W.out.grow ((size_t) L.cut.P * recs, who);
			if (rc != GDSP_OK) return rc;
			rep.ms[0] += tCut.ms ();
			const GdspTimer tDev;
			rc = ic_upload (L.B, vecs, nvec, W.pieces, W.items, L.cut, L.s);
			if (rc != GDSP_OK) return rc;
			GDSP_HIP_TRY (hipEventRecord (ev.ev0, L.s));
			start (W, L);
			GDSP_LAUNCH_CHECK ();
			GDSP_HIP_TRY (hipEventRecord (ev.ev1, L.s));
			GDSP_HIP_TRY (hipMemcpyAsync (W.out.h, W.out.d, (size_t) L.cut.P * recs * sizeof(*W.out.h), hipMemcpyDeviceToHost, L.s));
			GDSP_HIP_TRY (hipStreamSynchronize (L.s));
			float kernelMs = 0;
			GDSP_HIP_TRY (hipEventElapsedTime (&kernelMs, ev.ev0, ev.ev1));
			rc = device (W, L);
			if (rc != GDSP_OK) return rc;
			rep.ms[1] += kernelMs;
			rep.ms[2] += tDev.ms () - kernelMs;
			const GdspTimer tCombine;
			rc = combine (W, L);
			if (rc != GDSP_OK) return rc;
			rep.ms[3] += tCombine.ms ();
			rep.last[0] += nsel;  rep.last[1] += L.cut.P;
			return GDSP_OK;
			});
	}
