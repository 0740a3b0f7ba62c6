// gdsp_paint.hip -- keepsegments (not in the reference): the kept segments of `segments` written back into the signal
// (include/genodsp_hip.h).  Two layers:
//   gdsp_paint_spans_batch    a sorted list of disjoint spans, one value each, painted into the vectors' outputs: a store
//                             stream.  Every base between a cursor and a limit is written exactly once.
//   gdsp_keep_segments_batch  gdsp_segments_batch's pass over the inputs; each time kept segments arrive (a bounded number
//                             at a time) their spans are painted into the outputs from where the last paint ended to the
//                             end of the last segment received, and what is left is painted after the pass.  The outputs are
//                             other buffers than the inputs, so painting behind the pass cannot change what it reads, and
//                             neither host nor device memory grows with the number of segments.
//
// pn_paint_kernel: a 256-thread workgroup per tile of PN_TILE values of the 16-byte aligned frame the OUTPUT lies in, tiles
// in gdsp_xcd_tile order, 16-byte non-temporal stores with the lanes of a wave covering whole lines.  The host gives every
// tile the index of the first span that reaches into it and how many do (a walk of spans and tiles side by side, O(spans +
// tiles)); a tile never searches the list.  A tile without a span stores `outside` and reads nothing.  Otherwise the
// spans that cross it set their start and end bits in two LDS bit masks of the tile (disjoint spans: distinct bits), one
// scan gives every 32-bit word the popcounts before it, and a base is inside a span iff more spans have started at or
// before it than have ended, the span being `first + starts - 1`: its value comes from the span list (the lanes of a
// wave read neighbouring records the tile has just read), or, in copy mode, from the input's own base.  Figure modes read
// nothing of the signal: 8 B per base.
// No workgroup reads what another wrote and there is no atomic on global memory.
// The staging buffers, the per-device slot and the timing events are gdsp_pieces.h's, shared with statsover and segments.

#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <algorithm>
#include "gdsp_common.h"
#include "gdsp_pieces.h"

#define PN_THREADS      256
#define PN_PAIRS        8                             // 16-byte words a thread stores
#define PN_TILE         (PN_THREADS * PN_PAIRS * 2)   // 4096 values
#define PN_WORDS        (PN_TILE / 32)                // words of a bit mask of the tile
#define PN_CHUNK_SPANS  (1u << 21)                    // spans of one upload (32 MiB)

struct __align__(16) PnSpan { uint32_t start, end;  double value; };    // [start, end) of the vector the kernel sees
static_assert (sizeof(PnSpan) == 16, "one 16-byte load per span");
static_assert (PN_WORDS <= PN_THREADS / 2 && PN_WORDS == 128, "the word scan runs in the first two waves");
static_assert (PN_TILE <= 0xFFFF, "two 16-bit counts in a word");

// index[g] = { the first span that reaches into tile g of the grid, how many do }
template <bool COPY>
__global__ __launch_bounds__(PN_THREADS)
void pn_paint_kernel (GdspBatch B, const uint2* __restrict__ index, const PnSpan* __restrict__ spans, double outside)
	{
	__shared__ uint32_t sbits[PN_WORDS], ebits[PN_WORDS], pre[PN_WORDS], wtot;
	const double* in;  double* out;  uint32_t n;
	const uint32_t g     = gdsp_xcd_tile (blockIdx.x, B.tile0[GDSP_BATCH_MAX]);
	const uint32_t t     = gdsp_batch_tile (B, in, out, n);
	const uint32_t lead  = gdsp_aligned16 (out)? 0 : 1;
	const uint2    ix    = index[g];
	const uint32_t first = __builtin_amdgcn_readfirstlane (ix.x);
	const uint32_t count = __builtin_amdgcn_readfirstlane (ix.y);
	const uint64_t f0    = (uint64_t) t * PN_TILE, fend = (uint64_t) lead + n;     // the tile and the vector in the frame
	const bool     whole = (f0 >= lead) && (f0 + PN_TILE <= fend);
	const int64_t  p0    = (int64_t) f0 - lead;                                     // the vector position of the tile's first value
	const uint32_t tid   = threadIdx.x;
	double2 v[PN_PAIRS];

	if (count == 0)
		{
#pragma unroll
		for (int u=0 ; u<PN_PAIRS ; u++) v[u] = make_double2 (outside, outside);
		}
	else
		{
		double2 x[PN_PAIRS];
		if (COPY)                                              // (issued before the masks are built)
			{
			const uint32_t ilead = gdsp_aligned16 (in)? 0 : 1;
			if (whole && (ilead == lead))
				{
				const double2* src = reinterpret_cast<const double2*> (in - lead + f0);
#pragma unroll
				for (int u=0 ; u<PN_PAIRS ; u++) x[u] = gdsp_ld2 (&src[u*PN_THREADS + tid]);
				}
			else
				{
#pragma unroll
				for (int u=0 ; u<PN_PAIRS ; u++)
					{
					const int64_t p = p0 + 2 * (u*PN_THREADS + (int) tid);
					x[u].x = ((p   >= 0) && (p   < (int64_t) n))? in[p]   : outside;
					x[u].y = ((p+1 >= 0) && (p+1 < (int64_t) n))? in[p+1] : outside;
					}
				}
			}

		if (tid < PN_WORDS) { sbits[tid] = 0;  ebits[tid] = 0; }
		__syncthreads ();
		for (uint32_t k=tid ; k<count ; k+=PN_THREADS)         // (the host promises start < p0 + PN_TILE and end > p0)
			{
			const PnSpan  s = spans[first + k];
			const int64_t a = (int64_t) s.start - p0, e = (int64_t) s.end - p0;
			const uint32_t ua = (a < 0)? 0u : (uint32_t) a;
			atomicOr (&sbits[ua >> 5], 1u << (ua & 31));
			if (e < PN_TILE) atomicOr (&ebits[(uint32_t) e >> 5], 1u << ((uint32_t) e & 31));
			}
		__syncthreads ();
		// pre[w] = starts (low half) and ends (high half) in the words before w
		const uint32_t c = (tid < PN_WORDS)? ((uint32_t) __popc (sbits[tid]) | ((uint32_t) __popc (ebits[tid]) << 16)) : 0u;
		uint32_t incl = c;
		for (int off=1 ; off<64 ; off<<=1) { const uint32_t o = __shfl_up (incl, off, 64);  incl += ((tid & 63) >= (uint32_t) off)? o : 0u; }
		if (tid == 63) wtot = incl;
		__syncthreads ();
		if (tid < PN_WORDS) pre[tid] = incl - c + ((tid >= 64)? wtot : 0u);
		__syncthreads ();

#pragma unroll
		for (int u=0 ; u<PN_PAIRS ; u++)
			{
			const uint32_t i  = 2u * (u*PN_THREADS + tid), w = i >> 5, b = i & 31;      // (b is even: both values lie in word w)
			const uint32_t sw = sbits[w], ew = ebits[w], pr = pre[w];
			const uint32_t m0 = (2u << b) - 1u, m1 = (m0 << 1) | 1u;                    // the bits up to and including mine
			const uint32_t S0 = (pr & 0xFFFFu) + __popc (sw & m0), E0 = (pr >> 16) + __popc (ew & m0);
			const uint32_t S1 = (pr & 0xFFFFu) + __popc (sw & m1), E1 = (pr >> 16) + __popc (ew & m1);
			const bool in0 = (S0 > E0), in1 = (S1 > E1);
			if (COPY) { v[u].x = in0? x[u].x : outside;  v[u].y = in1? x[u].y : outside; }
			else
				{
				const double a0 = spans[first + (in0? S0 - 1 : 0u)].value;              // (count != 0: `first` is a record)
				const double a1 = spans[first + (in1? S1 - 1 : 0u)].value;
				v[u].x = in0? a0 : outside;  v[u].y = in1? a1 : outside;
				}
			}
		}

	double* base = out - lead;
	if (whole)
		{
		double2* dst = reinterpret_cast<double2*> (base + f0);
#pragma unroll
		for (int u=0 ; u<PN_PAIRS ; u++) gdsp_st2 (&dst[u*PN_THREADS + tid], v[u]);
		}
	else
		{
#pragma unroll
		for (int u=0 ; u<PN_PAIRS ; u++)
			{
			const uint64_t f = f0 + 2u * (u*PN_THREADS + tid);
			if ((f   >= lead) && (f   < fend)) base[f]   = v[u].x;
			if ((f+1 >= lead) && (f+1 < fend)) base[f+1] = v[u].y;
			}
		}
	}

// ---------------------------------------------------------------------------------------------- host ----
// per device: staging and device buffers, grown on demand and kept
struct PnBuffers { GdspStaged<PnSpan> spans;  GdspStaged<uint2> index; };
static PnBuffers pnBuffers[64];
static double    pnTimes[2];
static uint64_t  pnPainted[2];

struct PnPos { uint32_t vec, pos; };
static inline bool pn_before (const PnPos& a, const PnPos& b) { return (a.vec < b.vec) || ((a.vec == b.vec) && (a.pos < b.pos)); }

// a vector's share of one paint: [lo, hi) of items[vec], and its clipped spans in the staging array
struct PnPart { uint32_t vec, lo, hi;  size_t s0, s1; };

// every base from `from` up to `to` once, from the spans [spans, spans + nspans) (checked, in order; those outside the
// range are passed over)
static int pn_paint_range (PnBuffers& W, const gdsp_batch_item* items, int nitems, const gdsp_paint_span* spans, uint32_t nspans,
                           int copy, double outside, PnPos from, PnPos to, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1)
	{
	const GdspTimer tAll;
	int rc = W.spans.grow (std::max<size_t> (nspans, 1), "gdsp_paint_spans");
	if (rc != GDSP_OK) return rc;

	std::vector<PnPart> parts;
	size_t   ns = 0, tiles = 0;
	uint32_t k = 0;
	uint64_t inside = 0, total = 0;
	for (uint32_t v=from.vec ; (v<(uint32_t) nitems) && (v<=to.vec) ; v++)
		{
		const uint32_t lo = (v == from.vec)? from.pos : 0, hi = (v == to.vec)? to.pos : items[v].n;
		while ((k < nspans) && (spans[k].vec < v)) k++;
		if (hi <= lo) continue;
		PnPart p = { v, lo, hi, ns, ns };
		for ( ; (k<nspans) && (spans[k].vec == v) ; k++)
			{
			const uint32_t a = std::max (spans[k].start, lo), e = std::min (spans[k].end, hi);
			if (a >= e) { if (spans[k].start >= hi) break;  continue; }
			W.spans.h[ns].start = a - lo;  W.spans.h[ns].end = e - lo;  W.spans.h[ns].value = spans[k].value;
			ns++;  inside += e - a;
			}
		p.s1 = ns;
		tiles += (size_t) gdsp_frame_tiles (hi - lo, gdsp_frame_lead (items[v].d_out + lo), PN_TILE);
		total += hi - lo;
		parts.push_back (p);
		}
	if (parts.empty ()) return GDSP_OK;
	rc = W.index.grow (tiles, "gdsp_paint_spans");
	if (rc != GDSP_OK) return rc;

	// the tiles' spans: both ends only ever move forward
	size_t g = 0;
	for (const PnPart& p : parts)
		{
		const uint32_t lead = gdsp_frame_lead (items[p.vec].d_out + p.lo);
		const uint64_t nt   = gdsp_frame_tiles (p.hi - p.lo, lead, PN_TILE);
		size_t jf = p.s0, je = p.s0;
		for (uint64_t t=0 ; t<nt ; t++)
			{
			const int64_t ts = (int64_t) (t * PN_TILE) - lead, te = ts + PN_TILE;
			while ((jf < p.s1) && ((int64_t) W.spans.h[jf].end <= ts)) jf++;
			if (je < jf) je = jf;
			while ((je < p.s1) && ((int64_t) W.spans.h[je].start < te)) je++;
			W.index.h[g++] = make_uint2 ((uint32_t) jf, (uint32_t) (je - jf));
			}
		}

	if (ns != 0) GDSP_HIP_TRY (hipMemcpyAsync (W.spans.d, W.spans.h, ns * sizeof(PnSpan), hipMemcpyHostToDevice, s));
	GDSP_HIP_TRY (hipMemcpyAsync (W.index.d, W.index.h, tiles * sizeof(uint2), hipMemcpyHostToDevice, s));
	GDSP_HIP_TRY (hipEventRecord (ev0, s));
	size_t g0 = 0;
	for (size_t q0=0 ; q0<parts.size () ; )                              // a table of vectors at a time
		{
		GdspBatch B;
		int nvec = 0;
		B.tile0[0] = 0;
		for ( ; (q0<parts.size ()) && (nvec<GDSP_BATCH_MAX) ; q0++, nvec++)
			{
			const PnPart& p = parts[q0];
			const uint64_t tl = (uint64_t) B.tile0[nvec] + gdsp_frame_tiles (p.hi - p.lo, gdsp_frame_lead (items[p.vec].d_out + p.lo), PN_TILE);
			if ((tl > 0x7FFFFFFFull) && (nvec > 0)) break;                   // grid limit: the rest goes into the next launch
			B.in[nvec]  = copy? items[p.vec].d_in + p.lo : NULL;
			B.out[nvec] = items[p.vec].d_out + p.lo;  B.n[nvec] = p.hi - p.lo;
			B.tile0[nvec+1] = (uint32_t) tl;
			}
		for (int j=nvec ; j<GDSP_BATCH_MAX ; j++) { B.in[j] = NULL;  B.out[j] = NULL;  B.n[j] = 0;  B.tile0[j+1] = B.tile0[nvec]; }
		B.nvec = (uint32_t) nvec;
		const uint32_t grid = B.tile0[nvec];
		if (copy) hipLaunchKernelGGL ((pn_paint_kernel<true>),  dim3(grid), dim3(PN_THREADS), 0, s, B, W.index.d + g0, W.spans.d, outside);
		else      hipLaunchKernelGGL ((pn_paint_kernel<false>), dim3(grid), dim3(PN_THREADS), 0, s, B, W.index.d + g0, W.spans.d, outside);
		GDSP_LAUNCH_CHECK ();
		g0 += grid;
		}
	GDSP_HIP_TRY (hipEventRecord (ev1, s));
	GDSP_HIP_TRY (hipStreamSynchronize (s));                             // (the staging buffers are free again)
	float kernelMs = 0;
	GDSP_HIP_TRY (hipEventElapsedTime (&kernelMs, ev0, ev1));
	pnTimes[0] += kernelMs;
	pnTimes[1] += tAll.ms () - kernelMs;
	pnPainted[0] += inside;  pnPainted[1] += total - inside;
	return GDSP_OK;
	}

// ------------------------------------------------------------------------------------- keep_segments ----
struct KsState
	{
	const gdsp_batch_item* items;  int nitems;
	int      mode;  double one, zero;
	gdsp_segments_fn emit;  void* ctx;  void* stream;
	PnPos    cursor;
	std::vector<gdsp_paint_span> spans;
	int      rc;  std::string why;
	uint64_t painted[2];  double ms[2];
	};
static uint64_t ksLast[6];
static double   ksTimes[2];

static int ks_paint (KsState* k, uint32_t nspans, PnPos to)
	{
	k->rc = gdsp_paint_spans_batch (k->items, k->nitems, k->spans.data (), nspans, (k->mode == GDSP_KEEP_VALUE)? 1 : 0, k->zero,
	                                k->cursor.vec, k->cursor.pos, to.vec, to.pos, k->stream);
	if (k->rc != GDSP_OK) { k->why = gdsp_last_error ();  return 1; }
	k->cursor = to;
	for (int j=0 ; j<2 ; j++) { k->painted[j] += pnPainted[j];  k->ms[j] += pnTimes[j]; }
	return 0;
	}

static int ks_take (void* ctx, const gdsp_segment* segs, uint32_t count)
	{
	KsState* k = (KsState*) ctx;
	if (count == 0) return 0;
	k->spans.resize (count);
	for (uint32_t i=0 ; i<count ; i++)
		{
		const gdsp_segment& g = segs[i];
		gdsp_paint_span& p = k->spans[i];
		p.vec = g.vec;  p.start = g.start;  p.end = g.end;  p.reserved = 0;
		switch (k->mode)
			{
			case GDSP_KEEP_COUNT:  p.value = (double) g.stat.count;      break;
			case GDSP_KEEP_LENGTH: p.value = (double) (g.end - g.start); break;
			case GDSP_KEEP_SUM:    p.value = g.stat.sum;   break;
			case GDSP_KEEP_MEAN:   p.value = g.stat.mean;  break;
			case GDSP_KEEP_MIN:    p.value = g.stat.min;   break;
			case GDSP_KEEP_MAX:    p.value = g.stat.max;   break;
			default:               p.value = k->one;       break;    // (GDSP_KEEP_VALUE: not looked at)
			}
		}
	const PnPos to = { segs[count-1].vec, segs[count-1].end };
	if (ks_paint (k, count, to) != 0) return 1;
	return (k->emit != NULL)? k->emit (k->ctx, segs, count) : 0;
	}

extern "C" {

uint32_t gdsp_paint_tile (void) { return PN_TILE; }

int gdsp_paint_spans_batch (const gdsp_batch_item* items, int nitems, const gdsp_paint_span* spans, uint32_t nspans, int copy,
                            double outside, uint32_t fromVec, uint32_t fromPos, uint32_t toVec, uint32_t toPos, void* stream)
	{
	pnTimes[0] = pnTimes[1] = 0;  pnPainted[0] = pnPainted[1] = 0;
	GDSP_REQUIRE (nitems >= 0, "a negative number of vectors");
	GDSP_REQUIRE ((nitems == 0) || (items != NULL), "no vectors");
	GDSP_REQUIRE ((nspans == 0) || (spans != NULL), "NULL spans");
	PnPos from = { fromVec, fromPos }, to = { toVec, toPos };
	GDSP_REQUIRE (!pn_before (to, from), "the limit lies before the cursor");
	GDSP_REQUIRE ((toVec < (uint32_t) nitems) || ((toVec == (uint32_t) nitems) && (toPos == 0)), "the limit lies beyond the last vector");
	GDSP_REQUIRE ((fromVec >= (uint32_t) nitems) || (fromPos <= items[fromVec].n), "the cursor lies beyond its vector");
	GDSP_REQUIRE ((toVec >= (uint32_t) nitems) || (toPos <= items[toVec].n), "the limit lies beyond its vector");
	for (int k=0 ; k<nitems ; k++)
		{
		if (items[k].n == 0) continue;
		GDSP_REQUIRE ((items[k].d_out != NULL) && ((((uintptr_t) items[k].d_out) & 7) == 0), "an output must be 8-byte aligned");
		if (!copy) continue;
		GDSP_REQUIRE ((items[k].d_in != NULL) && ((((uintptr_t) items[k].d_in) & 7) == 0), "a vector must be 8-byte aligned");
		GDSP_REQUIRE ((items[k].d_in + items[k].n <= items[k].d_out) || (items[k].d_out + items[k].n <= items[k].d_in), "an output overlaps its input");
		}
	for (uint32_t k=0 ; k<nspans ; k++)
		{
		GDSP_REQUIRE (spans[k].vec < (uint32_t) nitems, "a span of a vector that is not there");
		GDSP_REQUIRE ((spans[k].start < spans[k].end) && (spans[k].end <= items[spans[k].vec].n), "a span must have start < end <= n");
		GDSP_REQUIRE ((k == 0) || (spans[k-1].vec < spans[k].vec) || ((spans[k-1].vec == spans[k].vec) && (spans[k-1].end <= spans[k].start)),
		              "the spans are not disjoint and in (vector, position) order");
		}
	if (!pn_before (from, to)) return GDSP_OK;
	int dev = 0, rc = gdsp_device_slot (&dev);
	if (rc != GDSP_OK) return rc;
	hipStream_t s = gdsp_stream (stream);
	GdspEventPair ev;
	rc = ev.create ("gdsp_paint_spans_batch");

	// PN_CHUNK_SPANS spans at a time, each time up to the end of the last of them
	uint32_t a = 0;
	while ((rc == GDSP_OK) && pn_before (from, to))
		{
		const uint32_t b = (uint32_t) std::min<uint64_t> ((uint64_t) a + PN_CHUNK_SPANS, nspans);
		PnPos upTo = to;
		if (b < nspans)
			{
			const PnPos last = { spans[b-1].vec, spans[b-1].end };
			if (pn_before (last, to)) upTo = last;
			}
		if (pn_before (from, upTo)) rc = pn_paint_range (pnBuffers[dev], items, nitems, spans + a, b - a, copy, outside, from, upTo, s, ev.ev0, ev.ev1);
		if (pn_before (from, upTo)) from = upTo;
		a = b;
		}
	return rc;
	}

void gdsp_paint_spans_last (uint64_t painted[2], double ms[2])
	{
	if (painted != NULL) memcpy (painted, pnPainted, sizeof(pnPainted));
	if (ms != NULL)      memcpy (ms, pnTimes, sizeof(pnTimes));
	}

int gdsp_keep_segments_batch (const gdsp_batch_item* items, int nitems, double T, int tiesAbove, uint32_t mergeGap, uint32_t minLength,
                              int haveMinHeight, double minHeight, int mode, double one, double zero, gdsp_segments_fn emit, void* ctx,
                              void* stream)
	{
	memset (ksLast, 0, sizeof(ksLast));  ksTimes[0] = ksTimes[1] = 0;
	GDSP_REQUIRE ((mode >= GDSP_KEEP_ONE) && (mode <= GDSP_KEEP_MAX), "no such mode");
	GDSP_REQUIRE (T == T, "the threshold is NaN");
	GDSP_REQUIRE (!haveMinHeight || (minHeight == minHeight), "the minimum height is NaN");
	if (nitems <= 0) return GDSP_OK;
	GDSP_REQUIRE (items != NULL, "no vectors");
	for (int k=0 ; k<nitems ; k++)
		{
		if (items[k].n == 0) continue;
		GDSP_REQUIRE ((items[k].d_in != NULL) && ((((uintptr_t) items[k].d_in) & 7) == 0), "a vector must be 8-byte aligned");
		GDSP_REQUIRE ((items[k].d_out != NULL) && ((((uintptr_t) items[k].d_out) & 7) == 0), "an output must be 8-byte aligned");
		GDSP_REQUIRE ((items[k].d_in + items[k].n <= items[k].d_out) || (items[k].d_out + items[k].n <= items[k].d_in),
		              "an output overlaps its input (the segments are painted while the signal is still being read)");
		}
	KsState k;
	k.items = items;  k.nitems = nitems;  k.mode = mode;  k.one = one;  k.zero = zero;  k.emit = emit;  k.ctx = ctx;  k.stream = stream;
	k.cursor.vec = 0;  k.cursor.pos = 0;  k.rc = GDSP_OK;
	k.painted[0] = k.painted[1] = 0;  k.ms[0] = k.ms[1] = 0;
	int rc = gdsp_segments_batch (items, nitems, T, tiesAbove, mergeGap, minLength, haveMinHeight, minHeight, ks_take, &k, stream);
	if ((rc != GDSP_OK) && (k.rc != GDSP_OK)) { gdsp_set_error ("%s", k.why.c_str ());  rc = k.rc; }      // (the paint's own complaint)
	if (rc == GDSP_OK)
		{
		const PnPos end = { (uint32_t) nitems, 0 };
		if (ks_paint (&k, 0, end) != 0) rc = k.rc;
		}
	gdsp_segments_last (ksLast);
	ksLast[4] = k.painted[0];  ksLast[5] = k.painted[1];
	ksTimes[0] = k.ms[0];  ksTimes[1] = k.ms[1];
	return rc;
	}

void gdsp_keep_segments_last  (uint64_t out[6]) { memcpy (out, ksLast, sizeof(ksLast)); }
void gdsp_keep_segments_times (double ms[2])    { memcpy (ms, ksTimes, sizeof(ksTimes)); }

} // extern "C"
