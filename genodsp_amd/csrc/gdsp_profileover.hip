// gdsp_profileover.hip -- profileover (not in the reference): the signal's figures at every offset from a list of anchors,
// exactly (include/genodsp_hip.h has the definitions).  gdsp_lagcorr.hip's construction with "lag" replaced by "offset
// from an anchor" and the walk driven by a list of positions: one integer image per offset, a lane's two-term expansion
// in registers over its whole walk, deposited once; the host rounds each image once.  Anchors times offsets values of
// 8 bytes are read, each once: bound by HBM (or by L2 where the windows of neighbouring anchors overlap).
//
// A workgroup is four waves and PF_BLOCK = 512 consecutive offsets (blockIdx.y picks the block): thread t owns the
// PF_LPL = 2 offsets t and t + 256 of the block, so that for one anchor the 64 lanes of a wave read 64 consecutive
// doubles -- ascending for a plus anchor (base p + k), descending for a minus one (base p - k) -- with plain 8-byte
// loads, which are right at any 8-byte alignment of the vector.  The workgroups of one block share the anchors of a
// launch by stride (blockIdx.x); an anchor (its position and gdsp_anchors.h's code word) is the same for every lane, so
// the walk is uniform, and it runs one anchor ahead of the sums.  An anchor whose block of offsets lies inside its chromosome reads
// without a test; any other anchor tests 0 <= g < n per lane.  Values that are not sampled (outside the chromosome, not finite, outside lo .. hi) are added as
// +0.0, which leaves no residual.  Pass 2 is the same walk over fl(fl(v - mean_k)^2), mean_k read once per lane; a q that
// is not finite is counted and not added.  Expansions, counts and INF counts stay in registers over the whole share and
// are deposited once at its end: grid x offsets atomics, not anchors x offsets.  No LDS, no barrier, no workgroup waits
// for another.
// What concerns the anchors rather than the sums -- their code word, the table of vectors a launch takes, the checks, the
// gather of a device's sources, the holder of its allocations -- is gdsp_anchors.h's, shared with matrixover.

#include <float.h>
#include <math.h>
#include <string.h>
#include <vector>
#include <algorithm>
#include "gdsp_common.h"
#include "gdsp_anchors.h"
#include "gdsp_xsum_dev.h"

#define PF_THREADS   256
#define PF_LPL       2                                // offsets of a lane: t and t + PF_THREADS
#define PF_BLOCK     (PF_THREADS * PF_LPL)            // offsets of a workgroup
#define PF_WG_TARGET (256 * 8)                        // workgroups of a launch: all resident (8 waves per SIMD), equal shares
#define PF_LAUNCH_ANCHORS (1u << 28)                  // anchors of a launch: an anchor gives an offset one value; were every
                                                      // one of them to flush (two deposits, each less than 2^32 into a
                                                      // word), a word of an offset's image still grows by less than
                                                      // 2^28 * 2 * 2^32 = 2^61 before the carry; the grid's own deposits
                                                      // (2 per workgroup) and a lane's u32 counts are far below that
#define PF_W         GDSP_XSUM_WORDS

template <bool SQ>
__global__ __launch_bounds__(PF_THREADS)
void profile_kernel (GdspAnchorTable P, const uint32_t* __restrict__ d_pos, const uint32_t* __restrict__ d_code, uint32_t aLo, uint32_t aHi,
                     int32_t offLo, uint32_t noffsets, double lo, double hi, const double* __restrict__ d_mean,
                     unsigned long long* __restrict__ d_acc)
	{
	const uint32_t k0   = blockIdx.y * PF_BLOCK;                              // the block's first offset, as an index
	const uint32_t kAct = (noffsets - k0 < PF_BLOCK)? noffsets - k0 : PF_BLOCK;   // its offsets
	const int64_t  dlo  = (int64_t) offLo + k0, dhi = dlo + kAct - 1;

	double   a[PF_LPL][XS_K], mean[PF_LPL];
	uint32_t cnt[PF_LPL], infs[PF_LPL];
	bool     live[PF_LPL];
	int64_t  d[PF_LPL];
	unsigned long long* img[PF_LPL];
#pragma unroll
	for (int j=0 ; j<PF_LPL ; j++)
		{
		const uint32_t k = threadIdx.x + j * PF_THREADS;
		live[j] = k < kAct;
		d[j]    = dlo + k;
		img[j]  = d_acc + (size_t) (k0 + (live[j]? k : 0)) * PF_W;          // (a lane that is not live never writes)
		a[j][0] = a[j][1] = 0.0;  cnt[j] = 0;  infs[j] = 0;
		mean[j] = 0.0;
		if (SQ && live[j]) mean[j] = d_mean[k0 + k];
		}

	// the walk, one anchor ahead: the next anchor and its vector are fetched while this one's values are added
	const double* __restrict__ nv = NULL;
	int64_t nn = 0, np = 0, ns = 1;
	auto fetch = [&] (uint64_t i)
		{
		const uint32_t code = d_code[i];
		const uint32_t vec  = gdsp_anchor_vec (code) - P.vec0;
		const bool     mine = vec < P.nvec;                               // (or a vector of another launch sequence)
		nv = P.v[mine? vec : 0];
		nn = mine? (int64_t) P.n[vec] : 0;
		np = d_pos[i];
		ns = gdsp_anchor_minus (code)? -1 : 1;
		};
	uint64_t i = (uint64_t) aLo + blockIdx.x;
	if (i < aHi) fetch (i);
	for ( ; i<aHi ; i+=gridDim.x)
		{
		const double* __restrict__ gv = nv;
		const int64_t n = nn, p = np, s = ns;
		if (i + gridDim.x < aHi) fetch (i + gridDim.x);
		const int64_t gLo = (s > 0)? p + dlo : p - dhi;                       // the bases the block's offsets look at
		const int64_t gHi = (s > 0)? p + dhi : p - dlo;
		if ((n == 0) || (gHi < 0) || (gLo >= n)) continue;

		double x[PF_LPL];
		bool   ok[PF_LPL];
		if ((gLo >= 0) && (gHi < n))
			{
#pragma unroll
			for (int j=0 ; j<PF_LPL ; j++)
				{
				ok[j] = live[j];
				x[j]  = live[j]? gv[p + s * d[j]] : 0.0;
				}
			}
		else
			{
#pragma unroll
			for (int j=0 ; j<PF_LPL ; j++)
				{
				const int64_t g = p + s * d[j];
				ok[j] = live[j] && (g >= 0) && (g < n);
				x[j]  = ok[j]? gv[g] : 0.0;
				}
			}
#pragma unroll
		for (int j=0 ; j<PF_LPL ; j++)
			{
			const bool take = ok[j] && xs_finite (x[j]) && !(x[j] < lo) && !(x[j] > hi);
			cnt[j] += take? 1u : 0u;
			double y = x[j];
			if (SQ)
				{
				const double dv = __dsub_rn (x[j], mean[j]);
				y = __dmul_rn (dv, dv);
				const bool inf = take && !xs_finite (y);
				infs[j] += inf? 1u : 0u;
				y = inf? 0.0 : y;
				}
			xs_grow (a[j], take? y : 0.0, img[j]);
			}
		}

#pragma unroll
	for (int j=0 ; j<PF_LPL ; j++)
		{
		if (!live[j]) continue;
#pragma unroll
		for (int k=0 ; k<XS_K ; k++) xs_deposit (img[j], a[j][k]);
		if (cnt[j] != 0)  atomicAdd (&img[j][GDSP_XSUM_WORD_COUNT], (unsigned long long) cnt[j]);
		if (infs[j] != 0) atomicAdd (&img[j][GDSP_XSUM_WORD_INF],   (unsigned long long) infs[j]);
		}
	}

// every image in canonical digits: the launches' images then add without overflow, and equal sums are equal words
__global__ void profile_carry_kernel (unsigned long long* __restrict__ d_acc, uint32_t noffsets)
	{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k < noffsets) xs_carry (d_acc + (size_t) k * PF_W);
	}

static uint32_t pfLaunchAnchors = PF_LAUNCH_ANCHORS;

extern "C" {

uint32_t gdsp_profile_block (void) { return PF_BLOCK; }

int gdsp_profile_set_launch_anchors (uint32_t anchors)
	{
	GDSP_REQUIRE (anchors <= PF_LAUNCH_ANCHORS, "more anchors in a launch than an image word can hold");
	pfLaunchAnchors = (anchors == 0)? PF_LAUNCH_ANCHORS : anchors;
	return GDSP_OK;
	}

int gdsp_profile_accumulate_batch (const gdsp_batch_item* items, int nitems, const uint32_t* d_pos, const uint32_t* d_code,
                                   uint32_t count, int32_t offLo, uint32_t noffsets, double lo, double hi, const double* d_mean,
                                   uint64_t* d_acc, void* stream)
	{
	GDSP_REQUIRE (d_acc != NULL, "NULL accumulator");
	GDSP_REQUIRE (nitems >= 0, "a negative number of vectors");
	GDSP_REQUIRE ((nitems == 0) || (items != NULL), "NULL items");
	GDSP_REQUIRE ((count == 0) || ((d_pos != NULL) && (d_code != NULL)), "NULL anchors");
	GDSP_REQUIRE ((count == 0) || (nitems > 0), "anchors without a vector");
	int rc = gdsp_anchor_check_offsets (offLo, noffsets);
	if (rc == GDSP_OK) rc = gdsp_anchor_check_aligned (items, nitems);
	if (rc != GDSP_OK) return rc;
	hipStream_t s = gdsp_stream (stream);
	unsigned long long* acc = reinterpret_cast<unsigned long long*> (d_acc);
	if (count == 0) return GDSP_OK;                              // (zeroed images are canonical)

	rc = gdsp_anchor_check (items, nitems, d_pos, d_code, count, s, __func__);     // on the device, where the anchors are
	if (rc != GDSP_OK) return rc;

	const uint32_t blocks = (noffsets + PF_BLOCK - 1) / PF_BLOCK;
	return gdsp_anchor_tables (items, nitems, [&] (const GdspAnchorTable& B) -> int
		{
		for (uint64_t aLo=0 ; aLo<count ; aLo+=pfLaunchAnchors)
			{
			const uint32_t aHi = (uint32_t) std::min<uint64_t> (count, aLo + pfLaunchAnchors);
			uint32_t gx = std::max (1u, PF_WG_TARGET / blocks);
			if (gx > aHi - (uint32_t) aLo) gx = aHi - (uint32_t) aLo;
			if (d_mean == NULL)
				hipLaunchKernelGGL (profile_kernel<false>, dim3 (gx, blocks), dim3 (PF_THREADS), 0, s, B, d_pos, d_code, (uint32_t) aLo, aHi,
				                    offLo, noffsets, lo, hi, d_mean, acc);
			else
				hipLaunchKernelGGL (profile_kernel<true>, dim3 (gx, blocks), dim3 (PF_THREADS), 0, s, B, d_pos, d_code, (uint32_t) aLo, aHi,
				                    offLo, noffsets, lo, hi, d_mean, acc);
			GDSP_LAUNCH_CHECK ();
			hipLaunchKernelGGL (profile_carry_kernel, dim3 ((noffsets + 63) / 64), dim3 (64), 0, s, acc, noffsets);
			GDSP_LAUNCH_CHECK ();
			}
		return GDSP_OK;
		});
	}

} // extern "C"

// ------------------------------------------------------------------------------------------- end to end ----
static gdsp_comm* pfComm = NULL;                             // see gdsp_genome_profile_use_comm
static uint64_t   pfLast[4];                                 // see gdsp_genome_profile_last

namespace {

// one pass over every device's sources and anchors into img (noffsets images): pass 1, or with h_mean pass 2
int pf_genome_pass (const gdsp_profile_source* sources, int nsources, int32_t offLo, uint32_t noffsets, double lo, double hi,
                    const double* h_mean, gdsp_reduce_fn reduce, void* reduceCtx, uint64_t* img)
	{
	std::vector<gdsp_xsum_source> xs (std::max (nsources, 0));
	for (int i=0 ; i<nsources ; i++)
		{ xs[i].d_v = sources[i].d_v;  xs[i].n = sources[i].n;  xs[i].first = 0;  xs[i].device = sources[i].device;  xs[i].stream = sources[i].stream; }
	const size_t words = (size_t) noffsets * PF_W;
	GdspAnchorHeld held;                                         // freed once every device's stream has been waited for
	std::vector<gdsp_batch_item> items;
	std::vector<uint32_t> pos, code;
	std::vector<int> mine;
	auto onDevice = [&] (const gdsp_xsum_source* its, int nits, uint64_t* d_acc, void* stream) -> int
		{
		// (a device's sources are those of its number, in the caller's order: gdsp_reduce_sources hands them over so)
		mine.clear ();
		for (int i=0 ; (i<nsources) && (nits>0) ; i++) { if (sources[i].device == its[0].device) mine.push_back (i); }
		gdsp_anchor_gather (sources, mine.data (), (int) mine.size (), items, pos, code);
		GDSP_REQUIRE ((int) items.size () == nits, "the sources of a device are not what it was handed");
		GDSP_REQUIRE (pos.size () <= UINT32_MAX, "more than 2^32 - 1 anchors on a device");
		hipStream_t s = gdsp_stream (stream);
		GDSP_HIP_TRY (hipMemsetAsync (d_acc, 0, words * sizeof(uint64_t), s));
		const size_t na = pos.size ();
		uint32_t* d_anchors = NULL;
		double*   d_mean    = NULL;
		if (na > 0)
			{
			const int rc = held.alloc ((void**) &d_anchors, 2 * na * sizeof(uint32_t), "gdsp_genome_profile", "anchors");
			if (rc != GDSP_OK) return rc;
			GDSP_HIP_TRY (hipMemcpyAsync (d_anchors,      pos.data (),  na * sizeof(uint32_t), hipMemcpyHostToDevice, s));
			GDSP_HIP_TRY (hipMemcpyAsync (d_anchors + na, code.data (), na * sizeof(uint32_t), hipMemcpyHostToDevice, s));
			}
		if (h_mean != NULL)
			{
			const int rc = held.alloc ((void**) &d_mean, noffsets * sizeof(double), "gdsp_genome_profile", "means");
			if (rc != GDSP_OK) return rc;
			GDSP_HIP_TRY (hipMemcpyAsync (d_mean, h_mean, noffsets * sizeof(double), hipMemcpyHostToDevice, s));
			}
		GDSP_HIP_TRY (hipStreamSynchronize (s));                 // (pos and code are reused for the next device)
		return gdsp_profile_accumulate_batch (items.data (), nits, d_anchors, (d_anchors == NULL)? NULL : d_anchors + na, (uint32_t) na,
		                                      offLo, noffsets, lo, hi, d_mean, d_acc, stream);
		};
	return gdsp_reduce_sources ("gdsp_genome_profile", "accumulators", pfComm, xs.data (), nsources, words, onDevice,
	                            reduce, reduceCtx, img);
	}

// column j's image: the sum of its bin's offset images, canonical or not
void pf_bin_image (const uint64_t* img, uint32_t j, uint32_t bin, uint64_t* out)
	{
	memset (out, 0, PF_W * sizeof(uint64_t));
	for (uint32_t k=j*bin ; k<(j+1)*bin ; k++)
		for (int w=0 ; w<PF_W ; w++) out[w] += img[(size_t) k * PF_W + w];
	}

} // namespace

extern "C" {

int gdsp_genome_profile_use_comm (gdsp_comm* comm) { pfComm = comm;  return GDSP_OK; }

void gdsp_genome_profile_last (uint64_t out[4]) { memcpy (out, pfLast, sizeof(pfLast)); }

int gdsp_genome_profile (const gdsp_profile_source* sources, int nsources, int32_t offLo, uint32_t noffsets, uint32_t bin,
                         double lo, double hi, gdsp_reduce_fn reduce, void* reduceCtx, uint64_t* count, double* sum,
                         double* mean, double* variance, double* stddev)
	{
	GDSP_REQUIRE ((count != NULL) && (sum != NULL) && (mean != NULL) && (variance != NULL) && (stddev != NULL), "NULL result");
	GDSP_REQUIRE (nsources >= 0, "a negative number of sources");
	GDSP_REQUIRE ((nsources == 0) || (sources != NULL), "NULL sources");
	int rc = gdsp_anchor_check_offsets (offLo, noffsets);
	if (rc != GDSP_OK) return rc;
	GDSP_REQUIRE ((bin >= 1) && (noffsets % bin == 0), "the bin must divide the number of offsets");
	GDSP_REQUIRE (!((pfComm != NULL) && (reduce != NULL)), "a host reduction hook next to a communicator");
	memset (pfLast, 0, sizeof(pfLast));
	rc = gdsp_anchor_check_sources (sources, nsources, [] (int) { return GDSP_OK; }, &pfLast[0]);
	if (rc != GDSP_OK) return rc;

	const uint32_t ncols = noffsets / bin;
	std::vector<uint64_t> img ((size_t) noffsets * PF_W);
	rc = pf_genome_pass (sources, nsources, offLo, noffsets, lo, hi, NULL, reduce, reduceCtx, img.data ());
	if (rc != GDSP_OK) return rc;
	std::vector<double> offMean (noffsets, 0.0);
	uint64_t col[PF_W];
	bool some = false;
	for (uint32_t j=0 ; j<ncols ; j++)
		{
		pf_bin_image (img.data (), j, bin, col);
		count[j]   = col[GDSP_XSUM_WORD_COUNT];
		pfLast[1] += col[GDSP_XSUM_WORD_COUNT];
		pfLast[2] += col[GDSP_XSUM_WORD_FLUSHES];
		sum[j]     = gdsp_xsum_round (col);
		mean[j]    = variance[j] = stddev[j] = NAN;
		if (count[j] == 0) continue;
		some = true;
		mean[j] = gdsp_xsum_div_round (col, count[j]);
		for (uint32_t k=j*bin ; k<(j+1)*bin ; k++) offMean[k] = mean[j];
		}
	if (!some) return GDSP_OK;                                   // (no column has a mean to centre on)

	rc = pf_genome_pass (sources, nsources, offLo, noffsets, lo, hi, offMean.data (), reduce, reduceCtx, img.data ());
	if (rc != GDSP_OK) return rc;
	for (uint32_t j=0 ; j<ncols ; j++)
		{
		pf_bin_image (img.data (), j, bin, col);
		pfLast[2] += col[GDSP_XSUM_WORD_FLUSHES];
		pfLast[3] += col[GDSP_XSUM_WORD_INF];
		if (count[j] == 0) continue;
		variance[j] = gdsp_xsum_div_round (col, count[j]);
		stddev[j]   = sqrt (variance[j]);
		}
	return GDSP_OK;
	}

} // extern "C"
