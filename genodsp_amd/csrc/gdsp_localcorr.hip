// gdsp_localcorr.hip -- localcorrelate: the correlation, covariance or regression of the signal against a second track
// over the window centred on every base.
//
// Not an operator of the reference.  Definition (include/genodsp_hip.h): localstats' window [lo, hi] = [max(0, c-lft),
// min(n-1, c+rgt)], rgt = (W-1)/2, lft = W-1-rgt, m = hi-lo+1; over it Sx, Sy and the sums Sxx, Syy, Sxy of one rounded
// product per term; Nxx = fl(fl(m Sxx) - fl(Sx Sx)), Nyy and Nxy alike, and the four figures from those.  Every step is
// one rounded operation (__dmul_rn and friends: never contracted); only the five window sums may be associated freely.
//
// x is the signal, only read.  y is the track on entry and the result on return: the driver holds two genome-sized
// buffers per chromosome and no third, so the result goes where the track was.  A tile's halo bases of y are the
// neighbouring tiles' own bases, which they overwrite; two launches in stream order keep every read ahead of every write:
//   1. copy    for every tile of every vector of the table, the HL track values before the tile and the HR behind it go to
//              a record of HL + HR doubles in workspace; positions outside the vector are written as 0.0, which is what
//              truncates the window at the chromosome ends.  Every slot of every record is written.
//   2. main    one workgroup of LC_THREADS threads owns T outputs and stages the NS = 16 LC_THREADS positions they read
//              (HL + T + HR, the reaches rounded up to even so that every tile starts on a 16-byte boundary): x whole
//              from d_x, the tile's own T track values from d_y, the track's halos from the tile's record.  From there
//              the tile is gdsp_window_sums_tile.h's, which localstats shares -- the two LDS images, the block sums of
//              all five sums and their scan, P(e), the slide, the results through LDS -- and its comments hold the
//              layout and its reasons; the results leave over the tile's own T bases of d_y.
// No workgroup reads a live base that another one writes; nothing is polled and nothing waits on another workgroup.
// One form: 512 threads, 8192 staged positions of each input, 156.6 KiB of LDS, one workgroup per CU.  8192 staged
// positions less a tile of 4096 outputs is what fixes GDSP_LOCALCORR_MAX_WINDOW at 4097.

#include <stdlib.h>
#include <algorithm>
#include "gdsp_window_sums_tile.h"
#include "gdsp_pieces.h"

#define LC_THREADS      512
#define LC_NS           (LC_THREADS * WS_G)                               // staged positions of each input
#define LC_MIN_TILE     4096
#define LC_COPY_THREADS 256
#define LC_NWHAT        4

struct LcTerms                                                            // x, y, fl(x x), fl(y y), fl(x y)
	{
	static constexpr int INPUTS = 2, SUMS = 5;
	static __device__ __forceinline__ void add (double p[SUMS], const double in[INPUTS])
		{
		const double x = in[0], y = in[1];
		p[0] = __dadd_rn (p[0], x);                  p[1] = __dadd_rn (p[1], y);
		p[2] = __dadd_rn (p[2], __dmul_rn (x, x));   p[3] = __dadd_rn (p[3], __dmul_rn (y, y));
		p[4] = __dadd_rn (p[4], __dmul_rn (x, y));
		}
	};
typedef WsLds<LC_THREADS, LcTerms::INPUTS, LcTerms::SUMS> LcLds;          // v[0]: the staged signal, v[1]: the staged track
static_assert (sizeof (LcLds) <= 160 * 1024, "one workgroup per CU");

__host__ __device__ constexpr uint32_t lc_tile (uint32_t lft, uint32_t rgt) { return ws_tile (LC_THREADS, lft, rgt); }
static_assert (lc_tile ((GDSP_LOCALCORR_MAX_WINDOW - 1) - (GDSP_LOCALCORR_MAX_WINDOW - 1) / 2, (GDSP_LOCALCORR_MAX_WINDOW - 1) / 2) == LC_MIN_TILE,
               "the largest window leaves a tile of 4096 outputs");
static_assert (LC_MIN_TILE / LC_THREADS >= 8, "ws_per never takes its 7 here");

// ---- launch 1: tile `gt` of the table -> its record: y[o0-HL .. o0) and y[o0+T .. o0+T+HR), 0.0 outside the vector
__global__ __launch_bounds__(LC_COPY_THREADS)
void localcorr_copy_kernel (GdspBatch B, WsArgs A, double* __restrict__ records)
	{
	const double* unused;  double* y;  uint32_t n;
	const uint32_t tile = gdsp_batch_tile (B, unused, y, n);
	const uint32_t gt   = gdsp_xcd_tile (blockIdx.x, B.tile0[GDSP_BATCH_MAX]);        // the tile's index in the table
	const int      HL   = (int) ws_even (A.lft), HR = (int) ws_even (A.rgt);
	const int      T    = LC_NS - HL - HR, len = HL + HR;
	const int64_t  o0   = (int64_t) tile * T;                             // (even: a pair never straddles the two halves or an end of the tile)
	double* rec = records + (size_t) gt * len;
	for (int q=threadIdx.x ; 2*q<len ; q+=LC_COPY_THREADS)
		{
		const int     p = 2*q;
		const int64_t g = (p < HL)? o0 - HL + p : o0 + T + (p - HL);
		double2 v;
		if ((g >= 0) && (g + 1 < (int64_t) n)) v = *reinterpret_cast<const double2*> (y + g);
		else
			{
			v.x = ((g >= 0) && (g < (int64_t) n))? y[g] : 0.0;
			v.y = ((g + 1 >= 0) && (g + 1 < (int64_t) n))? y[g+1] : 0.0;
			}
		*reinterpret_cast<double2*> (rec + p) = v;
		}
	}

// ---- launch 2
template <int WHAT>
__device__ __forceinline__ double lc_figure (const double S[LcTerms::SUMS], double md)
	{
	const double Sx = S[0], Sy = S[1];
	const double Nxy = __dsub_rn (__dmul_rn (md, S[4]), __dmul_rn (Sx, Sy));
	if (WHAT == GDSP_LOCALCORR_COVARIANCE) return (Nxy == 0.0)? 0.0 : __ddiv_rn (Nxy, __dmul_rn (md, md));
	const double Nxx = __dsub_rn (__dmul_rn (md, S[2]), __dmul_rn (Sx, Sx));
	if (WHAT == GDSP_LOCALCORR_CORRELATION)
		{
		const double Nyy = __dsub_rn (__dmul_rn (md, S[3]), __dmul_rn (Sy, Sy));
		if ((Nxx <= 0.0) || (Nyy <= 0.0)) return 0.0;
		const double D = __dmul_rn (__dsqrt_rn (Nxx), __dsqrt_rn (Nyy));
		if (D == 0.0) return 0.0;
		const double r = __ddiv_rn (Nxy, D);
		return (r > 1.0)? 1.0 : (r < -1.0)? -1.0 : r;
		}
	const double slope = (Nxx <= 0.0)? 0.0 : __ddiv_rn (Nxy, Nxx);
	if (WHAT == GDSP_LOCALCORR_SLOPE) return slope;
	return __dsub_rn (__ddiv_rn (Sy, md), __dmul_rn (slope, __ddiv_rn (Sx, md)));
	}

template <int WHAT>
__global__ __launch_bounds__(LC_THREADS)
void localcorr_kernel (GdspBatch B, WsArgs A, const double* __restrict__ records)      // one grid over every vector of the table (gdsp_common.h)
	{
	__shared__ __attribute__((aligned(16))) LcLds S;
	const double* x;  double* y;  uint32_t n;
	const uint32_t tile = gdsp_batch_tile (B, x, y, n);
	const uint32_t gt   = gdsp_xcd_tile (blockIdx.x, B.tile0[GDSP_BATCH_MAX]);
	const WsTile   t    = ws_tile_of<LC_THREADS> (A, tile);
	const int      tid  = threadIdx.x, HL = t.HL, T = t.T;
	const int64_t  o0   = t.o0;
	const double*  rec  = records + (size_t) gt * (LC_NS - T);            // HL values before the tile, then HR behind it

	// ---- stage: x whole, y from the tile's own bases and from its record
	ws_stage<LC_THREADS> (S.v[0], x, t.g0, n);
	if (o0 + T <= (int64_t) n)
		{
		double2 r[WS_G/2];
#pragma unroll
		for (int u=0 ; u<WS_G/2 ; u++)
			{
			const int e = 2 * (u*LC_THREADS + tid);                       // HL and T are even: a pair has one source
			const double* src = (e < HL)? rec + e : (e < HL + T)? y + o0 + (e - HL) : rec + (e - T);
			r[u] = *reinterpret_cast<const double2*> (src);
			}
#pragma unroll
		for (int u=0 ; u<WS_G/2 ; u++)
			{
			double* dst = S.v[1] + ws_at (2 * (u*LC_THREADS + tid));
			dst[0] = r[u].x;  dst[1] = r[u].y;
			}
		}
	else
		{
		for (int e=tid ; e<LC_NS ; e+=LC_THREADS)
			{
			double v;
			if (e < HL)          v = rec[e];
			else if (e < HL + T) v = (o0 + (e - HL) < (int64_t) n)? y[o0 + (e - HL)] : 0.0;
			else                 v = rec[e - T];
			S.v[1][ws_at (e)] = v;
			}
		}
	ws_block_sums<LC_THREADS, LcTerms> (S);
	ws_outputs<LC_THREADS, LcTerms> (S, A, t, n, y, [] (int, const double* sums, double md) { return lc_figure<WHAT> (sums, md); });
	}

// ---------------------------------------------------------------------------------------------- host ----
// per device: the records of one table of vectors; grown on demand and kept.  gdsp_malloc's (poisoned under
// GDSP_POISON): launch 1 writes every slot of every record before launch 2 reads any.  Calls on one device share it as
// gdsp_distance_batch's calls share theirs: each call's stream first waits for the event the call before it recorded
// behind its last launch, so calls on several streams of a device take the workspace in turn.
struct LcWork { void* d;  size_t cap;  hipEvent_t done; };
static LcWork lcWork[64];
static double lcTimes[2];

// GDSP_LOCALCORR_TIMES=1: the two launches are timed with events (profiles/localcorrelate.txt); the call then waits for them
static bool lc_timed (void)
	{
	static const bool value = [] () { const char* e = getenv ("GDSP_LOCALCORR_TIMES");  return (e != NULL) && (e[0] == '1'); } ();
	return value;
	}

static void lc_launch (const GdspBatch& B, uint32_t tiles, int what, const WsArgs& A, const double* records, hipStream_t s)
	{
	switch (what)
		{
		case GDSP_LOCALCORR_CORRELATION: hipLaunchKernelGGL ((localcorr_kernel<GDSP_LOCALCORR_CORRELATION>), dim3(tiles), dim3(LC_THREADS), 0, s, B, A, records);  break;
		case GDSP_LOCALCORR_COVARIANCE:  hipLaunchKernelGGL ((localcorr_kernel<GDSP_LOCALCORR_COVARIANCE>),  dim3(tiles), dim3(LC_THREADS), 0, s, B, A, records);  break;
		case GDSP_LOCALCORR_SLOPE:       hipLaunchKernelGGL ((localcorr_kernel<GDSP_LOCALCORR_SLOPE>),       dim3(tiles), dim3(LC_THREADS), 0, s, B, A, records);  break;
		default:                         hipLaunchKernelGGL ((localcorr_kernel<GDSP_LOCALCORR_INTERCEPT>),   dim3(tiles), dim3(LC_THREADS), 0, s, B, A, records);  break;
		}
	}

static int localcorr_run (const gdsp_batch_item* items, int nitems, uint32_t W, int what, void* stream)
	{
	WsArgs A = ws_window (W);
	const uint64_t T   = lc_tile (A.lft, A.rgt);
	const size_t   len = LC_NS - T;                                       // doubles per record (0 at W = 1: no halo, no launch 1)
	A.per = ws_per ((uint32_t) T, LC_THREADS);
	lcTimes[0] = lcTimes[1] = 0;
	auto tilesOf = [=] (uint32_t n) { return ((uint64_t) n + T - 1) / T; };

	// the largest table of the call decides the workspace (gdsp_batch_run: GDSP_BATCH_MAX vectors at a time)
	uint64_t most = 0;
		{
		uint64_t sum = 0;
		int      k = 0;
		for (int i=0 ; i<nitems ; i++)
			{
			if (items[i].n == 0) continue;
			if (k == GDSP_BATCH_MAX) { k = 0;  sum = 0; }
			sum += tilesOf (items[i].n);  k++;
			most = std::max (most, sum);
			}
		}
	if (most == 0) return GDSP_OK;
	hipStream_t s = gdsp_stream (stream);
	double* records = NULL;
	LcWork* work = NULL;
	if (len != 0)
		{
		int dev = 0;
		int rc = gdsp_device_slot (&dev);
		if (rc != GDSP_OK) return rc;
		work = &lcWork[dev];
		const size_t bytes = (size_t) most * len * sizeof(double);
		if (bytes > work->cap)
			{
			if (work->d != NULL) { (void) gdsp_free (work->d);  work->d = NULL;  work->cap = 0; }
			rc = gdsp_malloc (&work->d, bytes);
			if (rc != GDSP_OK) { work->d = NULL;  return rc; }
			work->cap = bytes;
			}
		records = (double*) work->d;
		if (work->done == NULL) GDSP_HIP_TRY (hipEventCreateWithFlags (&work->done, hipEventDisableTiming));
		else                    GDSP_HIP_TRY (hipStreamWaitEvent (s, work->done, 0));
		}

	const bool timed = lc_timed ();
	hipEvent_t ev[3] = { NULL, NULL, NULL };
	if (timed) { for (int k=0 ; k<3 ; k++) GDSP_HIP_TRY (hipEventCreate (&ev[k])); }
	hipError_t late = hipSuccess;
	gdsp_batch_run (items, nitems, tilesOf,
		[&] (const GdspBatch& B, uint32_t tiles)
			{
			if (timed) (void) hipEventRecord (ev[0], s);
			if (len != 0) hipLaunchKernelGGL (localcorr_copy_kernel, dim3(tiles), dim3(LC_COPY_THREADS), 0, s, B, A, records);
			if (timed) (void) hipEventRecord (ev[1], s);
			lc_launch (B, tiles, what, A, records, s);
			if (!timed) return;
			(void) hipEventRecord (ev[2], s);
			if (hipEventSynchronize (ev[2]) != hipSuccess) { late = hipErrorUnknown;  return; }
			for (int k=0 ; k<2 ; k++) { float ms = 0;  (void) hipEventElapsedTime (&ms, ev[k], ev[k+1]);  lcTimes[k] += ms; }
			});
	if (timed) { for (int k=0 ; k<3 ; k++) (void) hipEventDestroy (ev[k]); }
	GDSP_LAUNCH_CHECK ();
	GDSP_HIP_TRY (late);
	if (work != NULL) GDSP_HIP_TRY (hipEventRecord (work->done, s));
	return GDSP_OK;
	}

#define LC_CHECK_ARGS() \
	GDSP_REQUIRE (W >= 1, "window must be >= 1"); \
	GDSP_REQUIRE (W <= GDSP_LOCALCORR_MAX_WINDOW, "window above GDSP_LOCALCORR_MAX_WINDOW"); \
	GDSP_REQUIRE ((what >= 0) && (what < LC_NWHAT), "what must be one of GDSP_LOCALCORR_CORRELATION ... GDSP_LOCALCORR_INTERCEPT")

extern "C" {

uint32_t gdsp_localcorr_tile (uint32_t W)
	{
	if ((W < 1) || (W > GDSP_LOCALCORR_MAX_WINDOW)) return 0;
	const uint32_t rgt = (W - 1) / 2;
	return lc_tile ((W - 1) - rgt, rgt);
	}

int gdsp_localcorr (const double* d_x, double* d_y, uint32_t n, uint32_t W, int what, void* stream)
	{
	LC_CHECK_ARGS ();
	GDSP_REQUIRE ((n == 0) || (d_x != d_y), "the track must not alias the signal");
	if (n == 0) return GDSP_OK;
	GDSP_REQUIRE ((d_x != NULL) && (d_y != NULL), "NULL vector");
	GDSP_REQUIRE (gdsp_aligned16 (d_x) && gdsp_aligned16 (d_y), "vectors must be 16-byte aligned");
	gdsp_batch_item item = { d_x, d_y, n };
	return localcorr_run (&item, 1, W, what, stream);                     // the same launches, a table of one
	}

int gdsp_localcorr_batch (const gdsp_batch_item* items, int nitems, uint32_t W, int what, void* stream)
	{
	LC_CHECK_ARGS ();
	int rc = gdsp_batch_check (items, nitems, false);
	if (rc != GDSP_OK) return rc;
	if (nitems == 0) return GDSP_OK;
	return localcorr_run (items, nitems, W, what, stream);
	}

void gdsp_localcorr_times (double ms[2]) { for (int k=0 ; k<2 ; k++) ms[k] = lcTimes[k]; }

} // extern "C"
