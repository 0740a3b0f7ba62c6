// gdsp_localstats.hip -- localstats: every base against the mean and variance of the window centred on it.
//
// Not an operator of the reference.  Definition (include/genodsp_hip.h): slidingsum's window [lo, hi] =
// [max(0, c-lft), min(n-1, c+rgt)], rgt = (W-1)/2, lft = W-1-rgt, m = hi-lo+1; S1 = sum of v, S2 = sum of fl(v v) over
// it; mean = fl(S1/m), N = fl(fl(m S2) - fl(S1 S1)), variance = N <= 0 ? +0 : fl(N / fl(m m)), stddev = sqrt(variance);
// the written value is one of them, or v relative to them.  Every step is one rounded operation (__dmul_rn and friends:
// never contracted); only the two window sums may be associated freely.
//
// One workgroup of THREADS threads owns T outputs and stages the NS = 16 THREADS inputs they read (HL + T + HR, the
// two reaches rounded up to even so that every tile starts on a 16-byte boundary of the vector; positions outside the
// vector are staged as 0.0, which is what truncates the window at the chromosome ends).  Per tile:
//   1. the staged values go to LDS in blocks of 16 at a pitch of 17 doubles: a lane stride of 17 is conflict-free for
//      8-byte reads and writes;
//   2. thread p sums block p, v and fl(v v), and a scan over the workgroup leaves b1[k], b2[k] = the sums of blocks
//      0 .. k-1.  P(x), the sum of the staged positions below x, is then b[x/16] plus up to 15 values of block x/16;
//   3. a thread takes `per` consecutive outputs (T spread over the threads as far as ls_per's choice of strides allows:
//      the divisions and the square root are the larger part of the work and should not go to T/16 lanes only).  It forms
//      P(a) and P(a+W) for its first window, both sums each, and slides both ends one base per output; S = P(a+W) - P(a).
//      No sum reaches further than the staged tile: at most T bases to the left of a window, none to the right;
//   4. the results wait in registers until every thread has read the inputs, go back to LDS and leave as 16-byte
//      non-temporal stores.
// Two forms: 512 threads and 8192 staged values (76.3 KiB of LDS, two workgroups per CU) while that leaves a tile of
// at least 4096 outputs, 1024 threads and 16384 staged values (152.4 KiB, one per CU) for the longer windows.

#include "gdsp_common.h"

#define LS_G        16                                                    // staged positions per block
#define LS_PITCH    17                                                    // doubles from one block to the next in LDS
#define LS_SMALL    512                                                   // threads of the two forms
#define LS_LARGE    1024
#define LS_MIN_TILE 4096                                                  // the small form is used while its tile is at least this
#define LS_NWHAT    6

template <int THREADS>
struct LsLds
	{
	double v[(THREADS + 1) * LS_PITCH];                                   // staged inputs (one spare block: P(NS) looks at none of it); the results in the end
	double b1[THREADS + 1], b2[THREADS + 1];                              // [k]: sums of blocks 0 .. k-1
	double w1[THREADS / 64], w2[THREADS / 64];                            // the waves' totals
	};
static_assert (2 * sizeof (LsLds<LS_SMALL>) <= 160 * 1024, "two workgroups per CU");
static_assert (sizeof (LsLds<LS_LARGE>) <= 160 * 1024, "one workgroup per CU");

// host and device: the reaches rounded up to even, the form, the outputs per tile and per thread
__host__ __device__ constexpr uint32_t ls_even (uint32_t w) { return (w + 1) & ~1u; }
__host__ __device__ constexpr bool     ls_small (uint32_t lft, uint32_t rgt) { return ls_even (lft) + ls_even (rgt) + LS_MIN_TILE <= LS_SMALL * LS_G; }
__host__ __device__ constexpr uint32_t ls_tile (uint32_t lft, uint32_t rgt)
	{ return (ls_small (lft, rgt)? LS_SMALL : LS_LARGE) * LS_G - ls_even (lft) - ls_even (rgt); }
static_assert (ls_tile ((GDSP_LOCALSTATS_MAX_WINDOW - 1) - (GDSP_LOCALSTATS_MAX_WINDOW - 1) / 2, (GDSP_LOCALSTATS_MAX_WINDOW - 1) / 2) == LS_MIN_TILE,
               "the largest window leaves the long form a tile of 4096 outputs");
// Lane l of a wave reads staged position c + l per, which lies at c + l per + (c + l per) / 16 in LDS.  Over the 32 lanes
// that share an LDS cycle those are 32 different banks for per = 16 (a stride of 17 doubles) and at most two to a bank
// for 7, 8, 11, 13 and 14, whatever c is; 15 and 10 put eight on one bank, 5 and 6 six or seven.  So `per` is the
// smallest of the good ones that covers the tile.
__host__ __device__ __forceinline__ uint32_t ls_per (uint32_t T, uint32_t threads)
	{
	const uint32_t need = (T + threads - 1) / threads;                    // <= LS_G, as T <= threads LS_G
	return (need <= 7)? 7 : (need <= 8)? 8 : (need <= 11)? 11 : (need <= 13)? 13 : (need <= 14)? 14 : LS_G;
	}

__device__ __forceinline__ int ls_at (int e) { return e + (e >> 4); }    // where staged position e lies in LsLds::v

// P(x): the sums of v and fl(v v) over the staged positions below x (x <= NS)
template <int THREADS>
__device__ __forceinline__ void ls_prefix (const LsLds<THREADS>& S, int x, double& p1, double& p2)
	{
	const int blk = x >> 4, r = x & 15;
	const double* xb = S.v + blk * LS_PITCH;
	p1 = S.b1[blk];  p2 = S.b2[blk];
#pragma unroll
	for (int k=0 ; k<LS_G-1 ; k++)
		{
		const double y = xb[k];                                           // (inside the array whatever r is)
		if (k < r) { p1 = __dadd_rn (p1, y);  p2 = __dadd_rn (p2, __dmul_rn (y, y)); }
		}
	}

struct LsArgs { uint32_t W, lft, rgt, per;  int haveFloor, haveMinSd;  double floor, minSd; };

template <int WHAT>
__device__ __forceinline__ double ls_figure (double x, double S1, double S2, double md, const LsArgs& A)
	{
	const double mean = __ddiv_rn (S1, md);
	if ((WHAT == GDSP_LOCALSTATS_MEAN) || (WHAT == GDSP_LOCALSTATS_DIFFERENCE) || (WHAT == GDSP_LOCALSTATS_RATIO))
		{
		const double bg = (A.haveFloor && (A.floor > mean))? A.floor : mean;
		if (WHAT == GDSP_LOCALSTATS_MEAN)       return bg;
		if (WHAT == GDSP_LOCALSTATS_DIFFERENCE) return __dsub_rn (x, bg);
		return (bg == 0.0)? 0.0 : __ddiv_rn (x, bg);
		}
	const double N   = __dsub_rn (__dmul_rn (md, S2), __dmul_rn (S1, S1));
	const double var = (N <= 0.0)? 0.0 : __ddiv_rn (N, __dmul_rn (md, md));
	if (WHAT == GDSP_LOCALSTATS_VARIANCE) return var;
	double sd = __dsqrt_rn (var);
	if (A.haveMinSd && (A.minSd > sd)) sd = A.minSd;
	if (WHAT == GDSP_LOCALSTATS_STDDEV) return sd;
	return (sd == 0.0)? 0.0 : __ddiv_rn (__dsub_rn (x, mean), sd);
	}

template <int THREADS, int WHAT>
__global__ __launch_bounds__(THREADS)
void localstats_kernel (GdspBatch B, LsArgs A)                            // one grid over every vector of the table (gdsp_common.h)
	{
	constexpr int NS = THREADS * LS_G;
	__shared__ __attribute__((aligned(16))) LsLds<THREADS> S;
	const double* in;  double* out;  uint32_t n;
	const uint32_t tile = gdsp_batch_tile (B, in, out, n);
	const int     tid  = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int     HL   = (int) ls_even (A.lft);
	const int     T    = NS - HL - (int) ls_even (A.rgt);
	const int64_t o0   = (int64_t) tile * T;                              // first output of the tile (even)
	const int64_t g0   = o0 - HL;                                         // first staged base (even; negative in tile 0)

	// ---- 1. stage
	if ((g0 >= 0) && (g0 + NS <= (int64_t) n))
		{
		const double2* src = reinterpret_cast<const double2*> (in + g0);
		double2 r[LS_G/2];
#pragma unroll
		for (int u=0 ; u<LS_G/2 ; u++) r[u] = gdsp_ld2 (&src[u*THREADS + tid]);         // all loads in flight
#pragma unroll
		for (int u=0 ; u<LS_G/2 ; u++)
			{
			double* dst = S.v + ls_at (2 * (u*THREADS + tid));            // (an even position and the next share a block)
			dst[0] = r[u].x;  dst[1] = r[u].y;
			}
		}
	else
		{
		for (int e=tid ; e<NS ; e+=THREADS)
			{
			const int64_t g = g0 + e;
			S.v[ls_at (e)] = ((g >= 0) && (g < (int64_t) n))? in[g] : 0.0;
			}
		}
	__syncthreads ();

	// ---- 2. block sums and their running sums
		{
		const double* xb = S.v + tid * LS_PITCH;
		double run1 = 0.0, run2 = 0.0;
#pragma unroll
		for (int u=0 ; u<LS_G ; u++) { const double y = xb[u];  run1 = __dadd_rn (run1, y);  run2 = __dadd_rn (run2, __dmul_rn (y, y)); }
		for (int d=1 ; d<64 ; d*=2)
			{
			const double u1 = __shfl_up (run1, d, 64), u2 = __shfl_up (run2, d, 64);
			if (lane >= d) { run1 = __dadd_rn (run1, u1);  run2 = __dadd_rn (run2, u2); }
			}
		if (lane == 63) { S.w1[wave] = run1;  S.w2[wave] = run2; }
		if (tid == 0) { S.b1[0] = 0.0;  S.b2[0] = 0.0; }
		__syncthreads ();
		double before1 = 0.0, before2 = 0.0;
		for (int w=0 ; w<wave ; w++) { before1 = __dadd_rn (before1, S.w1[w]);  before2 = __dadd_rn (before2, S.w2[w]); }
		S.b1[tid + 1] = __dadd_rn (before1, run1);
		S.b2[tid + 1] = __dadd_rn (before2, run2);
		}
	__syncthreads ();

	// ---- 3. `per` consecutive outputs per thread
	const int o  = tid * (int) A.per;                                     // my first output, in the tile
	const int a0 = HL - (int) A.lft + o;                                  // its window is the staged positions [a0, a0+W)
	double res[LS_G];
	double l1 = 0.0, l2 = 0.0, r1 = 0.0, r2 = 0.0;
	if ((o < T) && (o0 + o < (int64_t) n))
		{
		ls_prefix (S, a0, l1, l2);
		ls_prefix (S, a0 + (int) A.W, r1, r2);
		}
#pragma unroll
	for (int u=0 ; u<LS_G ; u++)
		{
		const int64_t c = o0 + o + u;                                     // the base
		res[u] = 0.0;
		if ((u >= (int) A.per) || (o + u >= T) || (c >= (int64_t) n)) continue;
		if (u > 0)
			{
			const double yl = S.v[ls_at (a0 + u - 1)], yr = S.v[ls_at (a0 + (int) A.W + u - 1)];
			l1 = __dadd_rn (l1, yl);  l2 = __dadd_rn (l2, __dmul_rn (yl, yl));
			r1 = __dadd_rn (r1, yr);  r2 = __dadd_rn (r2, __dmul_rn (yr, yr));
			}
		const int64_t lo = (c > (int64_t) A.lft)? c - A.lft : 0;
		const int64_t hi = (c + A.rgt < (int64_t) n - 1)? c + A.rgt : (int64_t) n - 1;
		res[u] = ls_figure<WHAT> (S.v[ls_at (HL + o + u)], __dsub_rn (r1, l1), __dsub_rn (r2, l2), (double) (hi - lo + 1), A);
		}
	__syncthreads ();                                                     // every thread has read the inputs

	// ---- 4. the outputs, through LDS, two per lane (T and o0 are even)
#pragma unroll
	for (int u=0 ; u<LS_G ; u++)
		if ((u < (int) A.per) && (o + u < T)) S.v[ls_at (o + u)] = res[u];
	__syncthreads ();
	for (int q=tid ; 2*q<T ; q+=THREADS)
		{
		const int64_t g = o0 + 2*q;
		if (g >= (int64_t) n) break;
		const double* y = S.v + ls_at (2*q);
		if (g + 1 < (int64_t) n) gdsp_st2 (reinterpret_cast<double2*> (out + g), make_double2 (y[0], y[1]));
		else                     out[g] = y[0];
		}
	}

template <int THREADS>
static void localstats_launch (const GdspBatch& B, uint32_t tiles, int what, const LsArgs& A, hipStream_t s)
	{
	switch (what)
		{
		case GDSP_LOCALSTATS_ZSCORE:     hipLaunchKernelGGL ((localstats_kernel<THREADS, GDSP_LOCALSTATS_ZSCORE>),     dim3(tiles), dim3(THREADS), 0, s, B, A);  break;
		case GDSP_LOCALSTATS_MEAN:       hipLaunchKernelGGL ((localstats_kernel<THREADS, GDSP_LOCALSTATS_MEAN>),       dim3(tiles), dim3(THREADS), 0, s, B, A);  break;
		case GDSP_LOCALSTATS_VARIANCE:   hipLaunchKernelGGL ((localstats_kernel<THREADS, GDSP_LOCALSTATS_VARIANCE>),   dim3(tiles), dim3(THREADS), 0, s, B, A);  break;
		case GDSP_LOCALSTATS_STDDEV:     hipLaunchKernelGGL ((localstats_kernel<THREADS, GDSP_LOCALSTATS_STDDEV>),     dim3(tiles), dim3(THREADS), 0, s, B, A);  break;
		case GDSP_LOCALSTATS_DIFFERENCE: hipLaunchKernelGGL ((localstats_kernel<THREADS, GDSP_LOCALSTATS_DIFFERENCE>), dim3(tiles), dim3(THREADS), 0, s, B, A);  break;
		default:                         hipLaunchKernelGGL ((localstats_kernel<THREADS, GDSP_LOCALSTATS_RATIO>),      dim3(tiles), dim3(THREADS), 0, s, B, A);  break;
		}
	}

static int localstats_run (const gdsp_batch_item* items, int nitems, uint32_t W, int what,
                           int haveFloor, double floor, int haveMinSd, double minSd, void* stream)
	{
	LsArgs A;
	A.W = W;  A.rgt = (W - 1) / 2;  A.lft = (W - 1) - A.rgt;
	const bool     small = ls_small (A.lft, A.rgt);
	const uint64_t T     = ls_tile (A.lft, A.rgt);
	A.per = ls_per ((uint32_t) T, small? LS_SMALL : LS_LARGE);
	A.haveFloor = haveFloor? 1 : 0;  A.floor = floor;  A.haveMinSd = haveMinSd? 1 : 0;  A.minSd = minSd;
	hipStream_t s = gdsp_stream (stream);
	gdsp_batch_run (items, nitems, [=] (uint32_t n) { return ((uint64_t) n + T - 1) / T; },
		[&] (const GdspBatch& B, uint32_t tiles)
			{
			if (small) localstats_launch<LS_SMALL> (B, tiles, what, A, s);
			else       localstats_launch<LS_LARGE> (B, tiles, what, A, s);
			});
	GDSP_LAUNCH_CHECK ();
	return GDSP_OK;
	}

#define LS_CHECK_ARGS() \
	GDSP_REQUIRE (W >= 1, "window must be >= 1"); \
	GDSP_REQUIRE (W <= GDSP_LOCALSTATS_MAX_WINDOW, "window above GDSP_LOCALSTATS_MAX_WINDOW"); \
	GDSP_REQUIRE ((what >= 0) && (what < LS_NWHAT), "what must be one of GDSP_LOCALSTATS_ZSCORE ... GDSP_LOCALSTATS_RATIO")

extern "C" {

uint32_t gdsp_localstats_tile (uint32_t W)
	{
	if ((W < 1) || (W > GDSP_LOCALSTATS_MAX_WINDOW)) return 0;
	const uint32_t rgt = (W - 1) / 2;
	return ls_tile ((W - 1) - rgt, rgt);
	}

int gdsp_localstats (const double* d_in, double* d_out, uint32_t n, uint32_t W, int what,
                     int haveFloor, double floor, int haveMinSd, double minSd, void* stream)
	{
	LS_CHECK_ARGS ();
	GDSP_REQUIRE ((n == 0) || (d_in != d_out), "out-of-place operator: d_out must not alias d_in");
	if (n == 0) return GDSP_OK;
	GDSP_REQUIRE ((d_in != NULL) && (d_out != NULL), "NULL vector");
	GDSP_REQUIRE (gdsp_aligned16 (d_in) && gdsp_aligned16 (d_out), "vectors must be 16-byte aligned");
	gdsp_batch_item item = { d_in, d_out, n };
	return localstats_run (&item, 1, W, what, haveFloor, floor, haveMinSd, minSd, stream);      // the same kernel, a table of one
	}

int gdsp_localstats_batch (const gdsp_batch_item* items, int nitems, uint32_t W, int what,
                           int haveFloor, double floor, int haveMinSd, double minSd, void* stream)
	{
	LS_CHECK_ARGS ();
	int rc = gdsp_batch_check (items, nitems, false);
	if (rc != GDSP_OK) return rc;
	if (nitems == 0) return GDSP_OK;
	return localstats_run (items, nitems, W, what, haveFloor, floor, haveMinSd, minSd, stream);
	}

} // extern "C"
