// gdsp_window_sums_tile.h -- what gdsp_localstats.hip (localstats) and gdsp_localcorr.hip (localcorrelate) build alike: the
// sums of a few terms per base -- localstats' v and fl(v v), localcorrelate's x, y, fl(x x), fl(y y) and fl(x y) -- over the
// window [max(0, c-lft), min(n-1, c+rgt)] centred on every base c of a tile, and a figure of them written per base.
//
// One workgroup of THREADS threads owns T outputs and stages the NS = 16 THREADS positions they read (HL + T + HR, the two
// reaches rounded up to even so that every tile starts on a 16-byte boundary of the vector; positions outside the vector are
// staged as 0.0, which is what truncates the window at the chromosome ends).  Per tile:
//   1. the staged values of each input go to LDS in blocks of 16 at a pitch of 17 doubles (ws_stage, or the user's own
//      staging through ws_at): a lane stride of 17 is conflict-free for 8-byte reads and writes;
//   2. thread p sums block p, every sum, and a scan over the workgroup leaves b[s][k] = sum s over blocks 0 .. k-1
//      (ws_block_sums).  P(e), the sums over the staged positions below e, is then b[.][e/16] plus up to 15 terms of block
//      e/16 (ws_prefix);
//   3. a thread takes `per` consecutive outputs (T spread over the threads as far as ws_per's choice of strides allows: the
//      divisions and square roots of the figure are the larger part of the work and should not go to T/16 lanes only).  It
//      forms P(a) and P(a+W) for its first window and slides both ends one base per output; S = P(a+W) - P(a).  No sum
//      reaches further than the staged tile: at most T bases to the left of a window, none to the right;
//   4. the results wait in registers until every thread has read the inputs (a barrier), go back to LDS over the first
//      input and leave as 16-byte non-temporal stores (3 and 4: ws_outputs).
// The sums may be associated freely by the operators' definitions; this is the association: a block from 0.0 over its 16
// positions in order, the __shfl_up ladder over a wave, the totals of the waves before in order from 0.0 and then the
// thread's own, P(e) as b[e/16] plus the block's first e%16 terms in order, one term per end and output in the slide.
//
// A user describes its terms by a type with INPUTS, SUMS and add (p, in): what the staged position whose INPUTS values are
// `in` adds to the SUMS sums `p`, each step one rounded operation.
#pragma once

#include "gdsp_common.h"

#define WS_G     16                                                       // staged positions per block
#define WS_PITCH 17                                                       // doubles from one block to the next in LDS

struct WsArgs { uint32_t W, lft, rgt, per; };                             // the window, its two reaches, outputs per thread

static inline WsArgs ws_window (uint32_t W) { const uint32_t rgt = (W - 1) / 2;  return WsArgs { W, (W - 1) - rgt, rgt, 0 }; }   // (per: the user's to set)

template <int THREADS, int INPUTS, int SUMS>
struct WsLds
	{
	double v[INPUTS][(THREADS + 1) * WS_PITCH];                           // staged inputs (one spare block: P(NS) looks at none of it); [0] the results in the end
	double b[SUMS][THREADS + 1];                                          // [s][k]: sum s over blocks 0 .. k-1
	double w[SUMS][THREADS / 64];                                         // the waves' totals
	};

// host and device: a reach rounded up to even, the outputs per tile and per thread
__host__ __device__ constexpr uint32_t ws_even (uint32_t w) { return (w + 1) & ~1u; }
__host__ __device__ constexpr uint32_t ws_tile (uint32_t threads, uint32_t lft, uint32_t rgt) { return threads * WS_G - ws_even (lft) - ws_even (rgt); }
// Lane l of a wave reads staged position c + l per, which lies at c + l per + (c + l per) / 16 in LDS.  Over the 32 lanes
// that share an LDS cycle those are 32 different banks for per = 16 (a stride of 17 doubles) and at most two to a bank
// for 7, 8, 11, 13 and 14, whatever c is; 15 and 10 put eight on one bank, 5 and 6 six or seven.  So `per` is the
// smallest of the good ones that covers the tile.  (localcorrelate's tile is at least 4096 outputs on 512 threads: its
// need is 8 to 16 and it never takes the 7.)
__host__ __device__ __forceinline__ uint32_t ws_per (uint32_t T, uint32_t threads)
	{
	const uint32_t need = (T + threads - 1) / threads;                    // <= WS_G, as T <= threads WS_G
	return (need <= 7)? 7 : (need <= 8)? 8 : (need <= 11)? 11 : (need <= 13)? 13 : (need <= 14)? 14 : WS_G;
	}

__device__ __forceinline__ int ws_at (int e) { return e + (e >> 4); }    // where staged position e lies in WsLds::v[.]

// a tile's place: HL staged positions, then its T outputs from base o0 of the vector on; g0 = the first staged base
struct WsTile { int HL, T;  int64_t o0, g0; };

template <int THREADS>
__device__ __forceinline__ WsTile ws_tile_of (const WsArgs& A, uint32_t tile)
	{
	WsTile t;
	t.HL = (int) ws_even (A.lft);
	t.T  = (int) ws_tile (THREADS, A.lft, A.rgt);
	t.o0 = (int64_t) tile * t.T;                                          // (even)
	t.g0 = t.o0 - t.HL;                                                   // (even; negative in tile 0)
	return t;
	}

// ---- 1. stage one input whole from global memory into its LDS image v, 0.0 outside the vector
template <int THREADS>
__device__ __forceinline__ void ws_stage (double* v, const double* in, int64_t g0, uint32_t n)
	{
	constexpr int NS = THREADS * WS_G;
	const int tid = threadIdx.x;
	if ((g0 >= 0) && (g0 + NS <= (int64_t) n))
		{
		const double2* src = reinterpret_cast<const double2*> (in + g0);
		double2 r[WS_G/2];
#pragma unroll
		for (int u=0 ; u<WS_G/2 ; u++) r[u] = gdsp_ld2 (&src[u*THREADS + tid]);         // all loads in flight
#pragma unroll
		for (int u=0 ; u<WS_G/2 ; u++)
			{
			double* dst = v + ws_at (2 * (u*THREADS + tid));                  // (an even position and the next share a block)
			dst[0] = r[u].x;  dst[1] = r[u].y;
			}
		}
	else
		{
		for (int e=tid ; e<NS ; e+=THREADS)
			{
			const int64_t g = g0 + e;
			v[ws_at (e)] = ((g >= 0) && (g < (int64_t) n))? in[g] : 0.0;
			}
		}
	}

// the inputs' values at index base + k of their LDS images
template <int THREADS, int INPUTS, int SUMS>
__device__ __forceinline__ void ws_read (const WsLds<THREADS, INPUTS, SUMS>& S, int base, int k, double in[INPUTS])
	{
#pragma unroll
	for (int i=0 ; i<INPUTS ; i++) in[i] = (S.v[i] + base)[k];
	}

// ---- 2. block sums and their running sums, behind the staging and ahead of the first P(e)
template <int THREADS, class Terms>
__device__ __forceinline__ void ws_block_sums (WsLds<THREADS, Terms::INPUTS, Terms::SUMS>& S)
	{
	constexpr int SUMS = Terms::SUMS;
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	__syncthreads ();                                                     // the inputs are staged
	double run[SUMS], in[Terms::INPUTS];
#pragma unroll
	for (int s=0 ; s<SUMS ; s++) run[s] = 0.0;
#pragma unroll
	for (int u=0 ; u<WS_G ; u++) { ws_read (S, tid * WS_PITCH, u, in);  Terms::add (run, in); }
	for (int d=1 ; d<64 ; d*=2)
		{
#pragma unroll
		for (int s=0 ; s<SUMS ; s++)
			{
			const double up = __shfl_up (run[s], d, 64);
			if (lane >= d) run[s] = __dadd_rn (run[s], up);
			}
		}
	if (lane == 63)
		{
#pragma unroll
		for (int s=0 ; s<SUMS ; s++) S.w[s][wave] = run[s];
		}
	if (tid < SUMS) S.b[tid][0] = 0.0;
	__syncthreads ();
	double before[SUMS];
#pragma unroll
	for (int s=0 ; s<SUMS ; s++) before[s] = 0.0;
	for (int w=0 ; w<wave ; w++)                                          // (one loop for all sums: every total is read at once, not sum by sum)
		{
#pragma unroll
		for (int s=0 ; s<SUMS ; s++) before[s] = __dadd_rn (before[s], S.w[s][w]);
		}
#pragma unroll
	for (int s=0 ; s<SUMS ; s++) S.b[s][tid + 1] = __dadd_rn (before[s], run[s]);
	__syncthreads ();
	}

// P(e): the sums over the staged positions below e (e <= NS)
template <int THREADS, class Terms>
__device__ __forceinline__ void ws_prefix (const WsLds<THREADS, Terms::INPUTS, Terms::SUMS>& S, int e, double p[Terms::SUMS])
	{
	const int blk = e >> 4, r = e & 15;
	double in[Terms::INPUTS];
#pragma unroll
	for (int s=0 ; s<Terms::SUMS ; s++) p[s] = S.b[s][blk];
#pragma unroll
	for (int k=0 ; k<WS_G-1 ; k++)
		{
		ws_read (S, blk * WS_PITCH, k, in);                         // (inside the arrays whatever r is)
		if (k < r) Terms::add (p, in);
		}
	}

// ---- 3 and 4. `per` consecutive outputs per thread, figure (e, S, m) each: e = the staged position of the base (readable
// in S.v until the barrier), S = its window's sums, m = its window's length; then through LDS to out[o0 ..), two per lane
// (T and o0 are even: no pair straddles a tile)
template <int THREADS, class Terms, class Figure>
__device__ __forceinline__ void ws_outputs (WsLds<THREADS, Terms::INPUTS, Terms::SUMS>& S, const WsArgs& A, const WsTile& t,
                                            uint32_t n, double* out, const Figure figure)
	{
	constexpr int SUMS = Terms::SUMS;
	const int tid = threadIdx.x, T = t.T;
	const int o  = tid * (int) A.per;                                     // my first output, in the tile
	const int a0 = t.HL - (int) A.lft + o;                                // its window is the staged positions [a0, a0+W)
	double res[WS_G];
	double l[SUMS], r[SUMS], in[Terms::INPUTS];
#pragma unroll
	for (int s=0 ; s<SUMS ; s++) l[s] = r[s] = 0.0;
	if ((o < T) && (t.o0 + o < (int64_t) n))
		{
		ws_prefix<THREADS, Terms> (S, a0, l);
		ws_prefix<THREADS, Terms> (S, a0 + (int) A.W, r);
		}
#pragma unroll
	for (int u=0 ; u<WS_G ; u++)
		{
		const int64_t c = t.o0 + o + u;                                   // the base
		res[u] = 0.0;
		if ((u >= (int) A.per) || (o + u >= T) || (c >= (int64_t) n)) continue;
		if (u > 0)
			{
			ws_read (S, ws_at (a0 + u - 1), 0, in);               Terms::add (l, in);
			ws_read (S, ws_at (a0 + (int) A.W + u - 1), 0, in);   Terms::add (r, in);
			}
		const int64_t lo = (c > (int64_t) A.lft)? c - A.lft : 0;
		const int64_t hi = (c + A.rgt < (int64_t) n - 1)? c + A.rgt : (int64_t) n - 1;
		double sums[SUMS];
#pragma unroll
		for (int s=0 ; s<SUMS ; s++) sums[s] = __dsub_rn (r[s], l[s]);
		res[u] = figure (t.HL + o + u, sums, (double) (hi - lo + 1));
		}
	__syncthreads ();                                                     // every thread has read the inputs

#pragma unroll
	for (int u=0 ; u<WS_G ; u++)
		if ((u < (int) A.per) && (o + u < T)) S.v[0][ws_at (o + u)] = res[u];
	__syncthreads ();
	for (int q=tid ; 2*q<T ; q+=THREADS)
		{
		const int64_t g = t.o0 + 2*q;
		if (g >= (int64_t) n) break;
		const double* y = S.v[0] + ws_at (2*q);
		if (g + 1 < (int64_t) n) gdsp_st2 (reinterpret_cast<double2*> (out + g), make_double2 (y[0], y[1]));
		else                     out[g] = y[0];
		}
	}
