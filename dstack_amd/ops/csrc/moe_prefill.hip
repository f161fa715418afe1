// Routed expert GEMM for prefill (more than 256 token rows) on CDNA4 (gfx950): a tiled, compute-bound
// grouped GEMM beside the weight-streaming decode kernels (moe.hip, moe_fine.hip), for up to 2048 rows,
// 128 experts and 8 experts per token.
//
//   moe_prefill_plan   the live pairs grouped by expert into tiles of TM pairs, no host read
//   moe_prefill_gemm   part[0][p][:] = x[p / src_div] W[expert(p)]^T for the pairs of every tile, or, with
//                      the gate/up epilogue, a[p][:] = bf16(silu(g) u) straight from the accumulators
//
// A decode step is bound by reading the chosen experts' weights once, and the decode kernels stream them
// past a few token rows.  A prefill of thousands of rows gives every expert a hundred pairs and more: run
// in 256-row slices through the decode kernels it re-reads every expert once per slice.  Here a tile of
// pairs meets a tile of weight rows in LDS and every weight byte is read once per TM pairs of its expert.
//
// Plan.  One workgroup: a histogram of the pairs' experts in LDS (vector LDS atomics), an exclusive
// prefix sum of the experts' tile counts ceil(count / TM), a scatter of the pairs p = row k + j into their
// expert's tiles and -1 into the rest of every ragged tile.  tile_e[t] is the expert of tile t, -1 for
// the tiles past the last one.  The tiles number at most P / TM + min(E, P) whatever the routing (a sum of
// ceilings is at most the floor of the sum plus one per non-empty expert), so the GEMM's grid is sized by
// the shape alone and surplus workgroups leave at once.  The order of the pairs inside an expert's group
// is whatever the atomics give: a pair's output row is computed from its own operands in a fixed order of
// K, so its bits do not depend on its place.
//
// GEMM.  A workgroup of 4 waves owns TM pairs x 128 weight rows of one expert and runs the whole K (no
// split: the shape is compute-bound, and the fp32 partials of a split would be the larger traffic):
//  * K-steps of 64 elements, LDS double-buffered: 128-byte rows, TM of gathered x rows and 128 of W.  A
//    thread loads 16-byte pieces (8 lanes a row) of step t + 1 into registers before the MFMAs of step t
//    and stores them into the other half after them; one barrier per step.  Padding pairs (-1) are not
//    loaded: their LDS rows are zeros, and nothing of them is stored;
//  * the 16-byte chunk c of row r sits at chunk c ^ ((r >> 1) & 7): 16 consecutive rows of one chunk column
//    cover all 64 banks once, for the fragment reads (a lane reads row lane & 31, chunk 2 kk + (lane >> 5)) as
//    for the stores (16 lanes = 2 rows x 8 chunks);
//  * waves 2 x 2: a wave holds TM / 2 pairs x 64 weight rows as (TM / 64) x 2 accumulators of
//    v_mfma_f32_32x32x16_bf16, pairs as the M operand, weight rows as N, so that a lane's accumulator
//    element i is pair 8 (i / 4) + 4 (lane >> 5) + i % 4, weight row lane & 31: a store instruction writes
//    whole 128-byte lines of `part`;
//  * TM is 128 or 64, the caller's choice from the shape alone (ops.serving.moe_prefill_tile: 128 where
//    an expert has 96 pairs or more on average): at 128 experts and 384 rows an expert has 24 pairs, and
//    a 128-pair tile would multiply mostly zeros;
//  * plain epilogue: fp32 part[p][n], the tensor moe_gemm writes with one K slice (moe_combine reads it);
//  * gate/up epilogue: the workgroup's 128 weight rows are gate rows n0 .. n0 + 63 and up rows F + n0 ..,
//    laid out so that a wave's two accumulators of a pair block are g and u of the same 32 columns: a lane
//    holds g and u of one element and writes bf16(silu(g) u) with moe_swiglu's device function
//    (moe_frag.h: moe_silu_mul) -- the bits of moe_swiglu over the plain epilogue's partials, without
//    writing and reading the fp32 gate/up tensor.
//
// Every index read from memory (tile_e, pairs, topk_e) is checked against its range before it addresses
// anything.
#include <stdint.h>

#include "moe_frag.h"
#include "moe_host.h"

using namespace dsa;
using namespace dsa::moe;

namespace {

constexpr int PF_MAXE = 128;   // experts
constexpr int PF_BN = 128;     // weight rows per workgroup
constexpr int PF_BK = 64;      // K elements per step (128-byte LDS rows)
constexpr int PF_PLAN_THREADS = 1024;

struct PrefillArgs {
  const bf16_t* X;    // bf16 [xrows][ldx]
  const bf16_t* W;    // bf16 [E][N][K]
  const int* tile_e;  // [tiles]
  const int* pairs;   // [tiles][TM]
  float* part;        // plain epilogue: fp32 [P][N]
  bf16_t* A;          // gate/up epilogue: bf16 [P][N / 2]
  long ldx;           // elements
  int xrows, src_div, P, E, N, K;
};

// ================================================================================================
// Plan
// ================================================================================================
// tm = 1 << shift pairs per tile, tcap tiles in tile_e and pairs
__global__ __launch_bounds__(PF_PLAN_THREADS) void moe_prefill_plan_kernel(const int* __restrict__ topk_e,
                                                                           const int* __restrict__ live,
                                                                           int* __restrict__ tile_e, int* __restrict__ pairs,
                                                                           int P, int k, int E, int shift, int tcap) {
  __shared__ int cnt[PF_MAXE], base[PF_MAXE], cur[PF_MAXE];
  __shared__ int total;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, tm = 1 << shift, cap = tcap << shift;
  if (tid < PF_MAXE) cnt[tid] = 0, cur[tid] = 0;
  __syncthreads();
  for (int p = tid; p < P; p += PF_PLAN_THREADS) {
    const int e = topk_e[p];
    if (e >= 0 && e < E && live[p / k] > 0) atomicAdd(&cnt[e], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int t = 0;
    for (int e = 0; e < E; ++e) {
      base[e] = t;  // first tile of expert e
      t += (cnt[e] + tm - 1) >> shift;
    }
    total = min(t, tcap);  // (t <= tcap for any routing: the header)
  }
  __syncthreads();
  for (int p = tid; p < P; p += PF_PLAN_THREADS) {
    const int e = topk_e[p];
    if (e >= 0 && e < E && live[p / k] > 0) {
      const int at = (base[e] << shift) + atomicAdd(&cur[e], 1);
      if (at < cap) pairs[at] = p;
    }
  }
  // a wave per expert: the rest of its ragged tile, its tiles' expert
  for (int e = w; e < E; e += PF_PLAN_THREADS / 64) {
    const int n = cnt[e], tiles = (n + tm - 1) >> shift, first = base[e];
    for (int i = n + lane; i < (tiles << shift); i += 64)
      if ((first << shift) + i < cap) pairs[(first << shift) + i] = -1;
    for (int t = lane; t < tiles; t += 64)
      if (first + t < tcap) tile_e[first + t] = e;
  }
  for (int t = total + tid; t < tcap; t += PF_PLAN_THREADS) tile_e[t] = -1;
  for (int i = (total << shift) + tid; i < cap; i += PF_PLAN_THREADS) pairs[i] = -1;
}

// ================================================================================================
// Tiled grouped GEMM
// ================================================================================================
// byte offset of 16-byte chunk c of row r in a tile of 128-byte rows
__device__ __forceinline__ int pf_swz(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

// TM pairs x 128 weight rows of the tile's expert over the whole K.  GLU: the gate/up epilogue.
template <int TM, bool GLU>
__device__ __forceinline__ void prefill_body(const PrefillArgs& p, char* smem, int* spair, const int e) {
  constexpr int MB = TM / 64;                 // 32-pair accumulator blocks per wave
  constexpr int AL = TM / 32;                 // a thread's 16-byte x pieces per step
  constexpr int WL = PF_BN / 32;              // and W pieces
  constexpr int ABYTES = TM * 128, STAGE = ABYTES + PF_BN * 128;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 1, wn = w & 1, fr = lane & 31, fh = lane >> 5;
  const int lr = tid >> 3, lc = tid & 7;  // the loads' row within a group of 32, 16-byte chunk
  const int* pl = p.pairs + (long)blockIdx.y * TM;

  if (tid < TM) {
    const int pr = pl[tid];
    spair[tid] = pr >= 0 && pr < p.P ? pr : -1;
  }
  __syncthreads();

  // --- a thread's sources: x rows through the pair list (padding: none), W rows of the expert -----------
  const bf16_t* ap[AL];
  const bf16_t* wp[WL];
  int aoff[AL], woff[WL];
#pragma unroll
  for (int i = 0; i < AL; ++i) {
    const int row = lr + 32 * i, pr = spair[row];
    const int srow = min(max(pr, 0) / p.src_div, p.xrows - 1);
    ap[i] = pr >= 0 ? p.X + (long)srow * p.ldx + lc * 8 : nullptr;
    aoff[i] = pf_swz(row, lc);
  }
#pragma unroll
  for (int i = 0; i < WL; ++i) {
    // local row j = 64 wn + 32 nb + c.  GLU: block nb = 0 holds gate rows, nb = 1 the up rows of the same columns
    const int j = lr + 32 * i;
    const int grow = GLU ? ((j & 32) ? p.N / 2 : 0) + blockIdx.x * 64 + (j >> 6) * 32 + (j & 31) : blockIdx.x * PF_BN + j;
    wp[i] = p.W + ((long)e * p.N + grow) * p.K + lc * 8;
    woff[i] = ABYTES + pf_swz(j, lc);
  }

  f32x16 acc[MB][2];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[mb][nb][i] = 0.f;

  i32x4 ra[AL], rw[WL];
  const int nsteps = p.K / PF_BK;
  // step 0 into the first half
#pragma unroll
  for (int i = 0; i < AL; ++i) ra[i] = ap[i] ? *reinterpret_cast<const i32x4*>(ap[i]) : i32x4{0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < WL; ++i) rw[i] = *reinterpret_cast<const i32x4*>(wp[i]);
#pragma unroll
  for (int i = 0; i < AL; ++i) *reinterpret_cast<i32x4*>(smem + aoff[i]) = ra[i];
#pragma unroll
  for (int i = 0; i < WL; ++i) *reinterpret_cast<i32x4*>(smem + woff[i]) = rw[i];
  __syncthreads();

  for (int t = 0; t < nsteps; ++t) {
    const bool more = t + 1 < nsteps;  // (uniform)
    if (more) {
      const int ko = (t + 1) * PF_BK;
#pragma unroll
      for (int i = 0; i < AL; ++i) ra[i] = ap[i] ? *reinterpret_cast<const i32x4*>(ap[i] + ko) : i32x4{0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < WL; ++i) rw[i] = *reinterpret_cast<const i32x4*>(wp[i] + ko);
    }
    const char* st = smem + (t & 1) * STAGE;
#pragma unroll
    for (int kk = 0; kk < PF_BK / 16; ++kk) {
      bf16x8 a[MB], b[2];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
        a[mb] = *reinterpret_cast<const bf16x8*>(st + pf_swz(wm * (TM / 2) + 32 * mb + fr, 2 * kk + fh));
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
        b[nb] = *reinterpret_cast<const bf16x8*>(st + ABYTES + pf_swz(wn * 64 + 32 * nb + fr, 2 * kk + fh));
#pragma unroll
      for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) acc[mb][nb] = mfma(a[mb], b[nb], acc[mb][nb]);
    }
    if (more) {
      // the other half: every wave left it at the barrier that ended step t - 1
      char* nx = smem + ((t + 1) & 1) * STAGE;
#pragma unroll
      for (int i = 0; i < AL; ++i) *reinterpret_cast<i32x4*>(nx + aoff[i]) = ra[i];
#pragma unroll
      for (int i = 0; i < WL; ++i) *reinterpret_cast<i32x4*>(nx + woff[i]) = rw[i];
    }
    __syncthreads();
  }

  // --- epilogue: element i of a lane is pair 8 (i / 4) + 4 fh + i % 4 of the block, weight row fr --------
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int pr = spair[wm * (TM / 2) + 32 * mb + 8 * (i >> 2) + 4 * fh + (i & 3)];
      if (pr < 0) continue;
      if constexpr (GLU) {
        const int F = p.N / 2;
        p.A[(long)pr * F + blockIdx.x * 64 + wn * 32 + fr] = f2bf(moe_silu_mul(acc[mb][0][i], acc[mb][1][i]));
      } else {
        float* dst = p.part + (long)pr * p.N + blockIdx.x * PF_BN + wn * 64 + fr;
        dst[0] = acc[mb][0][i];
        dst[32] = acc[mb][1][i];
      }
    }
}

}  // namespace

template <int TM, bool GLU>
__global__ __launch_bounds__(256, 2) void moe_prefill_gemm_kernel(PrefillArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int spair[TM];
  const int e = __builtin_amdgcn_readfirstlane(p.tile_e[blockIdx.y]);
  if (e < 0 || e >= p.E) return;  // a tile past the plan's last one
  prefill_body<TM, GLU>(p, smem, spair, e);
}

// tiles of `tile` pairs that hold any routing of R k pairs over E experts
extern "C" int dsa_moe_prefill_tiles(int R, int k, int E, int tile) {
  const int P = R * k;
  return P / tile + (E < P ? E : P);
}

static bool prefill_dims_ok(int R, int k, int E, int tile) {
  return R >= 1 && R <= MOE_PREFILL_MAXR && k >= 1 && k <= MOE_MAXK && E >= k && E <= PF_MAXE && (tile == 64 || tile == 128);
}

// tile_e [tiles], pairs [tiles][tile] (tiles = dsa_moe_prefill_tiles) from topk_e [R][k] and live [R]
extern "C" hipError_t dsa_moe_prefill_plan(const int* topk_e, const int* live, int* tile_e, int* pairs, int R, int k,
                                           int E, int tile, hipStream_t st) {
  if (!prefill_dims_ok(R, k, E, tile)) return hipErrorInvalidValue;
  moe_prefill_plan_kernel<<<1, PF_PLAN_THREADS, 0, st>>>(topk_e, live, tile_e, pairs, R * k, k, E, tile == 128 ? 7 : 6,
                                                         dsa_moe_prefill_tiles(R, k, E, tile));
  return hipGetLastError();
}

extern "C" bool dsa_moe_prefill_gemm_supported(int N, int K) {
  return N > 0 && N % PF_BN == 0 && K >= 2 * PF_BK && K % PF_BK == 0;
}

template <int TM, bool GLU>
static hipError_t prefill_launch(const PrefillArgs& a, int tiles, hipStream_t st) {
  return moe_host_launch<&moe_prefill_gemm_kernel<TM, GLU>, 2 * (TM + PF_BN) * 128>(dim3(a.N / PF_BN, tiles), 256, a, st);
}

// For the pairs p of every tile: part[p][:] = X[p / src_div] W[tile's expert]^T (fp32 [R k][N]; A null), or
// A[p][n] = bf16(silu(g) u) of g = column n, u = column N / 2 + n of that product (bf16 [R k][N / 2]; part
// null).  X bf16 [xrows][K] (row stride ldx elements), W bf16 [E][N][K], tile_e and pairs from
// dsa_moe_prefill_plan at the same R, k, E and tile.  Rows of no pair are not written.
extern "C" hipError_t dsa_moe_prefill_gemm(const void* X, long ldx, int xrows, int src_div, const void* W,
                                           const int* tile_e, const int* pairs, float* part, void* A, int R, int k,
                                           int E, int N, int K, int tile, hipStream_t st) {
  if (!prefill_dims_ok(R, k, E, tile) || !dsa_moe_prefill_gemm_supported(N, K)) return hipErrorInvalidValue;
  if ((part == nullptr) == (A == nullptr) || !moe_host_x_ok(ldx, xrows, src_div, R, k, K)) return hipErrorInvalidValue;
  const PrefillArgs a{(const bf16_t*)X, (const bf16_t*)W, tile_e, pairs, part, (bf16_t*)A, ldx, xrows, src_div, R * k, E, N, K};
  const int tiles = dsa_moe_prefill_tiles(R, k, E, tile);
  if (tile == 128) return A ? prefill_launch<128, true>(a, tiles, st) : prefill_launch<128, false>(a, tiles, st);
  return A ? prefill_launch<64, true>(a, tiles, st) : prefill_launch<64, false>(a, tiles, st);
}
