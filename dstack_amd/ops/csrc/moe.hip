// Sparse mixture-of-experts MLP (Mixtral: E experts, a linear router picks k per token) for the serving
// engine's decode and verify steps on CDNA4 (gfx950): up to 256 token rows, everything from device
// memory (no host read of the routing), so the whole MLP sits inside a captured graph.
//
//   moe_route    router logits, softmax, top-k, renormalized weights; per-expert pair lists
//   moe_gemm     part[s][p][:] = x[p / src_div] W[expert(p)]^T over K slice s, for the pairs of each expert
//   moe_swiglu   a[p] = bf16(silu(g) u) from the gate/up partials (split-K reduce fused)
//   moe_combine  y[row] = bf16(sum_j w[row][j] down[row k + j]) from the down partials (reduce fused)
//
// A pair is p = row * k + j: token row `row` on its j-th expert.  lists[e] holds the pairs routed to
// expert e in ascending order, counts[e] how many.  Rows with live <= 0 (graph padding, inert verify
// rows) have no pairs.
//
// moe_gemm.  The weights stay row-major [E][N][K] bf16 -- the one copy the eager prefill path reads
// too.  The structure is w4_gemm's (w4.hip) with the dequantizer taken out and an expert dimension
// and a row gather put in:
//  * grid = N tiles of 256 weight rows x experts x K slices; a workgroup whose expert has no pairs
//    leaves at once, so a step streams only the chosen experts' weights;
//  * 8 waves x 2 fragments of 16 weight rows.  The weights are the MFMA A operand of
//    v_mfma_f32_16x16x32_bf16: lane (r = lane & 15, gq = lane >> 4) holds weight row r, K elements
//    [8 gq, 8 gq + 8) of a 32-wide MFMA step -- 16 bytes that lie contiguous in the row-major weight,
//    so a lane's operand is one nontemporal 16-byte buffer load with no shuffle, a load instruction
//    covers 16 rows x 64 contiguous bytes and the four of a 128-element K-step each row's two whole
//    128-byte lines.  Each weight byte is loaded once, NX - 1 K-steps ahead of its MFMAs;
//  * the expert's token rows are gathered through lists[e] by LDS-DMA into a ring of 256-byte-row slots
//    (16-byte chunks XOR-swizzled with the row, as w4_gemm's), token i of the expert in slot row i;
//    they are the B operand, consumed as blocks of 16 tokens; one bare barrier per K-step;
//  * the host picks the form by the row count R alone (the most blocks an expert can hold: 1, 2, 4,
//    8 or 16); inside, the workgroup runs the K loop specialized for the smallest of those that holds
//    its expert's ceil(counts[e] / 16) blocks -- accumulators, ring slots and gather loads for that
//    many -- and skips the blocks past the count wave-uniformly;
//  * fp32 accumulation; every K slice writes fp32 partials [S][R k][N] (rows of pairs only), added in a
//    fixed order by moe_swiglu / moe_combine: no atomics, the same inputs give the same bits.
//
// Every index read from memory (counts, lists, topk_e) is clamped to its range before it addresses
// anything, so no input bits can take an access out of bounds.
//
// Device code shared with moe_fine.hip: moe_frag.h.  Launch code shared with moe_fine.hip and moe_w4.hip
// (the form ladder, the check of x, the rule for the K slices, the launch): moe_host.h.
#include <stdint.h>

#include <type_traits>

#include "moe_frag.h"
#include "moe_host.h"

using namespace dsa;
using namespace dsa::moe;

namespace {

constexpr int MOE_MAXE = 64;      // experts of moe_gemm (one lane each in the router's first form)
constexpr int MOE_MAXE2 = 128;    // experts of the router and the lists (two per lane in the router's second form)
constexpr int MOE_WG_ROWS = 256;  // weight rows per workgroup
constexpr int MOE_NWV = 8;        // waves
constexpr int MOE_UNROLL = 4;     // K-steps per K slice are a multiple of this (both ring sizes divide it)

// ================================================================================================
// Router
// ================================================================================================
// (value, index) candidates of the top-k selection: an index >= 64 marks a lane that is out of the
// running (no expert, or already taken); ties go to the lower index; values are never NaN
__device__ __forceinline__ bool moe_better(float av, int ai, float bv, int bi) {
  const bool au = ai < 64, bu = bi < 64;
  if (au != bu) return au;
  return av > bv || (av == bv && ai < bi);
}

// One workgroup per token row.  The E logits in fp32 (a wave per expert, lanes over 16-byte pieces of
// the row, a fixed summation order), then wave 0 with expert e in lane e: softmax over all E, k rounds
// of arg-max (NaN ranks below every number, a tie goes to the lower index), the k probabilities
// divided by their sum.
__global__ __launch_bounds__(256) void moe_topk_kernel(const bf16_t* __restrict__ h, long ldh,
                                                       const bf16_t* __restrict__ gate, int* __restrict__ topk_e,
                                                       float* __restrict__ topk_w, int E, int k, int D) {
  __shared__ float logit[MOE_MAXE];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bf16_t* x = h + (long)row * ldh;
  for (int e = w; e < E; e += 4) {
    const bf16_t* g = gate + (long)e * D;
    float s = 0.f;
    for (int c = lane * 8; c < D; c += 512) {
      const us8 a = *reinterpret_cast<const us8*>(x + c), b = *reinterpret_cast<const us8*>(g + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) s = __builtin_fmaf(bf2f(a[j]), bf2f(b[j]), s);
    }
    s = wave_sum(s);
    if (lane == 0) logit[e] = s;
  }
  __syncthreads();
  if (w != 0) return;
  const bool valid = lane < E;
  const float l = valid ? logit[lane] : -INFINITY;
  const float key = (l != l) ? -INFINITY : l;
  const float m = wave_max(l);  // (fmaxf drops a NaN)
  float p = valid ? expf(l - m) : 0.f;
  p = p / wave_sum(p);
  bool taken = !valid;
  int my_e = 0;
  float my_p = 0.f, sum = 0.f;
  for (int j = 0; j < k; ++j) {
    float bv = key;
    int bi = taken ? 64 + lane : lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (moe_better(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    bi = min(bi & 63, E - 1);  // (k <= E: a lane is always left; in range whatever the bits)
    const float pj = __shfl(p, bi, 64);
    if (lane == bi) taken = true;
    if (lane == j) my_e = bi, my_p = pj;
    sum += pj;
  }
  if (lane < k) {
    topk_e[row * k + lane] = my_e;
    topk_w[row * k + lane] = my_p / sum;
  }
}

// moe_better for candidates of up to 128 experts: an index >= 128 is out of the running
__device__ __forceinline__ bool moe_better2(float av, int ai, float bv, int bi) {
  const bool au = ai < 128, bu = bi < 128;
  if (au != bu) return au;
  return av > bv || (av == bv && ai < bi);
}

// The same rule for 64 < E <= 128: lane l of wave 0 holds experts l and l + 64.  A round first takes the
// better of the lane's two candidates, then runs the wave's arg-max; the winner's probability comes from
// the half of its lane that holds it.
__global__ __launch_bounds__(256) void moe_topk2_kernel(const bf16_t* __restrict__ h, long ldh,
                                                        const bf16_t* __restrict__ gate, int* __restrict__ topk_e,
                                                        float* __restrict__ topk_w, int E, int k, int D) {
  __shared__ float logit[MOE_MAXE2];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bf16_t* x = h + (long)row * ldh;
  for (int e = w; e < E; e += 4) {
    const bf16_t* g = gate + (long)e * D;
    float s = 0.f;
    for (int c = lane * 8; c < D; c += 512) {
      const us8 a = *reinterpret_cast<const us8*>(x + c), b = *reinterpret_cast<const us8*>(g + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) s = __builtin_fmaf(bf2f(a[j]), bf2f(b[j]), s);
    }
    s = wave_sum(s);
    if (lane == 0) logit[e] = s;
  }
  __syncthreads();
  if (w != 0) return;
  const bool valid1 = lane + 64 < E;  // (E > 64: expert `lane` exists in every lane)
  const float l0 = logit[lane], l1 = valid1 ? logit[lane + 64] : -INFINITY;
  const float key0 = (l0 != l0) ? -INFINITY : l0, key1 = (l1 != l1) ? -INFINITY : l1;
  const float m = wave_max(fmaxf(l0, l1));  // (fmaxf drops a NaN)
  float p0 = expf(l0 - m), p1 = valid1 ? expf(l1 - m) : 0.f;
  const float z = wave_sum(p0 + p1);
  p0 = p0 / z, p1 = p1 / z;
  bool taken0 = false, taken1 = !valid1;
  int my_e = 0;
  float my_p = 0.f, sum = 0.f;
  for (int j = 0; j < k; ++j) {
    float bv = key0;
    int bi = taken0 ? 128 + lane : lane;
    const int ci = taken1 ? 192 + lane : 64 + lane;
    if (moe_better2(key1, ci, bv, bi)) bv = key1, bi = ci;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (moe_better2(ov, oi, bv, bi)) bv = ov, bi = oi;
    }
    bi = min(bi & 127, E - 1);  // (k <= E: an expert is always left; in range whatever the bits)
    const float a0 = __shfl(p0, bi & 63, 64), a1 = __shfl(p1, bi & 63, 64);
    const float pj = bi < 64 ? a0 : a1;
    if (lane == (bi & 63)) {
      if (bi < 64) taken0 = true;
      else taken1 = true;
    }
    if (lane == j) my_e = bi, my_p = pj;
    sum += pj;
  }
  if (lane < k) {
    topk_e[row * k + lane] = my_e;
    topk_w[row * k + lane] = my_p / sum;
  }
}

// One wave per expert: the pairs p = 0, 1, .. whose expert it is and whose row is live, in ascending
// order, by ballots and prefix counts (no atomics: the order is the same every time).  The tail of
// the list is -1.
__global__ __launch_bounds__(64) void moe_lists_kernel(const int* __restrict__ topk_e, const int* __restrict__ live,
                                                       int* __restrict__ counts, int* __restrict__ lists, int R,
                                                       int k) {
  const int e = blockIdx.x, lane = threadIdx.x, P = R * k;
  int base = 0;
  for (int p0 = 0; p0 < P; p0 += 64) {
    const int p = p0 + lane;
    const bool hit = p < P && topk_e[p] == e && live[p / k] > 0;
    const unsigned long long b = __ballot(hit);
    const int at = base + __popcll(b & ((1ull << lane) - 1ull));
    if (hit && at < R) lists[e * R + at] = p;
    base += __popcll(b);
  }
  base = min(base, R);
  for (int i = base + lane; i < R; i += 64) lists[e * R + i] = -1;
  if (lane == 0) counts[e] = base;
}

// ================================================================================================
// Grouped GEMM
// ================================================================================================
// XP 1 KiB activation pieces (4 tokens x 256 B) per wave and step; pieces past the last one are the
// last one again (identical bytes to one slot), so every wave issues the same number of loads
// (LB, TB: a tag per instantiation -- see the header of stream_frag.h)
template <int XP, int LB, int TB>
__device__ __forceinline__ void moe_issue_x(__amdgpu_buffer_rsrc_t xrs, const unsigned (&xoff)[XP], char* slot, int so,
                                            int w) {
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int piece = min(w + MOE_NWV * i, 4 * LB - 1);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, LDS3(void, slot + piece * 1024), 16, xoff[i], so, 0, 0);
  }
}

// The K loop and the partial store of a workgroup whose expert e has cnt (1 .. 16 LB) pairs, with LB
// token blocks of accumulators; TB: the form of the kernel it is part of.
template <int LB, int TB>
__device__ __forceinline__ void moe_body(const MoeArgs& p, char* smem, const int e, const int cnt) {
  constexpr int NX = LB >= 16 ? 2 : 4;  // ring slots (= weight register sets): 2 beside 128 accumulators
  constexpr int D = NX - 1;             // prefetch distance in K-steps
  constexpr int XT = LB * 4096;         // one ring slot: 16 LB tokens x 256 B
  constexpr int XP = (4 * LB + MOE_NWV - 1) / MOE_NWV;  // activation pieces per wave per step
  constexpr int OPS = XP + 4 * MOE_NF;                  // vector-memory ops per wave per step
  static_assert(LB <= TB && MOE_NWV * MOE_NF * 16 == MOE_WG_ROWS && MOE_UNROLL % NX == 0 && (D - 1) * OPS < 64, "form");
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, gq = lane >> 4;
  const int nb = (cnt + 15) >> 4;                             // token blocks in use (wave-uniform)
  const int n0 = blockIdx.x * MOE_WG_ROWS + w * 16 * MOE_NF;  // this wave's first weight row
  const int ks = p.K / p.S, nsteps = ks / MOE_BK;             // a multiple of MOE_UNROLL steps
  const long k0 = (long)blockIdx.z * ks;
  const int* list = p.lists + (long)e * p.R;

  // --- activation gather: token i of the expert is row list[i] / src_div of X -------------------------
  const __amdgpu_buffer_rsrc_t xrs = make_rsrc(p.X, (unsigned)(((long)(p.xrows - 1) * p.ldx + p.K) * 2));
  unsigned xoff[XP];
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int piece = min(w + MOE_NWV * i, 4 * LB - 1), row = 4 * piece + (lane >> 4);
    const int ch = moe_chunk(row, lane & 15);  // (the swizzle is an involution: slot chunk -> source chunk)
    const int pr = min(max(list[min(row, cnt - 1)], 0), p.P - 1);  // tokens past cnt: the last one again (not stored)
    const int srow = min(pr / p.src_div, p.xrows - 1);
    xoff[i] = (unsigned)(((long)srow * p.ldx) * 2 + ch * 16);
  }
  auto issue_x = [&](int t) {
    const int so = __builtin_amdgcn_readfirstlane((int)((k0 + (long)t * MOE_BK) * 2));
    moe_issue_x<XP, LB, TB>(xrs, xoff, smem + (t & (NX - 1)) * XT, so, w);
  };
  // --- weights: row-major, through a descriptor over this expert's [N][K] ------------------------------
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(p.W + (long)e * p.N * p.K, (unsigned)((long)p.N * p.K * 2));
  unsigned woff[MOE_NF];
#pragma unroll
  for (int f = 0; f < MOE_NF; ++f) woff[f] = (unsigned)(((long)(n0 + 16 * f + r) * p.K + k0 + 8 * gq) * 2);
  i32x4 wf[NX][MOE_NF][4];
  auto load_w = [&](int t, i32x4 (&dw)[MOE_NF][4]) {
    moe_load_w<LB, TB>(wrs, woff, __builtin_amdgcn_readfirstlane(t * MOE_BK * 2), dw);
  };

  f32x4 acc[LB][MOE_NF];
#pragma unroll
  for (int tb = 0; tb < LB; ++tb)
#pragma unroll
    for (int f = 0; f < MOE_NF; ++f) acc[tb][f] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue in the order the waits count: X(0) W(0) X(1) W(1) ... for D steps
#pragma unroll
  for (int j = 0; j < D; ++j) {
    issue_x(j);
    __builtin_amdgcn_sched_barrier(0);
    load_w(j, wf[j]);
    __builtin_amdgcn_sched_barrier(0);
  }
  // one K-step on register set J (= t % NX).  ISSUE: it issues the loads of step t + D into the set
  // and slot of step t - 1; WN: the vmcnt that leaves every load of step t landed
  auto step = [&](int t, auto J, auto ISSUE, auto WN) {
    constexpr int j = decltype(J)::value;
    stream::vmcnt<decltype(WN)::value>();
    stream::barrier();  // every wave's X(t); every wave is past step t-1 (its X slot is free)
    if constexpr (decltype(ISSUE)::value) {
      issue_x(t + D);
      __builtin_amdgcn_sched_barrier(0);
      load_w(t + D, wf[(j + D) % NX]);
    }
    __builtin_amdgcn_sched_barrier(0);
    const char* st = smem + (t & (NX - 1)) * XT + r * 256;
#pragma unroll
    for (int tb = 0; tb < LB; ++tb) {
      if (tb < nb) {
        bf16x8 xf[4];
        moe_read_x(st + tb * 4096, r, gq, xf);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int f = 0; f < MOE_NF; ++f) acc[tb][f] = moe_mfma(wf[j][f][kk], xf[kk], acc[tb][f]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  using T = std::true_type;
  using F = std::false_type;
  using WS = std::integral_constant<int, (D - 1) * OPS>;  // steady state
  const int last = nsteps - NX;
  if constexpr (NX == 4) {
    for (int t0 = 0; t0 < last; t0 += 4) {
      step(t0 + 0, std::integral_constant<int, 0>{}, T{}, WS{});
      step(t0 + 1, std::integral_constant<int, 1>{}, T{}, WS{});
      step(t0 + 2, std::integral_constant<int, 2>{}, T{}, WS{});
      step(t0 + 3, std::integral_constant<int, 3>{}, T{}, WS{});
    }
    // the last NX steps: the first still issues (step nsteps - 1), the rest drain
    step(last + 0, std::integral_constant<int, 0>{}, T{}, WS{});
    step(last + 1, std::integral_constant<int, 1>{}, F{}, std::integral_constant<int, 2 * OPS>{});
    step(last + 2, std::integral_constant<int, 2>{}, F{}, std::integral_constant<int, 1 * OPS>{});
    step(last + 3, std::integral_constant<int, 3>{}, F{}, std::integral_constant<int, 0>{});
  } else {
    for (int t0 = 0; t0 < last; t0 += 2) {
      step(t0 + 0, std::integral_constant<int, 0>{}, T{}, WS{});
      step(t0 + 1, std::integral_constant<int, 1>{}, T{}, WS{});
    }
    step(last + 0, std::integral_constant<int, 0>{}, T{}, WS{});
    step(last + 1, std::integral_constant<int, 1>{}, F{}, std::integral_constant<int, 0>{});
  }

  // --- partials: lane holds C[n = 4 gq + e][token r] of each (token block, fragment) -------------------
  float* part = p.part + (long)blockIdx.z * p.P * p.N;
#pragma unroll
  for (int tb = 0; tb < LB; ++tb) {
    const int i = 16 * tb + r;
    if (i >= cnt) continue;
    const int pr = min(max(list[i], 0), p.P - 1);
#pragma unroll
    for (int f = 0; f < MOE_NF; ++f)
      *reinterpret_cast<f32x4*>(part + (long)pr * p.N + n0 + 16 * f + 4 * gq) = acc[tb][f];
  }
}

}  // namespace

// TB: the most 16-token blocks an expert can hold at the launch's row count (R <= 16 TB)
template <int TB>
__global__ __launch_bounds__(64 * MOE_NWV, 1) void moe_gemm_kernel(MoeArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int e = blockIdx.y;
  const int cnt = __builtin_amdgcn_readfirstlane(min(p.counts[e], min(p.R, 16 * TB)));
  if (cnt <= 0) return;  // nobody chose this expert: its weights are not read
  if constexpr (TB >= 16) {
    if (cnt > 128) return moe_body<16, TB>(p, smem, e, cnt);
  }
  if constexpr (TB >= 8) {
    if (cnt > 64) return moe_body<8, TB>(p, smem, e, cnt);
  }
  if constexpr (TB >= 4) {
    if (cnt > 32) return moe_body<4, TB>(p, smem, e, cnt);
  }
  if constexpr (TB >= 2) {
    if (cnt > 16) return moe_body<2, TB>(p, smem, e, cnt);
  }
  moe_body<1, TB>(p, smem, e, cnt);
}

extern "C" int dsa_moe_gemm_form(int R) { return moe_host_form(R); }

extern "C" bool dsa_moe_gemm_supported(int R, int N, int K) {
  // 256 weight rows per workgroup; K slices of 4 whole K-steps; an expert's weight through a 32-bit
  // buffer range
  return R > 0 && R <= MOE_MAXR && N > 0 && N % MOE_WG_ROWS == 0 && K > 0 && K % (MOE_BK * MOE_UNROLL) == 0 &&
         (long)N * K * 2 <= 0xffffffffL;
}

// a K slice the loop can run: whole groups of 4 K-steps
static bool moe_slices(int K, int S) { return S >= 1 && K % (MOE_BK * MOE_UNROLL * S) == 0; }

// K slices: moe_host_split's rule with 256-row tiles and 2 bytes per weight
extern "C" int dsa_moe_gemm_split(int R, int k, int E, int N, int K) {
  if (!dsa_moe_gemm_supported(R, N, K) || k < 1 || k > MOE_MAXK || E < k || E > MOE_MAXE) return 0;
  return moe_host_split(R, k, E, N / MOE_WG_ROWS, K, 2, 1, [K](int s) { return moe_slices(K, s); });
}

template <int TB>
static hipError_t moe_launch(const MoeArgs& a, int E, hipStream_t st) {
  return moe_host_launch<&moe_gemm_kernel<TB>, (TB >= 16 ? 2 : 4) * TB * 4096>(dim3(a.N / MOE_WG_ROWS, E, a.S),
                                                                                64 * MOE_NWV, a, st);
}

// part[s][p][:] = X[p / src_div] W[expert(p)]^T over K slice s, for every pair p in the experts' lists:
// X bf16 [xrows][K] (row stride ldx elements), W bf16 [E][N][K], counts [E], lists [E][R] (moe_route),
// part fp32 [S][R k][N].  Rows of `part` whose pair is in no list are not written.
extern "C" hipError_t dsa_moe_gemm(const void* X, long ldx, int xrows, int src_div, const void* W, const int* counts,
                                   const int* lists, float* part, int R, int k, int E, int N, int K, int S,
                                   hipStream_t st) {
  if (!dsa_moe_gemm_supported(R, N, K) || k < 1 || k > MOE_MAXK || E < k || E > MOE_MAXE) return hipErrorInvalidValue;
  if (!moe_slices(K, S) || part == nullptr || !moe_host_x_ok(ldx, xrows, src_div, R, k, K)) return hipErrorInvalidValue;
  MoeArgs a{(const bf16_t*)X, (const bf16_t*)W, counts, lists, part, ldx, xrows, src_div, R, R * k, N, K, S};
  switch (moe_host_form(R)) {
    case 1: return moe_launch<1>(a, E, st);
    case 2: return moe_launch<2>(a, E, st);
    case 4: return moe_launch<4>(a, E, st);
    case 8: return moe_launch<8>(a, E, st);
    default: return moe_launch<16>(a, E, st);
  }
}

// ================================================================================================
// Router launch
// ================================================================================================
extern "C" hipError_t dsa_moe_lists(const int* topk_e, const int* live, int* counts, int* lists, int R, int k, int E,
                                    hipStream_t st) {
  if (R < 1 || R > MOE_MAXR || k < 1 || k > MOE_MAXK || E < k || E > MOE_MAXE2) return hipErrorInvalidValue;
  moe_lists_kernel<<<E, 64, 0, st>>>(topk_e, live, counts, lists, R, k);
  return hipGetLastError();
}

// h bf16 [R][D] (row stride ldh elements), gate bf16 [E][D]; D % 8 == 0, 16-byte aligned rows
extern "C" hipError_t dsa_moe_route(const void* h, long ldh, const void* gate, const int* live, int* topk_e,
                                    float* topk_w, int* counts, int* lists, int R, int k, int E, int D,
                                    hipStream_t st) {
  if (R < 1 || R > MOE_MAXR || k < 1 || k > MOE_MAXK || E < k || E > MOE_MAXE2 || D < 8 || D % 8 || ldh % 8 || ldh < D)
    return hipErrorInvalidValue;
  if (E <= MOE_MAXE)
    moe_topk_kernel<<<R, 256, 0, st>>>((const bf16_t*)h, ldh, (const bf16_t*)gate, topk_e, topk_w, E, k, D);
  else
    moe_topk2_kernel<<<R, 256, 0, st>>>((const bf16_t*)h, ldh, (const bf16_t*)gate, topk_e, topk_w, E, k, D);
  DSA_CHECK(hipGetLastError());
  return dsa_moe_lists(topk_e, live, counts, lists, R, k, E, st);
}

// ================================================================================================
// Split-K reduces, fused with what follows the GEMM
// ================================================================================================
// (a block per pair or per row, so these two take the prefill GEMM's row counts too: moe_prefill.hip)
// a[p][n] = bf16(silu(g) u), g = sum_s part[s][p][n], u = sum_s part[s][p][F + n] in the order s = 0, 1, ..
// (fp32, one rounding), for the pairs of live rows; 4 columns per thread
__global__ __launch_bounds__(256) void moe_swiglu_kernel(const float* __restrict__ part, const int* __restrict__ live,
                                                         bf16_t* __restrict__ A, int P, int k, int F, int S) {
  const int p = blockIdx.y, n = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (n >= F || live[p / k] <= 0) return;
  const float* src = part + (long)p * 2 * F + n;
  f32x4 g = *reinterpret_cast<const f32x4*>(src), u = *reinterpret_cast<const f32x4*>(src + F);
  for (int s = 1; s < S; ++s) {
    g += *reinterpret_cast<const f32x4*>(src + (long)s * P * 2 * F);
    u += *reinterpret_cast<const f32x4*>(src + (long)s * P * 2 * F + F);
  }
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = moe_silu_mul(g[i], u[i]);
  stream::store_bf16x4(A + (long)p * F + n, o);
}

extern "C" hipError_t dsa_moe_swiglu(const float* part, const int* live, void* A, int R, int k, int F, int S,
                                     hipStream_t st) {
  if (R < 1 || R > MOE_PREFILL_MAXR || k < 1 || k > MOE_MAXK || F < 4 || F % 4 || S < 1) return hipErrorInvalidValue;
  moe_swiglu_kernel<<<dim3((F / 4 + 255) / 256, R * k), 256, 0, st>>>(part, live, (bf16_t*)A, R * k, k, F, S);
  return hipGetLastError();
}

// y[row][n] = bf16(sum_j w[row][j] sum_s part[s][row k + j][n]) in the order j = 0, 1, .. and within it
// s = 0, 1, .. (fp32, one rounding); a row with live <= 0 gets zeros and its partials, which nobody
// wrote, are not read
__global__ __launch_bounds__(256) void moe_combine_kernel(const float* __restrict__ part,
                                                          const float* __restrict__ topk_w,
                                                          const int* __restrict__ live, bf16_t* __restrict__ Y, long ldy,
                                                          int P, int k, int N, int S) {
  const int row = blockIdx.y, n = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (n >= N) return;
  f32x4 y{0.f, 0.f, 0.f, 0.f};
  if (live[row] > 0) {
    for (int j = 0; j < k; ++j) {
      const float* src = part + (long)(row * k + j) * N + n;
      f32x4 d = *reinterpret_cast<const f32x4*>(src);
      for (int s = 1; s < S; ++s) d += *reinterpret_cast<const f32x4*>(src + (long)s * P * N);
      const float wj = topk_w[row * k + j];
#pragma unroll
      for (int i = 0; i < 4; ++i) y[i] = __builtin_fmaf(wj, d[i], y[i]);
    }
  }
  stream::store_bf16x4(Y + (long)row * ldy + n, y);
}

extern "C" hipError_t dsa_moe_combine(const float* part, const float* topk_w, const int* live, void* Y, long ldy, int R,
                                      int k, int N, int S, hipStream_t st) {
  if (R < 1 || R > MOE_PREFILL_MAXR || k < 1 || k > MOE_MAXK || N < 4 || N % 4 || ldy % 4 || ldy < N || S < 1)
    return hipErrorInvalidValue;
  moe_combine_kernel<<<dim3((N / 4 + 255) / 256, R), 256, 0, st>>>(part, topk_w, live, (bf16_t*)Y, ldy, R * k, k, N, S);
  return hipGetLastError();
}
