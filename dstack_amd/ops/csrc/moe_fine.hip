// Routed expert GEMM for fine-grained mixtures of experts (Qwen3-MoE: 128 experts of F = 768 or 1536,
// 8 per token) on CDNA4 (gfx950): moe_gemm's contract (moe.hip) with the work split for many small
// experts.
//
//   part[s][p][:] = x[p / src_div] W[expert(p)]^T over K slice s, for the pairs of each expert
//
// W bf16 row-major [E][N][K] (the one copy every path reads), pairs from counts / lists (moe_route),
// fp32 partials [S][R k][N] added in a fixed order by moe_swiglu / moe_combine: no atomics, the same
// inputs give the same bits.  Every index read from memory (counts, lists) is clamped to its range
// before it addresses anything.  The grid depends on the shapes only, so the launch sits in a captured
// graph.
//
// With 128 experts a step of 256 rows leaves an expert about 16 pairs and a K loop of 6 .. 32 steps, so
// what counts is how many workgroups are in flight and how soon each reaches its loop, not how many
// tokens one workgroup can hold:
//  * a workgroup owns 128 weight rows of one expert: 4 waves x 2 fragments of 16 rows, 256 threads.  The
//    weights are the A operand of v_mfma_f32_16x16x32_bf16 straight from HBM, one nontemporal 16-byte
//    buffer load per lane and MFMA step, three K-steps ahead of their MFMAs (moe_frag.h: moe_load_w);
//  * grid = N / 128 tiles x E experts x K slices; a workgroup whose expert has no pairs returns at once;
//  * the expert's token rows are gathered through lists[e] by LDS-DMA into a ring of four slots of
//    256-byte rows with moe_gemm's swizzle, consumed as blocks of 16 tokens, one bare barrier per K-step;
//  * accumulators for at most 4 token blocks.  The K loop is instantiated for 1, 2 and 4 blocks and the
//    one that holds the pass's pairs is taken wave-uniformly from counts[e]; there is no form picked by
//    the row count on the host.  An expert with more than 64 pairs runs ceil(cnt / 64) passes over its
//    tile, re-reading its (at most 1 MB of) weights, so skewed routing stays correct up to cnt = R = 256
//    while every workgroup is sized for the common case: 64 KB of LDS (4 slots x 64 tokens x 256 B) and
//    __launch_bounds__(256, 2), two workgroups per CU, one's prologue beside the other's K loop;
//  * a K slice is any even number >= 4 of 128-element steps: the ring's body is unrolled by four, the
//    last steps drain, and a slice of 4 m + 2 steps ends in a six-step tail instead of a four-step one
//    (an instantiation of its own, picked from K and the slices).
//
// Chosen: 128-row tiles (Qwen3-30B-A3B's down projection has N = 2048: 16 tiles x 8 chosen experts is
// 128 workgroups for one token, half the CUs; 256-row tiles would halve that again), a ring four deep
// for every form (6-step loops spend half their time in prologue and drain at any depth; 4 keeps three
// loads in flight per lane and fragment), K slices by moe_gemm's rule (moe_host.h) with this kernel's tile
// and step constraints (dsa_moe_fine_gemm_split).  Not tried: 64-row tiles, 2 waves x 4 fragments, 8-block
// passes with one workgroup per CU, a narrower tile at row counts where few experts are hit, keeping a
// multi-pass expert's weights in registers or LDS instead of re-reading them.
#include <stdint.h>

#include <type_traits>

#include "moe_frag.h"
#include "moe_host.h"

using namespace dsa;
using namespace dsa::moe;

namespace {

constexpr int FINE_MAXE = 128;     // experts
constexpr int FINE_WG_ROWS = 128;  // weight rows per workgroup
constexpr int FINE_NWV = 4;        // waves
constexpr int FINE_NX = 4;         // ring slots (= weight register sets)
constexpr int FINE_MAXB = 4;       // token blocks of a pass
constexpr int FINE_LDS = FINE_NX * FINE_MAXB * 4096;

// LB 1 KiB activation pieces (4 tokens x 256 B) per wave and step: piece w + 4 i of the slot's 4 LB
// (TAG: a tag per kernel instantiation -- see the header of stream_frag.h)
template <int LB, int TAG>
__device__ __forceinline__ void fine_issue_x(__amdgpu_buffer_rsrc_t xrs, const unsigned (&xoff)[LB], char* slot, int so,
                                             int w) {
#pragma unroll
  for (int i = 0; i < LB; ++i)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, LDS3(void, slot + (w + FINE_NWV * i) * 1024), 16, xoff[i], so, 0, 0);
}

// One pass: the K loop and the partial store for pairs list[0 .. cnt) of the workgroup's expert (1 <= cnt
// <= 16 LB; `list` points at the pass's first pair), with LB token blocks of accumulators.  SIX: a K slice
// is 4 m + 2 steps.
template <int LB, bool SIX>
__device__ __forceinline__ void fine_body(const MoeArgs& p, char* smem, const int e, const int* list, const int cnt) {
  constexpr int NX = FINE_NX, D = NX - 1;  // prefetch distance in K-steps
  constexpr int XT = LB * 4096;            // one ring slot: 16 LB tokens x 256 B
  constexpr int OPS = LB + 4 * MOE_NF;     // vector-memory ops per wave per step
  constexpr int TAG = SIX ? 6 : 4;         // of the helpers' instantiations: the steps of the kernel's tail
  static_assert(LB <= FINE_MAXB && FINE_NWV * MOE_NF * 16 == FINE_WG_ROWS && (D - 1) * OPS < 64, "form");
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, gq = lane >> 4;
  const int nb = (cnt + 15) >> 4;                              // token blocks in use (wave-uniform)
  const int n0 = blockIdx.x * FINE_WG_ROWS + w * 16 * MOE_NF;  // this wave's first weight row
  const int ks = p.K / p.S, nsteps = ks / MOE_BK;              // even, >= 4
  const long k0 = (long)blockIdx.z * ks;

  // --- activation gather: token i of the pass is row list[i] / src_div of X ----------------------------
  const __amdgpu_buffer_rsrc_t xrs = make_rsrc(p.X, (unsigned)(((long)(p.xrows - 1) * p.ldx + p.K) * 2));
  unsigned xoff[LB];
#pragma unroll
  for (int i = 0; i < LB; ++i) {
    const int row = 4 * (w + FINE_NWV * i) + (lane >> 4);
    const int ch = moe_chunk(row, lane & 15);  // (the swizzle is an involution: slot chunk -> source chunk)
    const int pr = min(max(list[min(row, cnt - 1)], 0), p.P - 1);  // tokens past cnt: the last one again (not stored)
    const int srow = min(pr / p.src_div, p.xrows - 1);
    xoff[i] = (unsigned)(((long)srow * p.ldx) * 2 + ch * 16);
  }
  auto issue_x = [&](int t) {
    const int so = __builtin_amdgcn_readfirstlane((int)((k0 + (long)t * MOE_BK) * 2));
    fine_issue_x<LB, TAG>(xrs, xoff, smem + (t & (NX - 1)) * XT, so, w);
  };
  // --- weights: row-major, through a descriptor over this expert's [N][K] ------------------------------
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(p.W + (long)e * p.N * p.K, (unsigned)((long)p.N * p.K * 2));
  unsigned woff[MOE_NF];
#pragma unroll
  for (int f = 0; f < MOE_NF; ++f) woff[f] = (unsigned)(((long)(n0 + 16 * f + r) * p.K + k0 + 8 * gq) * 2);
  i32x4 wf[NX][MOE_NF][4];
  auto load_w = [&](int t, i32x4 (&dw)[MOE_NF][4]) {
    moe_load_w<LB, TAG>(wrs, woff, __builtin_amdgcn_readfirstlane(t * MOE_BK * 2), dw);
  };

  f32x4 acc[LB][MOE_NF];
#pragma unroll
  for (int tb = 0; tb < LB; ++tb)
#pragma unroll
    for (int f = 0; f < MOE_NF; ++f) acc[tb][f] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue in the order the waits count: X(0) W(0) X(1) W(1) X(2) W(2)
#pragma unroll
  for (int j = 0; j < D; ++j) {
    issue_x(j);
    __builtin_amdgcn_sched_barrier(0);
    load_w(j, wf[j]);
    __builtin_amdgcn_sched_barrier(0);
  }
  // one K-step on register set J (= t % 4).  ISSUE: it issues the loads of step t + 3 into the set and
  // slot of step t - 1; WN: the vmcnt that leaves every load of step t landed
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
  using J0 = std::integral_constant<int, 0>;
  using J1 = std::integral_constant<int, 1>;
  using J2 = std::integral_constant<int, 2>;
  using J3 = std::integral_constant<int, 3>;
  using WS = std::integral_constant<int, (D - 1) * OPS>;  // steady state
  using W1 = std::integral_constant<int, OPS>;
  using W0 = std::integral_constant<int, 0>;
  // steps 0 .. nsteps - 4 issue, the last three drain; `tail` is the first step outside the whole groups
  // of four issuing steps: nsteps - 4 (four steps left) or, SIX, nsteps - 6 (six left, nsteps = 4 m + 2)
  const int tail = nsteps - (SIX ? 6 : 4);
  for (int t0 = 0; t0 < tail; t0 += 4) {
    step(t0 + 0, J0{}, T{}, WS{});
    step(t0 + 1, J1{}, T{}, WS{});
    step(t0 + 2, J2{}, T{}, WS{});
    step(t0 + 3, J3{}, T{}, WS{});
  }
  if constexpr (SIX) {
    step(tail + 0, J0{}, T{}, WS{});
    step(tail + 1, J1{}, T{}, WS{});
    step(tail + 2, J2{}, T{}, WS{});
    step(tail + 3, J3{}, F{}, WS{});
    step(tail + 4, J0{}, F{}, W1{});
    step(tail + 5, J1{}, F{}, W0{});
  } else {
    step(tail + 0, J0{}, T{}, WS{});
    step(tail + 1, J1{}, F{}, WS{});
    step(tail + 2, J2{}, F{}, W1{});
    step(tail + 3, J3{}, F{}, W0{});
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

// SIX: a K slice is 4 m + 2 steps (a shape's property, so the host instantiates it: with the two tails behind
// a branch in one kernel the register allocator spilled, 76 .. 344 bytes of scratch in every arrangement
// tried; apart, the kernels take 230 and 234 VGPRs and no scratch)
template <bool SIX>
__global__ __launch_bounds__(64 * FINE_NWV, 2) void moe_fine_gemm_kernel(MoeArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int e = blockIdx.y;
  const int cnt = __builtin_amdgcn_readfirstlane(min(p.counts[e], p.R));
  if (cnt <= 0) return;  // nobody chose this expert: its weights are not read
  const int* list = p.lists + (long)e * p.R;
  for (int base = 0; base < cnt; base += 16 * FINE_MAXB) {
    const int c = min(cnt - base, 16 * FINE_MAXB);
    if (base) {  // every wave has read the previous pass's last slots; its stores leave the wait counts
      stream::vmcnt<0>();
      stream::barrier();
    }
    if (c > 32)
      fine_body<4, SIX>(p, smem, e, list + base, c);
    else if (c > 16)
      fine_body<2, SIX>(p, smem, e, list + base, c);
    else
      fine_body<1, SIX>(p, smem, e, list + base, c);
  }
}

extern "C" bool dsa_moe_fine_gemm_supported(int R, int N, int K) {
  // 128 weight rows per workgroup; an even number >= 4 of K-steps; an expert's weight through a 32-bit
  // buffer range
  return R > 0 && R <= MOE_MAXR && N > 0 && N % FINE_WG_ROWS == 0 && K >= 4 * MOE_BK && K % (2 * MOE_BK) == 0 &&
         (long)N * K * 2 <= 0xffffffffL;
}

// a K slice the loop can run: an even number >= 4 of whole steps
static bool fine_slices(int K, int S) { return S >= 1 && K % S == 0 && (K / S) % (2 * MOE_BK) == 0 && K / S >= 4 * MOE_BK; }

// K slices: moe_host_split's rule with 128-row tiles and 2 bytes per weight
extern "C" int dsa_moe_fine_gemm_split(int R, int k, int E, int N, int K) {
  if (!dsa_moe_fine_gemm_supported(R, N, K) || k < 1 || k > MOE_MAXK || E < k || E > FINE_MAXE) return 0;
  return moe_host_split(R, k, E, N / FINE_WG_ROWS, K, 2, 1, [K](int s) { return fine_slices(K, s); });
}

template <bool SIX>
static hipError_t fine_launch(const MoeArgs& a, int E, hipStream_t st) {
  return moe_host_launch<&moe_fine_gemm_kernel<SIX>, FINE_LDS>(dim3(a.N / FINE_WG_ROWS, E, a.S), 64 * FINE_NWV, a, st);
}

// part[s][p][:] = X[p / src_div] W[expert(p)]^T over K slice s, for every pair p in the experts' lists:
// X bf16 [xrows][K] (row stride ldx elements), W bf16 [E][N][K], counts [E], lists [E][R] (moe_route),
// part fp32 [S][R k][N].  Rows of `part` whose pair is in no list are not written.
extern "C" hipError_t dsa_moe_fine_gemm(const void* X, long ldx, int xrows, int src_div, const void* W, const int* counts,
                                        const int* lists, float* part, int R, int k, int E, int N, int K, int S,
                                        hipStream_t st) {
  if (!dsa_moe_fine_gemm_supported(R, N, K) || k < 1 || k > MOE_MAXK || E < k || E > FINE_MAXE) return hipErrorInvalidValue;
  if (!fine_slices(K, S) || part == nullptr || !moe_host_x_ok(ldx, xrows, src_div, R, k, K)) return hipErrorInvalidValue;
  MoeArgs a{(const bf16_t*)X, (const bf16_t*)W, counts, lists, part, ldx, xrows, src_div, R, R * k, N, K, S};
  return (K / S / MOE_BK) & 2 ? fine_launch<true>(a, E, st) : fine_launch<false>(a, E, st);
}
