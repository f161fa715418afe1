// Grouped GEMM of the sparse mixture-of-experts MLP over W4A16 expert weights (AWQ Mixtral checkpoints)
// for the serving engine's decode and verify steps on CDNA4 (gfx950):
//
//   moe_w4_gemm   part[s][p][:] = x[p / src_div] W[expert(p)]^T over K slice s, W[e][n][k] = (q - z) s
//
// moe_gemm's contract (moe.hip) for counts, lists, src_div, live rows and the fp32 partials [S][R k][N],
// so moe_route, moe_swiglu and moe_combine run unchanged around it.  It is moe_gemm and w4_gemm
// (w4.hip) put together -- expert dimension, row gather and dequantizer:
//  * every expert is stored in ops.serving.w4_shuffle's form, the experts stacked: codes uint8
//    [E][N][K/2], zeros uint8 [E][N][K/g] (128 + z), scales fp16 [E][N][K/g].  An expert's bytes are
//    contiguous; each of its three arrays goes through a buffer descriptor of its own, sized to the
//    exact byte count.  One copy; no bf16 copy of an expert exists anywhere;
//  * grid = N tiles of 256 weight rows x experts x K slices; a workgroup whose expert has no pairs
//    leaves before any load.  The host picks the form from the row count R alone (TB = 1, 2, 4, 8, 16
//    token blocks); inside, the workgroup runs the K loop specialized for the smallest LB <= TB that
//    holds its expert's ceil(counts[e] / 16) blocks and skips blocks past the count wave-uniformly
//    (moe_body's scheme);
//  * 8 waves x 2 fragments of 16 weight rows for every LB: the block size is fixed per launch while LB
//    is chosen at run time, so w4_gemm's 4 x 4 split of its small forms does not carry over;
//  * activations, moe_gemm's path: the expert's token rows gathered through lists[e] by LDS-DMA into a
//    ring of 256-byte-row slots, 16-byte chunks XOR-swizzled with the row, NX - 1 K-steps ahead, one
//    bare barrier per K-step;
//  * weights, w4_gemm's path: per lane, fragment and K-step one nontemporal 16-byte load of codes plus
//    the step's scales and zero bytes; (dword >> 4 i) & 0x000F000F | 0x43004300 gives the bf16 values
//    128 + q; X = sum x from one more MFMA against a row of ones per token block and MFMA step;
//    acc += s (P - (128 + z) X) once per group, the fmas unpaired (w4_fold).  g = 32, 64, 128: GS = 4, 2,
//    1 groups per K-step;
//  * ring slots (= weight register sets) NX: 2 where 4 sets do not fit the registers -- 128
//    accumulators (LB 16) or 12 dwords of scales and zeros per fragment and step (g = 32) -- else 4.
//    A K-step goes group by group (a group's codes expanded and its scales and zeros converted once
//    for all token blocks, then every token block's reads, MFMAs and folds of that group), so only one
//    group's operands are live; LB 16 keeps one register set of weights and loads the next step's into
//    it as soon as the step's last group is expanded (see mw4_body);
//  * fp32 partials [S][R k][N] (rows of pairs only), added in a fixed order by moe_swiglu /
//    moe_combine: no atomics, the same inputs give the same bits.
//
// Every index read from memory (counts, lists) is clamped to its range before it addresses anything,
// and every weight and activation load goes through a descriptor sized to its array.  The form ladder,
// the check of x, the rule for the K slices and the launch are moe_gemm's: moe_host.h.
//
// Registers, from the build's metadata (-Rpass-analysis=kernel-resource-usage; 512 threads, so 256
// registers per lane).  A kernel of form TB holds the bodies of every LB <= TB, so its figures cover
// all of them.  VGPRs by TB = 1, 2, 4, 8, 16 -- g = 128: 125, 152, 172, 220, 256; g = 64: 141, 154, 178,
// 226, 256; g = 32: 114, 132, 158, 206, 256.  Private segment (scratch) size: 0 bytes in all fifteen, no
// spill.  (With a step's operands of all groups live at once, and two weight register sets at LB 16,
// the forms TB 16 at every g and TB 8 at g = 64 and 32 spilled 8 to 592 bytes per lane.)
#include <stdint.h>

#include <type_traits>

#include "w4_frag.h"
#include "moe_host.h"

using namespace dsa;
using namespace dsa::w4;
using stream::f32x4;
using stream::i32x4;

namespace {

constexpr int MW4_MAXR = 256;     // token rows
constexpr int MW4_MAXE = 64;      // experts
constexpr int MW4_MAXK = 8;       // experts per token
constexpr int MW4_BK = 128;       // K elements per step
constexpr int MW4_WG_ROWS = 256;  // weight rows per workgroup
constexpr int MW4_NWV = 8;        // waves
constexpr int MW4_NF = 2;         // 16-row weight fragments per wave
constexpr int MW4_UNROLL = 4;     // K-steps per K slice are a multiple of this (both ring sizes divide it)

struct MoeW4Args {
  const bf16_t* X;    // bf16 [xrows][ldx]
  const uint8_t* W;   // stored codes [E][N K / 2]
  const uint8_t* Z;   // stored zeros [E][N K / g]
  const uint8_t* SC;  // stored scales [E][N K / g] fp16
  const int* counts;  // [E]
  const int* lists;   // [E][R]
  float* part;        // [S][P][N] fp32
  long ldx;           // elements
  int xrows, src_div, R, P, N, K, S;
};

// 16-byte chunk of a 256-byte activation row that holds K elements [8 c, 8 c + 8) of token `row`
__device__ __forceinline__ int mw4_chunk(int row, int c) { return c ^ (row & 15); }

// XP 1 KiB activation pieces (4 tokens x 256 B) per wave and step; pieces past the last one are the
// last one again (identical bytes to one slot), so every wave issues the same number of loads
// (TAG: one per kernel instantiation and body -- see the header of stream_frag.h)
template <int XP, int LB, int TAG>
__device__ __forceinline__ void mw4_issue_x(__amdgpu_buffer_rsrc_t xrs, const unsigned (&xoff)[XP], char* slot, int so,
                                            int w) {
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int piece = min(w + MW4_NWV * i, 4 * LB - 1);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, LDS3(void, slot + piece * 1024), 16, xoff[i], so, 0, 0);
  }
}

// a lane's codes of one K-step: per fragment the 16 bytes of its 4 MFMA steps
template <int TAG>
__device__ __forceinline__ void mw4_load_w(__amdgpu_buffer_rsrc_t wrs, const unsigned (&woff)[MW4_NF], int so,
                                           i32x4 (&dst)[MW4_NF]) {
#pragma unroll
  for (int f = 0; f < MW4_NF; ++f) {
    const auto a = __builtin_amdgcn_raw_buffer_load_b128(wrs, (int)woff[f], so, 2);  // 2: nontemporal
    dst[f] = i32x4{(int)a[0], (int)a[1], (int)a[2], (int)a[3]};
  }
}

// the B operand of MFMA step kk of one token block: token r (`row` points at it), K chunk 4 kk + gq
__device__ __forceinline__ bf16x8 mw4_read_x(const char* row, int r, int gq, int kk) {
  return *reinterpret_cast<const bf16x8*>(row + mw4_chunk(r, 4 * kk + gq) * 16);
}

__device__ __forceinline__ f32x4 mw4_mfma(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// ring slots of the body with LB token blocks at GS groups per K-step
constexpr int mw4_slots(int LB, int GS) { return (LB >= 16 || GS == 4) ? 2 : 4; }

// The K loop and the partial store of a workgroup whose expert e has cnt (1 .. 16 LB) pairs, with LB
// token blocks of accumulators; TB, GS: the form of the kernel it is part of.
template <int LB, int TB, int GS>
__device__ __forceinline__ void mw4_body(const MoeW4Args& p, char* smem, const int e, const int cnt) {
  constexpr int NX = mw4_slots(LB, GS);  // ring slots (= weight register sets)
  constexpr int D = NX - 1;              // prefetch distance in K-steps
  constexpr int KG = 4 / GS;             // MFMA steps per group
  constexpr int TAG = (TB * 32 + LB) * 8 + GS;
  constexpr int XR = LB >= 16 ? (KG + 1) / 2 : KG;  // MFMA steps whose B operands are read at once
  constexpr int XT = LB * 4096;                          // one ring slot: 16 LB tokens x 256 B
  constexpr int XP = (4 * LB + MW4_NWV - 1) / MW4_NWV;   // activation pieces per wave per step
  constexpr int OPS = XP + MW4_NF * (GS == 4 ? 4 : 3);   // vector-memory ops per wave per step
  static_assert(LB <= TB && MW4_NWV * MW4_NF * 16 == MW4_WG_ROWS && MW4_UNROLL % NX == 0 && (D - 1) * OPS < 64 &&
                    NX * LB <= mw4_slots(TB, GS) * TB,
                "form");
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, gq = lane >> 4;
  const int nb = (cnt + 15) >> 4;                              // token blocks in use (wave-uniform)
  const int n0 = blockIdx.x * MW4_WG_ROWS + w * 16 * MW4_NF;   // this wave's first weight row
  const int ks = p.K / p.S, nsteps = ks / MW4_BK;              // a multiple of MW4_UNROLL steps
  const long k0 = (long)blockIdx.z * ks;
  const int* list = p.lists + (long)e * p.R;

  // --- activation gather: token i of the expert is row list[i] / src_div of X -------------------------
  const __amdgpu_buffer_rsrc_t xrs = make_rsrc(p.X, (unsigned)(((long)(p.xrows - 1) * p.ldx + p.K) * 2));
  unsigned xoff[XP];
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int piece = min(w + MW4_NWV * i, 4 * LB - 1), row = 4 * piece + (lane >> 4);
    const int ch = mw4_chunk(row, lane & 15);  // (the swizzle is an involution: slot chunk -> source chunk)
    const int pr = min(max(list[min(row, cnt - 1)], 0), p.P - 1);  // tokens past cnt: the last one again (not stored)
    const int srow = min(pr / p.src_div, p.xrows - 1);
    xoff[i] = (unsigned)(((long)srow * p.ldx) * 2 + ch * 16);
  }
  auto issue_x = [&](int t) {
    const int so = __builtin_amdgcn_readfirstlane((int)((k0 + (long)t * MW4_BK) * 2));
    mw4_issue_x<XP, LB, TAG>(xrs, xoff, smem + (t & (NX - 1)) * XT, so, w);
  };
  // --- this expert's weights: per 16-row block and K-step 1 KiB of codes, 32 GS bytes of scales, 16 GS
  // of zeros, each array through a descriptor over the expert's part of it ------------------------------
  const long ksteps = p.K / MW4_BK;
  const long wbytes = (long)p.N * p.K / 2, zbytes = (long)p.N * ksteps * GS;
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(p.W + e * wbytes, (unsigned)wbytes);
  const __amdgpu_buffer_rsrc_t srs = make_rsrc(p.SC + e * zbytes * 2, (unsigned)(zbytes * 2));
  const __amdgpu_buffer_rsrc_t zrs = make_rsrc(p.Z + e * zbytes, (unsigned)zbytes);
  unsigned woff[MW4_NF], soff[MW4_NF], zoff[MW4_NF];
#pragma unroll
  for (int f = 0; f < MW4_NF; ++f) {
    const long at = ((n0 >> 4) + f) * ksteps + k0 / MW4_BK;  // (block, step) index
    woff[f] = (unsigned)(at * 1024 + lane * 16);
    soff[f] = (unsigned)((at * 4 + gq) * (GS * 8));
    zoff[f] = (unsigned)((at * 4 + gq) * (GS * 4));
  }
  // LB 16: one register set of codes, raw scales and zeros beside the 128 accumulators.  A step loads
  // the next step's into the registers of its own as soon as its last group is expanded and converted
  // -- at g = 128 that is the top of the step (NX = 2: every wait is vmcnt(0), so the order of the
  // loads within a step does not matter).  The activations stay a whole step ahead.
  constexpr bool SZ1 = LB >= 16;
  constexpr int NS = SZ1 ? 1 : NX;
  static_assert(!SZ1 || NX == 2, "one scale set needs a prefetch distance of one step");
  i32x4 wf[NS][MW4_NF];
  int sc[NS][MW4_NF][2 * GS], zp[NS][MW4_NF][GS];
  auto load_w = [&](int t, i32x4 (&dw)[MW4_NF]) {
    mw4_load_w<TAG>(wrs, woff, __builtin_amdgcn_readfirstlane(t * 1024), dw);
  };
  auto load_sz = [&](int t, int (&ds)[MW4_NF][2 * GS], int (&dz)[MW4_NF][GS]) {
    w4_load_sz<MW4_NF, TAG, GS>(srs, zrs, soff, zoff, __builtin_amdgcn_readfirstlane(t * 32 * GS),
                                __builtin_amdgcn_readfirstlane(t * 16 * GS), ds, dz);
  };

  f32x4 acc[LB][MW4_NF];
#pragma unroll
  for (int tb = 0; tb < LB; ++tb)
#pragma unroll
    for (int f = 0; f < MW4_NF; ++f) acc[tb][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  const i32x4 ones_i{0x3F803F80, 0x3F803F80, 0x3F803F80, 0x3F803F80};
  const bf16x8 ones = __builtin_bit_cast(bf16x8, ones_i);
  const f32x4 zero4{0.f, 0.f, 0.f, 0.f};
  unsigned kmask = 0x000F000Fu, kbias = 0x43004300u;
  asm volatile("" : "+v"(kmask), "+v"(kbias));  // (see w4_expand)

  // prologue in the order the waits count: X(0) W(0) S(0) Z(0) ... for D steps
#pragma unroll
  for (int j = 0; j < D; ++j) {
    issue_x(j);
    __builtin_amdgcn_sched_barrier(0);
    load_w(j, wf[SZ1 ? 0 : j]);
    load_sz(j, sc[SZ1 ? 0 : j], zp[SZ1 ? 0 : j]);
    __builtin_amdgcn_sched_barrier(0);
  }
  // one K-step on register set J (= t % NX).  ISSUE: it issues the loads of step t + D into the set
  // and slot of step t - 1; WN: the vmcnt that leaves every load of step t landed
  auto step = [&](int t, auto J, auto ISSUE, auto WN) {
    constexpr int j = decltype(J)::value, js = SZ1 ? 0 : j;
    constexpr bool issue = decltype(ISSUE)::value;
    stream::vmcnt<decltype(WN)::value>();
    stream::barrier();  // every wave's X(t); every wave is past step t-1 (its X slot is free)
    if constexpr (issue) {
      issue_x(t + D);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (!SZ1) {
        load_w(t + D, wf[(j + D) % NX]);
        load_sz(t + D, sc[(j + D) % NX], zp[(j + D) % NX]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // Group by group: the group's codes -> bf16 (128 + q), its scales -> fp32 and zero bytes -> 128 + z
    // once for all token blocks, then every token block's reads, MFMAs and folds of the group.  Only
    // one group's operands are live at a time (at g = 32 a step's converted scales and zeros would
    // take 64 registers beside the 128 accumulators of 16 token blocks); the scheduling barriers keep
    // a token block's work together.  Blocks past the expert's count are skipped by every wave alike.
    const char* st = smem + (t & (NX - 1)) * XT + r * 256;
#pragma unroll
    for (int G = 0; G < GS; ++G) {
      bf16x8 a[KG][MW4_NF];
      float s[MW4_NF][4], zn[MW4_NF][4];
#pragma unroll
      for (int f = 0; f < MW4_NF; ++f) {
#pragma unroll
        for (int q = 0; q < KG; ++q) a[q][f] = w4_expand(wf[js][f][G * KG + q], kmask, kbias);
        w4_convert<GS>(sc[js][f], zp[js][f], G, s[f], zn[f]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (SZ1 && issue) {
        if (G == GS - 1) load_w(t + D, wf[0]), load_sz(t + D, sc[0], zp[0]);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int tb = 0; tb < LB; ++tb) {
        if (tb < nb) {
          f32x4 P[MW4_NF], PX = zero4;
#pragma unroll
          for (int f = 0; f < MW4_NF; ++f) P[f] = zero4;
#pragma unroll
          for (int q0 = 0; q0 < KG; q0 += XR) {
            bf16x8 x[XR];
#pragma unroll
            for (int q = 0; q < XR; ++q) x[q] = mw4_read_x(st + tb * 4096, r, gq, G * KG + q0 + q);
#pragma unroll
            for (int q = 0; q < XR; ++q) {
              PX = mw4_mfma(ones, x[q], PX);
#pragma unroll
              for (int f = 0; f < MW4_NF; ++f) P[f] = mw4_mfma(a[q0 + q][f], x[q], P[f]);
            }
          }
#pragma unroll
          for (int f = 0; f < MW4_NF; ++f) {
            w4_fold(acc[tb][f], P[f], PX[0], s[f], zn[f]);
            // (pins the fold here: otherwise the compiler sinks the folds and keeps every P alive)
            asm volatile("" : "+v"(acc[tb][f]));
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
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
    for (int f = 0; f < MW4_NF; ++f)
      *reinterpret_cast<f32x4*>(part + (long)pr * p.N + n0 + 16 * f + 4 * gq) = acc[tb][f];
  }
}

}  // namespace

// TB: the most 16-token blocks an expert can hold at the launch's row count (R <= 16 TB); GS groups per
// 128-wide K-step (g = 128 / GS)
template <int TB, int GS>
__global__ __launch_bounds__(64 * MW4_NWV, 1) void moe_w4_gemm_kernel(MoeW4Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int e = blockIdx.y;
  const int cnt = __builtin_amdgcn_readfirstlane(min(p.counts[e], min(p.R, 16 * TB)));
  if (cnt <= 0) return;  // nobody chose this expert: its weights are not read
  if constexpr (TB >= 16) {
    if (cnt > 128) return mw4_body<16, TB, GS>(p, smem, e, cnt);
  }
  if constexpr (TB >= 8) {
    if (cnt > 64) return mw4_body<8, TB, GS>(p, smem, e, cnt);
  }
  if constexpr (TB >= 4) {
    if (cnt > 32) return mw4_body<4, TB, GS>(p, smem, e, cnt);
  }
  if constexpr (TB >= 2) {
    if (cnt > 16) return mw4_body<2, TB, GS>(p, smem, e, cnt);
  }
  mw4_body<1, TB, GS>(p, smem, e, cnt);
}

extern "C" int dsa_moe_w4_gemm_form(int R) { return moe_host_form(R); }

extern "C" bool dsa_moe_w4_gemm_supported(int R, int N, int K, int g) {
  // 256 weight rows per workgroup; K slices of 4 whole K-steps; an expert's codes through a 32-bit
  // buffer range
  return R > 0 && R <= MW4_MAXR && N > 0 && N % MW4_WG_ROWS == 0 && K > 0 && K % (MW4_BK * MW4_UNROLL) == 0 &&
         (g == 32 || g == 64 || g == 128) && (long)N * K / 2 <= 0xffffffffL;
}

// a K slice the loop can run: whole groups of 4 K-steps
static bool mw4_slices(int K, int S) { return S >= 1 && K % (MW4_BK * MW4_UNROLL * S) == 0; }

// K slices: moe_host_split's rule with 256-row tiles and the weight bytes of W4 at g = 128, 0.52 = 13 / 25
// per weight
extern "C" int dsa_moe_w4_gemm_split(int R, int k, int E, int N, int K) {
  if (!dsa_moe_w4_gemm_supported(R, N, K, 128) || k < 1 || k > MW4_MAXK || E < k || E > MW4_MAXE) return 0;
  return moe_host_split(R, k, E, N / MW4_WG_ROWS, K, 13, 25, [K](int s) { return mw4_slices(K, s); });
}

namespace {
template <int TB, int GS>
hipError_t mw4_launch(const MoeW4Args& a, int E, hipStream_t st) {
  return moe_host_launch<&moe_w4_gemm_kernel<TB, GS>, mw4_slots(TB, GS) * TB * 4096>(dim3(a.N / MW4_WG_ROWS, E, a.S),
                                                                                      64 * MW4_NWV, a, st);
}

template <int GS>
hipError_t mw4_launch_form(const MoeW4Args& a, int E, hipStream_t st) {
  switch (moe_host_form(a.R)) {
    case 1: return mw4_launch<1, GS>(a, E, st);
    case 2: return mw4_launch<2, GS>(a, E, st);
    case 4: return mw4_launch<4, GS>(a, E, st);
    case 8: return mw4_launch<8, GS>(a, E, st);
    default: return mw4_launch<16, GS>(a, E, st);
  }
}
}  // namespace

// part[s][p][:] = X[p / src_div] W[expert(p)]^T over K slice s, for every pair p in the experts' lists:
// X bf16 [xrows][K] (row stride ldx elements); W, Z, SC the experts' stored W4 weights [E][N][K] (codes
// E N K / 2 bytes, zeros E N K / g bytes, scales E N K / g fp16: ops.serving.w4_shuffle per expert);
// counts [E], lists [E][R] (moe_route), part fp32 [S][R k][N].  Rows of `part` whose pair is in no list
// are not written.
extern "C" hipError_t dsa_moe_w4_gemm(const void* X, long ldx, int xrows, int src_div, const void* W, const void* Z,
                                      const void* SC, const int* counts, const int* lists, float* part, int R, int k,
                                      int E, int N, int K, int g, int S, hipStream_t st) {
  if (!dsa_moe_w4_gemm_supported(R, N, K, g) || k < 1 || k > MW4_MAXK || E < k || E > MW4_MAXE)
    return hipErrorInvalidValue;
  if (!mw4_slices(K, S) || part == nullptr || !moe_host_x_ok(ldx, xrows, src_div, R, k, K)) return hipErrorInvalidValue;
  MoeW4Args a{(const bf16_t*)X, (const uint8_t*)W, (const uint8_t*)Z, (const uint8_t*)SC, counts, lists, part, ldx,
              xrows, src_div, R, R * k, N, K, S};
  return g == 128 ? mw4_launch_form<1>(a, E, st) : g == 64 ? mw4_launch_form<2>(a, E, st) : mw4_launch_form<4>(a, E, st);
}
