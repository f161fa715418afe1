// W4A16 weights (AWQ checkpoints: unsigned 4-bit codes q, per group of g = 32 / 64 / 128 elements along K
// and output row an fp16 scale s and a 4-bit zero point z; W[n][k] = (q - z) s) for the serving engine
// on CDNA4 (gfx950): the decode GEMM on bf16 activations and the exact dequantizer.
//
// Decode GEMM: Y[m][n] = bf16( sum_k X[m][k] (q[n][k] - z[n][k/g]) s[n][k/g] ), fp32 accumulation, one
// rounding, for 1 <= M <= 256 token rows.  gfx950 has no int4 MFMA: the codes stream from HBM, become
// bf16 in registers and feed v_mfma_f32_16x16x32_bf16.  The structure is mxfp4_gemm's (mxfp4.hip):
//  * the weights are the A operand: lane (r = lane & 15, gq = lane >> 4) holds weight row r, K elements
//    [8 gq, 8 gq + 8) of a 32-wide MFMA step, the activations the B operand (token row r, the same K);
//    a lane's accumulator holds output columns n = 4 gq + e (e = 0..3) of token row r;
//  * a K-step is 128 elements = four MFMA steps kk.  The stored weight (ops.serving.w4_shuffle) is in
//    lane order: per 16-row block and K-step the 1 KiB of the 64 lanes' 16 bytes, dword kk of a lane its
//    8 codes of MFMA step kk; per block, step and lane group gq the step's 128 / g groups of 4 fp16
//    scales (rows 4 gq + e) and of 4 zero bytes (128 + z: what the kernel subtracts).  Every weight load is one contiguous, nontemporal
//    16-byte-per-lane buffer load through a descriptor sized to the exact byte count;
//  * the bf16 activations (L2-resident) are LDS-DMA'd into a ring of 256-byte-row slots (16-byte chunks
//    XOR-swizzled with the row: w4_chunk), D = NX - 1 K-steps ahead, one bare barrier per step;
//  * K is split over gridDim.y with fp32 partials [S][M][N] that stream::reduce_kernel adds in a fixed
//    order (no atomics: the same inputs give the same bits).
//
// The dequantize budget.  At 0.52 bytes per weight, HBM rate is about 45 G weights/s per CU, which
// leaves about 3.4 vector lane-ops per weight beside the MFMAs.  Designed for: 0.875 per weight in the
// 1-token-block form, plus a per-group part that shrinks with g:
//  * the nibble order of a stored dword is K elements (0, 2, 4, 6, 1, 3, 5, 7): (dword >> 4 i) & 0x000F000F
//    | 0x43004300 is the bf16 pair (128 + q[2i], 128 + q[2i+1]) -- one MFMA operand register from one
//    shift and one v_and_or_b32 (the first needs no shift): 7 instructions per 8 weights, exact
//    (128 + q <= 143 has 8 significant bits);
//  * the zero point and the scale are applied to the accumulator, once per group, token block and
//    16-row fragment: acc += s (P - (128 + z) X), with P the MFMA sum of x (128 + q) over the group and
//    X the sum of x over the group.  X comes from one more MFMA per token block and MFMA step whose A
//    operand is all ones (every accumulator register of its result is X of the lane's token row), so
//    no lane exchanges.  Per lane, group, fragment and token block that is 2 fma per accumulator
//    register = 8 instructions for 8 g / 16 weights: 16 / g per weight (0.125 at g = 128), plus the 8
//    conversions of 4 scales and 4 zero bytes per fragment and group, shared by the token blocks.
//  Counted in the disassembly of the 1-token-block form at g = 128, per K-step and wave (128 weights
//  per lane, 20 MFMAs): 64 v_and_or_b32 + 48 v_lshrrev_b32 (0.875 per weight), 32 fma, 32 conversions, 16
//  v_xor_b32 of the activation addresses: 1.5 per weight.  Left to itself the compiler pairs the fmas
//  into v_pk_fma_f32, which costs issue cycles beside MFMAs (packed f32 beside MFMAs: about 22 cycles
//  per instruction more than the two v_fma_f32); w4_fold keeps them apart.
//  The cancellation P - (128 + z) X is done in one fma, so only P's own fp32 accumulation error (on
//  terms 128 + q instead of q - z) is amplified: about 30x an fp32 accumulation's error, 2e-6 relative.
//
// Forms, by 16-row token blocks TB (a 1-row batch must not run 16 blocks of MFMAs):
//    TB 16 (M <= 256) and TB 8 (M <= 128): 8 waves x 2 fragments;
//    TB 4  (M <= 64)  and TB 1 (M <= 16):  4 waves x 4 fragments.
// All cover 256 weight rows per workgroup.  Ring: 4 slots of TB x 4 KiB (TB 16: 2 slots of 64 KiB, one
// step ahead: at 256 rows the MFMAs, not the loads, take the time).
#include <stdint.h>

#include <type_traits>

#include "stream_frag.h"

using namespace dsa;
using stream::f32x4;
using stream::i32x4;

namespace {

constexpr int W4_MAXM = 256;     // token rows
constexpr int W4_BK = 128;       // K elements per step
constexpr int W4_WG_ROWS = 256;  // weight rows per workgroup, every form
constexpr int W4_UNROLL = 4;     // K-steps per K slice are a multiple of this (both ring sizes divide it)

struct W4Args {
  const bf16_t* X;    // bf16 [M][ldx]
  const uint8_t* W;   // stored codes, N * K / 2 bytes
  const uint8_t* Z;   // stored zeros, N * K / g bytes
  const uint8_t* SC;  // stored scales, N * K / g fp16
  bf16_t* Y;
  float* part;        // [S][M][N] fp32 (S > 1)
  long ldx, ldy;      // elements
  int M, N, K, S;
};

// 16-byte chunk of a 256-byte activation row that holds K elements [8 c, 8 c + 8) of token row `row`:
// the 16 lanes of a ds_read_b128 lane group read one chunk column of 16 rows, and the XOR spreads them
// over the 16 bank windows of 16 bytes
__device__ __forceinline__ int w4_chunk(int row, int c) { return c ^ (row & 15); }

// XP 1 KiB activation pieces (4 token rows x 256 B) per wave and step; pieces past the last one are
// the last one again (identical bytes to one slot), so every wave issues the same number of loads
// (GS, TB below: a tag per kernel instantiation -- see the header of stream_frag.h)
template <int XP, int NWV, int TB, int GS>
__device__ __forceinline__ void w4_issue_x(__amdgpu_buffer_rsrc_t xrs, const unsigned (&xoff)[XP], char* slot, int so,
                                           int w) {
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int piece = min(w + NWV * i, 4 * TB - 1);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, LDS3(void, slot + piece * 1024), 16, xoff[i], so, 0, 0);
  }
}

template <int NF, int TB, int GS>
__device__ __forceinline__ void w4_load_w(__amdgpu_buffer_rsrc_t wrs, const unsigned (&woff)[NF], int so,
                                          i32x4 (&dst)[NF]) {
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const auto a = __builtin_amdgcn_raw_buffer_load_b128(wrs, (int)woff[f], so, 2);  // 2: nontemporal
    dst[f] = i32x4{(int)a[0], (int)a[1], (int)a[2], (int)a[3]};
  }
}

// a lane's scales (GS groups x 4 fp16 = 2 GS dwords) and zeros (GS groups x 4 bytes = GS dwords) of one step
template <int NF, int TB, int GS>
__device__ __forceinline__ void w4_load_sz(__amdgpu_buffer_rsrc_t srs, __amdgpu_buffer_rsrc_t zrs,
                                           const unsigned (&soff)[NF], const unsigned (&zoff)[NF], int sso, int zso,
                                           int (&sc)[NF][2 * GS], int (&zp)[NF][GS]) {
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    if constexpr (GS == 1) {
      const auto a = __builtin_amdgcn_raw_buffer_load_b64(srs, (int)soff[f], sso, 0);
      sc[f][0] = (int)a[0], sc[f][1] = (int)a[1];
      zp[f][0] = (int)__builtin_amdgcn_raw_buffer_load_b32(zrs, (int)zoff[f], zso, 0);
    } else if constexpr (GS == 2) {
      const auto a = __builtin_amdgcn_raw_buffer_load_b128(srs, (int)soff[f], sso, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) sc[f][i] = (int)a[i];
      const auto b = __builtin_amdgcn_raw_buffer_load_b64(zrs, (int)zoff[f], zso, 0);
      zp[f][0] = (int)b[0], zp[f][1] = (int)b[1];
    } else {
      const auto a = __builtin_amdgcn_raw_buffer_load_b128(srs, (int)soff[f], sso, 0);
      const auto a2 = __builtin_amdgcn_raw_buffer_load_b128(srs, (int)soff[f] + 16, sso, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) sc[f][i] = (int)a[i], sc[f][4 + i] = (int)a2[i];
      const auto b = __builtin_amdgcn_raw_buffer_load_b128(zrs, (int)zoff[f], zso, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) zp[f][i] = (int)b[i];
    }
  }
}

// the 8 codes of one stored dword as the bf16 values 128 + q, in MFMA operand order.  mask = 0x000F000F
// and bias = 0x43004300 come in registers (w4_gemm_kernel hides their values from the compiler): as
// literals the compiler emits v_and_b32 + v_or_b32, the VOP3 v_and_or_b32 taking no literal
__device__ __forceinline__ bf16x8 w4_expand(int d, unsigned mask, unsigned bias) {
  const unsigned u = (unsigned)d;
  const i32x4 v{(int)((u & mask) | bias), (int)(((u >> 4) & mask) | bias), (int)(((u >> 8) & mask) | bias),
                (int)(((u >> 12) & mask) | bias)};
  return __builtin_bit_cast(bf16x8, v);
}

// the 4 MFMA steps' B operands of one token block: token row r (st points at it), K chunks 4 kk + gq
__device__ __forceinline__ void w4_read_x(const char* row, int r, int gq, bf16x8 (&xf)[4]) {
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) xf[kk] = *reinterpret_cast<const bf16x8*>(row + w4_chunk(r, 4 * kk + gq) * 16);
}

__device__ __forceinline__ float w4_half(unsigned bits) {
  return (float)__builtin_bit_cast(_Float16, (unsigned short)bits);
}

// group G of a lane's raw scales and zeros of one step and fragment: s[e] fp32, zn[e] = 128 + z[e] (8
// conversions: v_cvt_f32_f16 and v_cvt_f32_ubyte0..3 pick their half / byte themselves)
template <int GS>
__device__ __forceinline__ void w4_convert(const int (&sc)[2 * GS], const int (&zp)[GS], int G, float (&s)[4],
                                           float (&zn)[4]) {
  const unsigned s01 = (unsigned)sc[2 * G], s23 = (unsigned)sc[2 * G + 1], zb = (unsigned)zp[G];
  s[0] = w4_half(s01 & 0xffffu), s[1] = w4_half(s01 >> 16);
  s[2] = w4_half(s23 & 0xffffu), s[3] = w4_half(s23 >> 16);
#pragma unroll
  for (int e = 0; e < 4; ++e) zn[e] = (float)((zb >> (8 * e)) & 0xffu);  // (the stored byte is 128 + z)
}

__device__ __forceinline__ f32x4 w4_mfma(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// acc += s (P - zn X) for the 4 accumulator registers of one fragment (zn = 128 + z), as 8 v_fma_f32
__device__ __forceinline__ void w4_fold(f32x4& acc, const f32x4& P, float X, const float (&s)[4], const float (&zn)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float d = __builtin_fmaf(-zn[e], X, P[e]);
    asm("" : "+v"(d));  // (an opaque value: the compiler cannot pair it with its neighbour into v_pk_fma_f32)
    float a = __builtin_fmaf(s[e], d, acc[e]);
    asm("" : "+v"(a));
    acc[e] = a;
  }
}

}  // namespace

// TB 16-row token blocks, NWV waves x NF 16-row weight fragments per wave (NWV * NF == 16), GS groups
// per 128-wide K-step (g = 128 / GS)
template <int TB, int NWV, int NF, int GS>
__global__ __launch_bounds__(64 * NWV, TB == 1 ? 2 : 1) void w4_gemm_kernel(W4Args p) {
  // ring slots (= weight register sets): 2 where 4 sets do not fit the registers -- 128 accumulators
  // (TB 16), or 12 dwords of scales and zeros per fragment and step (g = 32)
  constexpr int NX = (TB >= 16 || GS == 4) ? 2 : 4;
  constexpr int D = NX - 1;             // prefetch distance in K-steps
  constexpr int KG = 4 / GS;            // MFMA steps per group
  constexpr int LA = (TB > 1 && TB < 16 && (GS == 1 || NWV == 4)) ? 1 : 0;  // look-ahead of the LDS reads, token blocks
  // codes expanded and scales / zeros converted once per step for all token blocks; with one token
  // block at their use instead, which keeps them out of registers
  constexpr bool EAGER = TB > 1;
  constexpr int XT = TB * 4096;         // one ring slot: 16 TB token rows x 256 B
  constexpr int XP = (4 * TB + NWV - 1) / NWV;          // activation pieces per wave per step
  constexpr int OPS = XP + NF * (2 + (GS == 4 ? 2 : 1));  // vector-memory ops per wave per step
  static_assert(NWV * NF * 16 == W4_WG_ROWS && W4_UNROLL % NX == 0 && (D - 1) * OPS < 64, "form");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, gq = lane >> 4;
  const int n0 = (blockIdx.x * NWV + w) * 16 * NF;  // this wave's first weight row
  const int ks = p.K / p.S, nsteps = ks / W4_BK;    // a multiple of W4_UNROLL steps
  const long k0 = (long)blockIdx.y * ks;

  // --- activation DMA ---------------------------------------------------------------------------
  const __amdgpu_buffer_rsrc_t xrs = make_rsrc(p.X, (unsigned)(((long)(p.M - 1) * p.ldx + p.K) * 2));
  unsigned xoff[XP];
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int piece = min(w + NWV * i, 4 * TB - 1), row = 4 * piece + (lane >> 4);
    const int ch = w4_chunk(row, lane & 15);     // (the swizzle is an involution: slot chunk -> source chunk)
    const int srow = row < p.M ? row : p.M - 1;  // rows past M re-read the last real row (not stored)
    xoff[i] = (unsigned)(((long)srow * p.ldx) * 2 + ch * 16);
  }
  auto issue_x = [&](int t) {
    const int so = __builtin_amdgcn_readfirstlane((int)((k0 + (long)t * W4_BK) * 2));
    w4_issue_x<XP, NWV, TB, GS>(xrs, xoff, smem + (t & (NX - 1)) * XT, so, w);
  };
  // --- weights: per 16-row block and K-step 1 KiB of codes, 32 GS bytes of scales, 16 GS of zeros -----
  const long ksteps = p.K / W4_BK;
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(p.W, (unsigned)((long)p.N * p.K / 2));
  const __amdgpu_buffer_rsrc_t srs = make_rsrc(p.SC, (unsigned)((long)p.N * ksteps * GS * 2));
  const __amdgpu_buffer_rsrc_t zrs = make_rsrc(p.Z, (unsigned)((long)p.N * ksteps * GS));
  unsigned woff[NF], soff[NF], zoff[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const long at = ((n0 >> 4) + f) * ksteps + k0 / W4_BK;  // (block, step) index
    woff[f] = (unsigned)(at * 1024 + lane * 16);
    soff[f] = (unsigned)((at * 4 + gq) * (GS * 8));
    zoff[f] = (unsigned)((at * 4 + gq) * (GS * 4));
  }
  i32x4 wf[NX][NF];
  int sc[NX][NF][2 * GS], zp[NX][NF][GS];
  auto load_w = [&](int t, i32x4 (&dw)[NF], int (&ds)[NF][2 * GS], int (&dz)[NF][GS]) {
    w4_load_w<NF, TB, GS>(wrs, woff, __builtin_amdgcn_readfirstlane(t * 1024), dw);
    w4_load_sz<NF, TB, GS>(srs, zrs, soff, zoff, __builtin_amdgcn_readfirstlane(t * 32 * GS),
                       __builtin_amdgcn_readfirstlane(t * 16 * GS), ds, dz);
  };

  f32x4 acc[TB][NF];
#pragma unroll
  for (int tb = 0; tb < TB; ++tb)
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[tb][f] = f32x4{0.f, 0.f, 0.f, 0.f};
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
    load_w(j, wf[j], sc[j], zp[j]);
    __builtin_amdgcn_sched_barrier(0);
  }
  // one K-step on register set J (= t % NX).  ISSUE: it issues the loads of step t + D into the set
  // and slot of step t - 1; WN: the vmcnt that leaves every load of step t landed (everything issued
  // after it: the steps in between)
  auto step = [&](int t, auto J, auto ISSUE, auto WN) {
    constexpr int j = decltype(J)::value;
    stream::vmcnt<decltype(WN)::value>();
    stream::barrier();  // every wave's X(t); every wave is past step t-1 (its X slot is free)
    if constexpr (decltype(ISSUE)::value) {
      issue_x(t + D);
      load_w(t + D, wf[(j + D) % NX], sc[(j + D) % NX], zp[(j + D) % NX]);
    }
    __builtin_amdgcn_sched_barrier(0);
    // codes -> bf16 (128 + q), scales -> fp32, zero bytes -> 128 + z (EAGER above)
    bf16x8 a[4][NF];
    float s[NF][GS][4], zn[NF][GS][4];
    if constexpr (EAGER) {
#pragma unroll
      for (int f = 0; f < NF; ++f) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) a[kk][f] = w4_expand(wf[j][f][kk], kmask, kbias);
#pragma unroll
        for (int G = 0; G < GS; ++G)
          if constexpr (EAGER) w4_convert<GS>(sc[j][f], zp[j][f], G, s[f][G], zn[f][G]);
      }
    }
    // token-block fragments LA blocks ahead of their MFMAs (LA + 1 buffers of 4 ds_read_b128); the
    // scheduling barriers keep a block's reads, MFMAs and fold together, which bounds the live registers
    const char* st = smem + (t & (NX - 1)) * XT + r * 256;
    bf16x8 xf[LA + 1][4];
#pragma unroll
    for (int i = 0; i < LA; ++i) w4_read_x(st + i * 4096, r, gq, xf[i]);
#pragma unroll
    for (int tb = 0; tb < TB; ++tb) {
      if (tb + LA < TB) w4_read_x(st + (tb + LA) * 4096, r, gq, xf[(tb + LA) % (LA + 1)]);
      __builtin_amdgcn_sched_barrier(0);
      const bf16x8(&x)[4] = xf[tb % (LA + 1)];
#pragma unroll
      for (int G = 0; G < GS; ++G) {
        f32x4 P[NF], PX = zero4;
#pragma unroll
        for (int f = 0; f < NF; ++f) P[f] = zero4;
#pragma unroll
        for (int q = 0; q < KG; ++q) {
          const int kk = G * KG + q;
          PX = w4_mfma(ones, x[kk], PX);
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            if constexpr (EAGER)
              P[f] = w4_mfma(a[kk][f], x[kk], P[f]);
            else
              P[f] = w4_mfma(w4_expand(wf[j][f][kk], kmask, kbias), x[kk], P[f]);
          }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          if constexpr (!EAGER) w4_convert<GS>(sc[j][f], zp[j][f], G, s[f][G], zn[f][G]);
          w4_fold(acc[tb][f], P[f], PX[0], s[f][G], zn[f][G]);
          // (pins the fold here: without it the compiler sinks every step's folds to the end of the
          // unrolled loop body and keeps all their P alive until then -- hundreds of spilled registers)
          asm volatile("" : "+v"(acc[tb][f]));
        }
      }
      __builtin_amdgcn_sched_barrier(0);
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

  // --- epilogue: lane holds C[n = 4 gq + e][m = r] of each (token block, fragment) -----------------
  if (p.S > 1) {
    float* part = p.part + (long)blockIdx.y * p.M * p.N;
#pragma unroll
    for (int tb = 0; tb < TB; ++tb) {
      const int m = 16 * tb + r;
      if (m >= p.M) continue;
#pragma unroll
      for (int f = 0; f < NF; ++f)
        *reinterpret_cast<f32x4*>(part + (long)m * p.N + n0 + 16 * f + 4 * gq) = acc[tb][f];
    }
    return;
  }
#pragma unroll
  for (int tb = 0; tb < TB; ++tb) {
    const int m = 16 * tb + r;
    if (m >= p.M) continue;
#pragma unroll
    for (int f = 0; f < NF; ++f) stream::store_bf16x4(p.Y + (long)m * p.ldy + n0 + 16 * f + 4 * gq, acc[tb][f]);
  }
}

// 16-row token blocks of the form that runs M rows: 1 (M <= 16), 4 (<= 64), 8 (<= 128), 16
extern "C" int dsa_w4_gemm_form(int M) { return M <= 16 ? 1 : M <= 64 ? 4 : M <= 128 ? 8 : 16; }

extern "C" bool dsa_w4_gemm_supported(int M, int N, int K, int g) {
  // 256 weight rows per workgroup; K slices of 4 whole K-steps; codes and activations through 32-bit
  // buffer ranges
  return M > 0 && M <= W4_MAXM && N > 0 && N % W4_WG_ROWS == 0 && K > 0 && K % (W4_BK * W4_UNROLL) == 0 &&
         (g == 32 || g == 64 || g == 128) && (long)N * K / 2 <= 0xffffffffL;
}

// K slices: the most that divide K / 512, keep the grid within the CUs' workgroup slots (one per CU
// for the forms of 4 and more token blocks, two for the smallest) and keep the fp32 partials (written
// and read once) under the weight bytes: S * M * N * 8 <= N * K / 2
extern "C" int dsa_w4_gemm_split(int M, int N, int K) {
  if (!dsa_w4_gemm_supported(M, N, K, 128)) return 0;
  const int groups = K / (W4_BK * W4_UNROLL), wgs = N / W4_WG_ROWS;
  const int slots = dsa_w4_gemm_form(M) > 1 ? 256 : 512;
  int best = 1;
  for (int s = 2; s <= groups && s <= 16; ++s)
    if (groups % s == 0 && wgs * s <= slots && (long)s * M * 16 <= K) best = s;
  return best;
}

namespace {
template <int GS>
hipError_t w4_launch(const W4Args& a, hipStream_t st) {
  constexpr int NX = GS == 4 ? 2 : 4;  // ring slots of the forms below 16 token blocks (w4_gemm_kernel)
  static bool attr = false;
  if (!attr) {
    DSA_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&w4_gemm_kernel<16, 8, 2, GS>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 16 * 4096));
    DSA_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&w4_gemm_kernel<8, 8, 2, GS>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, NX * 8 * 4096));
    DSA_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&w4_gemm_kernel<4, 4, 4, GS>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, NX * 4 * 4096));
    attr = true;
  }
  const dim3 grid(a.N / W4_WG_ROWS, a.S);
  switch (dsa_w4_gemm_form(a.M)) {
    case 1: w4_gemm_kernel<1, 4, 4, GS><<<grid, 256, NX * 1 * 4096, st>>>(a); break;
    case 4: w4_gemm_kernel<4, 4, 4, GS><<<grid, 256, NX * 4 * 4096, st>>>(a); break;
    case 8: w4_gemm_kernel<8, 8, 2, GS><<<grid, 512, NX * 8 * 4096, st>>>(a); break;
    default: w4_gemm_kernel<16, 8, 2, GS><<<grid, 512, 2 * 16 * 4096, st>>>(a); break;
  }
  return hipGetLastError();
}
}  // namespace

// Y[M][N] = bf16(X W^T): X [M][K] bf16 (row stride ldx elements), W the stored W4 weight (codes
// N * K / 2 bytes, zeros N * K / g bytes, scales N * K / g fp16: ops.serving.w4_shuffle), Y bf16 (ldy
// elements).  S = dsa_w4_gemm_split(M, N, K); S > 1: `part` holds S * M * N floats.
extern "C" hipError_t dsa_w4_gemm(const void* X, const void* W, const void* Z, const void* SC, void* Y, float* part,
                                  int M, int N, int K, int g, long ldx, long ldy, int S, hipStream_t st) {
  if (!dsa_w4_gemm_supported(M, N, K, g) || ldx % 8 || ldy % 4 || ldx < K || ldy < N) return hipErrorInvalidValue;
  if (S < 1 || K % (W4_BK * W4_UNROLL * S) || (S > 1 && part == nullptr)) return hipErrorInvalidValue;
  if (((long)(M - 1) * ldx + K) * 2 > 0xffffffffL) return hipErrorInvalidValue;  // X through a 32-bit buffer range
  W4Args a{(const bf16_t*)X, (const uint8_t*)W, (const uint8_t*)Z, (const uint8_t*)SC, (bf16_t*)Y, part, ldx, ldy,
           M, N, K, S};
  DSA_CHECK(g == 128 ? w4_launch<1>(a, st) : g == 64 ? w4_launch<2>(a, st) : w4_launch<4>(a, st));
  return S > 1 ? stream::reduce<false, false>(part, nullptr, nullptr, Y, M, N, ldy, S, st) : hipSuccess;
}

// ================================================================================================
// Dequantizer
// ================================================================================================
// The stored weight back to bf16 [N][K] (row stride ldo elements): element (n, k) = bf16((q - z) s), the
// fp32 product rounded once.  One thread per lane piece (16 B of codes = 4 x 8 consecutive elements),
// writing four 16-byte runs.  The stored form covers Kp = K rounded up to 128 columns; the padding is
// not written.
__global__ __launch_bounds__(256) void w4_dequant_kernel(const uint8_t* __restrict__ W, const uint8_t* __restrict__ Z,
                                                         const uint16_t* __restrict__ SC, bf16_t* __restrict__ out,
                                                         long ldo, int N, int K, int Kp, int g) {
  const long ksteps = Kp / W4_BK, total = (long)N * ksteps * 4;
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int lane = (int)(i & 63), r = lane & 15, gq = lane >> 4;
  const long at = i >> 6, t = at % ksteps, blk = at / ksteps;  // (block, step) index `at`
  const int GS = W4_BK / g;
  const uint4 c = *reinterpret_cast<const uint4*>(W + (at * 64 + lane) * 16);
  const unsigned words[4] = {c.x, c.y, c.z, c.w};
  bf16_t* dst = out + (16 * blk + r) * ldo + t * W4_BK + 8 * gq;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const long k = t * W4_BK + 32 * kk + 8 * gq;
    if (k >= K) continue;
    const long sz = ((at * 4 + (r >> 2)) * GS + (32 * kk + 8 * gq) / g) * 4 + (r & 3);
    const float s = w4_half(SC[sz]), z = (float)(Z[sz] - 128);  // (the stored byte is 128 + z)
    us8 o;
#pragma unroll
    for (int pq = 0; pq < 8; ++pq) {
      const int j = pq < 4 ? 2 * pq : 2 * (pq - 4) + 1;  // nibble pq holds element j
      o[j] = f2bf(((float)((words[kk] >> (4 * pq)) & 15u) - z) * s);
    }
    *reinterpret_cast<us8*>(dst + 32 * kk) = o;
  }
}

// W, Z, SC: the stored form of an [N][K] weight (N % 16 == 0, K % g == 0): Kp = K rounded up to 128
extern "C" hipError_t dsa_w4_dequant(const void* W, const void* Z, const void* SC, void* out, long ldo, int N, int K,
                                     int g, hipStream_t st) {
  if (N <= 0 || N % 16 || K <= 0 || (g != 32 && g != 64 && g != 128) || K % g || ldo % 8 || ldo < K)
    return hipErrorInvalidValue;
  const int Kp = (K + W4_BK - 1) / W4_BK * W4_BK;
  const long total = (long)N * (Kp / W4_BK) * 4;
  w4_dequant_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>((const uint8_t*)W, (const uint8_t*)Z,
                                                                     (const uint16_t*)SC, (bf16_t*)out, ldo, N, K, Kp, g);
  return hipGetLastError();
}
