// MXFP4 (OCP MX v1.0: e2m1 codes, one E8M0 scale per 32 elements along K) weights for the serving
// engine on CDNA4 (gfx950): the load-time quantizer, the decode GEMM and the exact dequantizer.
//
// Decode GEMM: Y[m][n] = bf16( xs[m] * sum_k X[m][k] * 2^(sc[n][k/32] - 127) * e2m1(W[n][k]) ) for
// 1 <= M <= 256 token rows.  It is fp8_stream_gemm (fp8_gemm.hip) with the weight operand in FP4:
//  * v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = 4: the weights are the A operand (FP4, the first
//    4 of its 8 VGPRs) with their real E8M0 scales, the activations the e4m3 B operand with unit
//    scale; a lane's accumulator holds 4 consecutive output columns of one token row;
//  * lane (r = lane & 15, g = lane >> 4) holds weight row r, K elements [32 g, 32 g + 32) of a
//    128-wide K-step: one MX block, so one scale byte per lane and step (and, of the activations,
//    token row r, K bytes [16 g, 16 g + 16) and [64 + 16 g, 64 + 16 g + 16): see mx_swz).  The scales of 4 K-steps
//    sit in one dword per lane, picked by op_sel;
//  * the stored weight (ops.serving.mxfp4_shuffle) is in that order: per 16-row block and K-step the
//    1 KiB of codes in lane order, per 16-row block and 4 K-steps the 256 B of scale dwords in lane
//    order.  Every weight load is a contiguous 1 KiB, nontemporal (read once), through a buffer
//    descriptor sized to the exact byte count (a bad offset reads zeros);
//  * the activations (L2-resident: every workgroup reads them) are LDS-DMA'd into a 4-slot ring
//    (swizzled: mx_swz), D = 3 K-steps ahead, one bare barrier per step (stream_frag.h);
//  * K is split over gridDim.y with fp32 partials [S][M][N] that stream::reduce_kernel adds in a fixed
//    order (no atomics: a seeded request stays reproducible).
// Forms, by 16-row token blocks TB (a 1-row batch must not run 16 blocks of MFMAs):
//    TB 16 (M <= 256) and TB 8 (M <= 128): 8 waves x 2 fragments -- 128 / 64 accumulator VGPRs;
//    TB 4  (M <= 64)  and TB 1 (M <= 16):  4 waves x 4 fragments -- 64 / 16 accumulator VGPRs, two
//    or more workgroups per CU.
// All cover 256 weight rows per workgroup.  In flight per workgroup: D = 3 steps x 16 fragments x 1 KiB
// = 48 KiB of codes.  The in-flight-bytes argument in the header of fp8_gemm.hip: an FP4 step is half
// the bytes of an fp8 one, so the distance is 3 steps and the small forms, whose accumulators leave
// the registers free, run 2-4 workgroups per CU.
#include <stdint.h>

#include <type_traits>

#include "stream_frag.h"

using namespace dsa;
using stream::f32x4;
using stream::i32x4;
using stream::i32x8;

namespace {

constexpr int MX_MAXM = 256;   // token rows
constexpr int MX_BK = 128;     // K elements (activation bytes) per step
constexpr int MX_WG_ROWS = 256;  // weight rows per workgroup, every form
constexpr int MX_NX = 4;       // activation ring slots
constexpr int MX_GROUP = 4;    // K-steps per scale dword (and the unroll factor)

struct MXArgs {
  const uint8_t* X;    // e4m3 [M][ldx]
  const float* xs;     // [M]
  const uint8_t* W;    // stored codes, N * K / 2 bytes
  const uint8_t* SC;   // stored scales, N * K / 32 bytes
  bf16_t* Y;
  float* part;         // [S][M][N] fp32 (S > 1)
  long ldx, ldy;
  int M, N, K, S;
};

// 16-byte-chunk XOR swizzle of the activation tiles (128-byte rows).  The e4m3 B operand of the
// 128-wide MFMA is two K = 64 halves: lane (r, g) holds K bytes [16 g, 16 g + 16) in its first 4
// VGPRs and [64 + 16 g, 64 + 16 g + 16) in the other 4 (measured with one-hot operands; the FP4 A
// operand holds [32 g, 32 g + 32)), so a fragment is chunks g and g + 4 of row r.  A ds_read_b128
// lane group holds rows of lane groups g and g + 1 (g even), whose chunks differ in bit 0: the XOR
// uses bits 1 and 2, and with the row's parity (8 chunks per 256-B bank row) the 16 lanes of a group
// hit 16 different 16-byte bank windows.
__device__ __forceinline__ int mx_swz(int r) { return (((r >> 1) & 1) << 1) | (((r >> 3) & 1) << 2); }

// XP 1 KiB activation pieces (8 token rows x 128 B) per wave and step; pieces past the last one are
// the last one again (identical bytes to one slot), so every wave issues the same number of loads
template <int XP, int NWV, int TB>
__device__ __forceinline__ void mx_issue_x(__amdgpu_buffer_rsrc_t xrs, const unsigned (&xoff)[XP], char* slot, int so,
                                           int w) {
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int piece = min(w + NWV * i, 2 * TB - 1);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, LDS3(void, slot + piece * 1024), 16, xoff[i], so, 0, 0);
  }
}

template <int NF, int TB>
__device__ __forceinline__ void mx_load_w(__amdgpu_buffer_rsrc_t wrs, const unsigned (&woff)[NF], int so,
                                          i32x4 (&dst)[NF]) {
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const auto a = __builtin_amdgcn_raw_buffer_load_b128(wrs, (int)woff[f], so, 2);  // 2: nontemporal
    dst[f] = i32x4{(int)a[0], (int)a[1], (int)a[2], (int)a[3]};
  }
}

// acc += A (FP4, 4 VGPRs, E8M0 scale byte J of `sa` per lane) x B (e4m3, 8 VGPRs, unit scale) in place.
// Inline assembly: the builtin's FP4 form has no accumulate-in-place variant, so the register
// allocator moved the accumulators through fresh registers at every step and the 256-row form
// spilled 15 VGPRs into its main loop.  The scale byte selector is op_sel (bit 0) and op_sel_hi
// (bit 1) of the first source.  s_nop 1: the compiler pads nothing around inline assembly (two wait
// states cover a dependent MFMA on the same accumulator; every other producer of an operand is a
// memory load the compiler waits for).
template <int J>
__device__ __forceinline__ void mx_mfma(f32x4& acc, const i32x4& a, const i32x8& b, int sa, int unit) {
  static_assert(J >= 0 && J < 4, "scale byte");
  if constexpr (J == 0)
    asm volatile("s_nop 1\n\tv_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0] cbsz:4"
                 : "+v"(acc) : "v"(a), "v"(b), "v"(sa), "v"(unit));
  else if constexpr (J == 1)
    asm volatile("s_nop 1\n\tv_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel:[1,0,0] op_sel_hi:[0,0,0] cbsz:4"
                 : "+v"(acc) : "v"(a), "v"(b), "v"(sa), "v"(unit));
  else if constexpr (J == 2)
    asm volatile("s_nop 1\n\tv_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[1,0,0] cbsz:4"
                 : "+v"(acc) : "v"(a), "v"(b), "v"(sa), "v"(unit));
  else
    asm volatile("s_nop 1\n\tv_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel:[1,0,0] op_sel_hi:[1,0,0] cbsz:4"
                 : "+v"(acc) : "v"(a), "v"(b), "v"(sa), "v"(unit));
}

template <int NF, int TB>
__device__ __forceinline__ void mx_load_sc(__amdgpu_buffer_rsrc_t srs, const unsigned (&soff)[NF], int so,
                                           int (&dst)[NF]) {
#pragma unroll
  for (int f = 0; f < NF; ++f) dst[f] = (int)__builtin_amdgcn_raw_buffer_load_b32(srs, (int)soff[f], so, 2);
}

}  // namespace

// TB 16-row token blocks, NWV waves x NF 16-row weight fragments per wave (NWV * NF == 16)
template <int TB, int NWV, int NF>
__global__ __launch_bounds__(64 * NWV, TB >= 8 ? 1 : 2) void mxfp4_gemm_kernel(MXArgs p) {
  constexpr int D = 3, NSET = MX_GROUP;  // prefetch distance in K-steps; weight register sets
  constexpr int XT = TB * 2048;                   // one ring slot: 16 TB token rows x 128 B
  constexpr int XP = (2 * TB + NWV - 1) / NWV;    // activation pieces per wave per step
  constexpr int OPS = XP + NF;                    // vector-memory ops per wave per step
  static_assert(NWV * NF * 16 == MX_WG_ROWS && D + 1 <= NSET && D + 1 <= MX_NX, "form");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int n0 = (blockIdx.x * NWV + w) * 16 * NF;  // this wave's first weight row
  const int ks = p.K / p.S, nsteps = ks / MX_BK;    // a multiple of 4 steps
  const long k0 = (long)blockIdx.y * ks;

  // --- activation DMA ---------------------------------------------------------------------------
  const __amdgpu_buffer_rsrc_t xrs = make_rsrc(p.X, (unsigned)((long)(p.M - 1) * p.ldx + p.K));
  unsigned xoff[XP];
#pragma unroll
  for (int i = 0; i < XP; ++i) {
    const int piece = min(w + NWV * i, 2 * TB - 1), row = 8 * piece + (lane >> 3);
    const int ch = (lane & 7) ^ mx_swz(row & 15);
    const int srow = row < p.M ? row : p.M - 1;  // rows past M re-read the last real row (not stored)
    xoff[i] = (unsigned)((long)srow * p.ldx + ch * 16);
  }
  auto issue_x = [&](int t) {
    const int so = __builtin_amdgcn_readfirstlane((int)(k0 + (long)t * MX_BK));
    mx_issue_x<XP, NWV, TB>(xrs, xoff, smem + (t & (MX_NX - 1)) * XT, so, w);
  };
  // --- weights: per 16-row block and K-step 1 KiB of codes, per block and 4 steps 256 B of scales --
  const long ksteps = p.K / MX_BK, kgroups = ksteps / MX_GROUP;
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(p.W, (unsigned)((long)p.N * p.K / 2));
  const __amdgpu_buffer_rsrc_t srs = make_rsrc(p.SC, (unsigned)((long)p.N * p.K / 32));
  unsigned woff[NF], soff[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const long blk = (n0 >> 4) + f;
    woff[f] = (unsigned)((blk * ksteps + k0 / MX_BK) * 1024 + lane * 16);
    soff[f] = (unsigned)((blk * kgroups + k0 / (MX_BK * MX_GROUP)) * 256 + lane * 4);
  }
  auto load_w = [&](int t, i32x4 (&dst)[NF]) {
    mx_load_w<NF, TB>(wrs, woff, __builtin_amdgcn_readfirstlane(t * 1024), dst);
  };
  auto load_sc = [&](int grp, int (&dst)[NF]) {
    mx_load_sc<NF, TB>(srs, soff, __builtin_amdgcn_readfirstlane(grp * 256), dst);
  };

  f32x4 acc[TB][NF];
#pragma unroll
  for (int tb = 0; tb < TB; ++tb)
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[tb][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int sw = mx_swz(r), c0 = (g ^ sw) * 16, c1 = ((g + 4) ^ sw) * 16;
  const int unit = 127;  // E8M0 1.0 for the activations

  // prologue in the order the waits count: S(0), X(0) W(0) ... X(D-1) W(D-1)
  i32x4 wf[NSET][NF];
  int sc[NF], scn[NF];
  // (pinned: reordered prologue loads would make the compiler's own waits for the first weight sets,
  // which are static and so apply to every iteration, stricter than the steady state needs)
  load_sc(0, sc);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < D; ++j) {
    issue_x(j);
    __builtin_amdgcn_sched_barrier(0);
    load_w(j, wf[j]);
    __builtin_amdgcn_sched_barrier(0);
  }
  // one K-step on weight set J (= t % 4: byte J of the scale dword).  ISSUE: it issues X(t+D), W(t+D);
  // NEXTSC: it is the first step of a group that is not the last and loads the next group's scales;
  // WN: the vmcnt that leaves this wave's X(t) landed (everything issued after W(t))
  auto step = [&](int t, auto J, auto ISSUE, auto NEXTSC, auto WN) {
    constexpr int j = decltype(J)::value;
    stream::vmcnt<decltype(WN)::value>();
    stream::barrier();  // every wave's X(t); every wave is past step t-1 (its X slot is free)
    if constexpr (decltype(ISSUE)::value) {
      issue_x(t + D);
      load_w(t + D, wf[(j + D) % NSET]);
    }
    if constexpr (decltype(NEXTSC)::value) load_sc(t / MX_GROUP + 1, scn);
    __builtin_amdgcn_sched_barrier(0);
    const char* st = smem + (t & (MX_NX - 1)) * XT + r * MX_BK;
    if constexpr (TB <= 2) {
      i32x8 xf[TB];
#pragma unroll
      for (int tb = 0; tb < TB; ++tb) xf[tb] = stream::frag(st + tb * 2048 + c0, st + tb * 2048 + c1);
#pragma unroll
      for (int tb = 0; tb < TB; ++tb)
#pragma unroll
        for (int f = 0; f < NF; ++f) mx_mfma<j>(acc[tb][f], wf[j][f], xf[tb], sc[f], unit);
    } else {
      // token-block fragments LA = 2 blocks ahead of their MFMAs (3 buffers); the scheduling barriers
      // keep each block's two ds_read_b128 in front of the MFMAs of the block LA before it
      constexpr int LA = 2;
      i32x8 xf[LA + 1];
#pragma unroll
      for (int i = 0; i < LA; ++i) xf[i] = stream::frag(st + i * 2048 + c0, st + i * 2048 + c1);
#pragma unroll
      for (int tb = 0; tb < TB; ++tb) {
        if (tb + LA < TB)
          xf[(tb + LA) % (LA + 1)] = stream::frag(st + (tb + LA) * 2048 + c0, st + (tb + LA) * 2048 + c1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int f = 0; f < NF; ++f) mx_mfma<j>(acc[tb][f], wf[j][f], xf[tb % (LA + 1)], sc[f], unit);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  using T = std::true_type;
  using F = std::false_type;
  using W0 = std::integral_constant<int, 0>;
  // issued after X(t), W(t) in a full group: (D - 1) steps' X and W, and the scale loads of the
  // group's first step when that step lies in (t - D, t - 1] (j = 1 .. D - 1)
  using WA = std::integral_constant<int, (D - 1) * OPS>;
  using WB = std::integral_constant<int, (D - 1) * OPS + NF>;
  using W3 = std::conditional_t<D == 4, WB, WA>;
  const int last = nsteps - NSET;
  for (int t0 = 0; t0 < last; t0 += NSET) {
    step(t0 + 0, std::integral_constant<int, 0>{}, T{}, T{}, WA{});
    step(t0 + 1, std::integral_constant<int, 1>{}, T{}, F{}, WB{});
    step(t0 + 2, std::integral_constant<int, 2>{}, T{}, F{}, WB{});
    step(t0 + 3, std::integral_constant<int, 3>{}, T{}, F{}, W3{});
#pragma unroll
    for (int f = 0; f < NF; ++f) sc[f] = scn[f];
  }
  // the last group loads no scales; its steps with j + D < 4 still issue and wait as usual, the rest drain
  step(last + 0, std::integral_constant<int, 0>{}, std::bool_constant<(0 + D < NSET)>{}, F{},
       std::integral_constant<int, (0 + D < NSET) ? (D - 1) * OPS : 0>{});
  step(last + 1, std::integral_constant<int, 1>{}, std::bool_constant<(1 + D < NSET)>{}, F{},
       std::integral_constant<int, (1 + D < NSET) ? (D - 1) * OPS : 0>{});
  step(last + 2, std::integral_constant<int, 2>{}, std::bool_constant<(2 + D < NSET)>{}, F{},
       std::integral_constant<int, (2 + D < NSET) ? (D - 1) * OPS : 0>{});
  step(last + 3, std::integral_constant<int, 3>{}, F{}, F{}, W0{});

  // the last MFMAs' results are not readable by vector ALU / store instructions for up to 19 wait
  // states (16-pass MFMA), which the compiler does not count for inline assembly
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  // --- epilogue: lane holds C[n = 4 g + e][m = r] of each (token block, fragment) ------------------
  if (p.S > 1) {
    float* part = p.part + (long)blockIdx.y * p.M * p.N;
#pragma unroll
    for (int tb = 0; tb < TB; ++tb) {
      const int m = 16 * tb + r;
      if (m >= p.M) continue;
#pragma unroll
      for (int f = 0; f < NF; ++f)
        *reinterpret_cast<f32x4*>(part + (long)m * p.N + n0 + 16 * f + 4 * g) = acc[tb][f];
    }
    return;
  }
#pragma unroll
  for (int tb = 0; tb < TB; ++tb) {
    const int m = 16 * tb + r;
    if (m >= p.M) continue;
    const float xsc = p.xs[m];
#pragma unroll
    for (int f = 0; f < NF; ++f)
      stream::store_bf16x4(p.Y + (long)m * p.ldy + n0 + 16 * f + 4 * g, acc[tb][f], xsc);
  }
}

// 16-row token blocks of the form that runs M rows: 1 (M <= 16), 4 (<= 64), 8 (<= 128), 16
extern "C" int dsa_mxfp4_gemm_form(int M) { return M <= 16 ? 1 : M <= 64 ? 4 : M <= 128 ? 8 : 16; }

extern "C" bool dsa_mxfp4_gemm_supported(int M, int N, int K) {
  // 256 weight rows per workgroup; K slices of whole scale dwords (4 K-steps); codes and activations
  // through 32-bit buffer ranges
  return M > 0 && M <= MX_MAXM && N > 0 && N % MX_WG_ROWS == 0 && K > 0 && K % (MX_BK * MX_GROUP) == 0 &&
         (long)N * K / 2 <= 0xffffffffL;
}

// K slices: the most that divide K / 512, keep the grid within the CUs' workgroup slots (one per CU
// for the 8-wave forms, two for the 4-wave ones) and keep the fp32 partials (written and read once)
// under the weight bytes: S * M * N * 8 <= N * K / 2
extern "C" int dsa_mxfp4_gemm_split(int M, int N, int K) {
  if (!dsa_mxfp4_gemm_supported(M, N, K)) return 0;
  const int groups = K / (MX_BK * MX_GROUP), wgs = N / MX_WG_ROWS;
  const int slots = dsa_mxfp4_gemm_form(M) >= 8 ? 256 : 512;
  int best = 1;
  for (int s = 2; s <= groups && s <= 16; ++s)
    if (groups % s == 0 && wgs * s <= slots && (long)s * M * 16 <= K) best = s;
  return best;
}

// Y[M][N] = bf16(xs[m] * X W^T): X [M][K] e4m3 (row stride ldx bytes), W the stored MXFP4 weight
// (codes N * K / 2 bytes, scales N * K / 32 bytes, ops.serving.mxfp4_shuffle), Y bf16 (ldy elements).
// S = dsa_mxfp4_gemm_split(M, N, K); S > 1: `part` holds S * M * N floats.
extern "C" hipError_t dsa_mxfp4_gemm(const void* X, const float* xs, const void* W, const void* SC, void* Y,
                                     float* part, int M, int N, int K, long ldx, long ldy, int S, hipStream_t st) {
  if (!dsa_mxfp4_gemm_supported(M, N, K) || ldx % 16 || ldy % 4 || ldx < K || ldy < N) return hipErrorInvalidValue;
  if (S < 1 || K % (MX_BK * MX_GROUP * S) || (S > 1 && part == nullptr)) return hipErrorInvalidValue;
  if ((long)(M - 1) * ldx + K > 0xffffffffL) return hipErrorInvalidValue;  // X through a 32-bit buffer range
  static bool attr = false;
  if (!attr) {
    DSA_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&mxfp4_gemm_kernel<16, 8, 2>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, MX_NX * 16 * 2048));
    DSA_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&mxfp4_gemm_kernel<8, 8, 2>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, MX_NX * 8 * 2048));
    attr = true;
  }
  MXArgs a{(const uint8_t*)X, xs, (const uint8_t*)W, (const uint8_t*)SC, (bf16_t*)Y, part, ldx, ldy, M, N, K, S};
  const dim3 grid(N / MX_WG_ROWS, S);
  switch (dsa_mxfp4_gemm_form(M)) {
    case 1: mxfp4_gemm_kernel<1, 4, 4><<<grid, 256, MX_NX * 1 * 2048, st>>>(a); break;
    case 4: mxfp4_gemm_kernel<4, 4, 4><<<grid, 256, MX_NX * 4 * 2048, st>>>(a); break;
    case 8: mxfp4_gemm_kernel<8, 8, 2><<<grid, 512, MX_NX * 8 * 2048, st>>>(a); break;
    default: mxfp4_gemm_kernel<16, 8, 2><<<grid, 512, MX_NX * 16 * 2048, st>>>(a); break;
  }
  DSA_CHECK(hipGetLastError());
  return S > 1 ? stream::reduce<false>(part, xs, nullptr, Y, M, N, ldy, S, st) : hipSuccess;
}

// ================================================================================================
// Quantizer (load time) and dequantizer
// ================================================================================================
namespace {
// e2m1 magnitude of code c (0..7): 0, 0.5, 1, 1.5, 2, 3, 4, 6
__device__ __forceinline__ float mx_e2m1(int c) {
  const int e = c >> 1, m = c & 1;
  return e ? (1.f + 0.5f * m) * (float)(1 << (e - 1)) : 0.5f * m;
}
// 2^(b - 127) for an E8M0 byte b < 255 (b = 0: the fp32 subnormal 2^-127)
__device__ __forceinline__ float mx_e8m0(int b) { return __uint_as_float(b ? (unsigned)b << 23 : 0x00400000u); }
}  // namespace

// One thread per MX block (32 elements along K) of W bf16 [N][K] (row stride ldw elements): the OCP MX
// v1.0 rule -- e = floor(log2(amax)) - 2 clamped to [-127, 127] (-127 for a zero block), elements
// x / 2^e rounded to nearest even on the e2m1 grid, saturated at 6, with the input's sign bit.
// Canonical output: codes [N][K/2] (element 2j in the low nibble), scales [N][K/32].
__global__ __launch_bounds__(256) void mxfp4_quant_kernel(const bf16_t* __restrict__ W, long ldw,
                                                          uint8_t* __restrict__ codes, uint8_t* __restrict__ scales,
                                                          int N, int K) {
  const long kb = K / 32, total = (long)N * kb;
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long n = i / kb, b = i % kb;
  const bf16_t* src = W + n * ldw + b * 32;
  us8 v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = *reinterpret_cast<const us8*>(src + 8 * q);
  unsigned amax = 0;  // |x| as bf16 bits: ordered like the values (finite inputs)
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = max(amax, (unsigned)(v[q][j] & 0x7fff));
  // floor(log2(amax)) = exponent field - 127 (a subnormal or zero amax clamps to -127 either way)
  int e = (int)(amax >> 7) - 127 - 2;
  e = e < -127 ? -127 : e;  // (the exponent field is at most 254: e <= 125)
  const float inv = mx_e8m0(127 - e);  // 2^-e, e in [-127, 125]: byte 254 .. 2
  unsigned out[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned word = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = bf2f(v[q][j] & 0x7fff) * inv;
      int c;
      if (a < 2.f) c = (int)rintf(2.f * a);               // 0, 0.5, 1, 1.5, 2 -> codes 0..4
      else if (a < 4.f) c = 2 + (int)rintf(a);            // 2, 3, 4 -> codes 4..6
      else c = min(7, 4 + (int)rintf(0.5f * a));          // 4, 6, (8 -> 6) -> codes 6, 7
      word |= (unsigned)(c | ((v[q][j] >> 15) << 3)) << (4 * j);
    }
    out[q] = word;
  }
  *reinterpret_cast<uint4*>(codes + n * (K / 2) + b * 16) = uint4{out[0], out[1], out[2], out[3]};
  scales[n * kb + b] = (uint8_t)(e + 127);
}

extern "C" hipError_t dsa_mxfp4_quant(const void* W, long ldw, void* codes, void* scales, int N, int K,
                                      hipStream_t st) {
  if (N <= 0 || K <= 0 || K % 32 || ldw % 8 || ldw < K) return hipErrorInvalidValue;
  const long total = (long)N * (K / 32);
  mxfp4_quant_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>((const bf16_t*)W, ldw, (uint8_t*)codes,
                                                                      (uint8_t*)scales, N, K);
  return hipGetLastError();
}

// The stored weight back to bf16 [N][K] (row stride ldo elements), exactly: one thread per lane piece
// (16 B of codes = 32 elements), 4 consecutive threads writing 256 contiguous bytes of a row.  The
// stored form covers Kp = K rounded up to 512 columns; the padding is not written.
__global__ __launch_bounds__(256) void mxfp4_dequant_kernel(const uint8_t* __restrict__ W,
                                                            const uint8_t* __restrict__ SC, bf16_t* __restrict__ out,
                                                            long ldo, int N, int K, int Kp) {
  const long ksteps = Kp / MX_BK, kgroups = ksteps / MX_GROUP, total = (long)N * ksteps * 4;
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int g = (int)(i & 3), r = (int)((i >> 2) & 15);
  const long rest = i >> 6, t = rest % ksteps, blk = rest / ksteps;
  if (t * MX_BK + 32 * g >= K) return;
  const int lane = r + 16 * g;
  const uint4 c = *reinterpret_cast<const uint4*>(W + ((blk * ksteps + t) * 64 + lane) * 16);
  const float s = mx_e8m0(SC[((blk * kgroups + t / MX_GROUP) * 64 + lane) * 4 + (t % MX_GROUP)]);
  const unsigned words[4] = {c.x, c.y, c.z, c.w};
  bf16_t* dst = out + (16 * blk + r) * ldo + t * MX_BK + 32 * g;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    us8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int nib = (words[q] >> (4 * j)) & 15;
      // (exact: an e2m1 value times a power of two has at most 2 significant bits)
      o[j] = (bf16_t)((__float_as_uint(mx_e2m1(nib & 7) * s) >> 16) | ((nib >> 3) << 15));
    }
    *reinterpret_cast<us8*>(dst + 8 * q) = o;
  }
}

// W, SC: the stored form of an [N][K] weight (N % 16 == 0, K % 32 == 0): N * Kp / 2 and N * Kp / 32 bytes
extern "C" hipError_t dsa_mxfp4_dequant(const void* W, const void* SC, void* out, long ldo, int N, int K,
                                        hipStream_t st) {
  if (N <= 0 || N % 16 || K <= 0 || K % 32 || ldo % 8 || ldo < K) return hipErrorInvalidValue;
  const int Kp = (K + MX_BK * MX_GROUP - 1) / (MX_BK * MX_GROUP) * (MX_BK * MX_GROUP);
  const long total = (long)N * (Kp / MX_BK) * 4;
  mxfp4_dequant_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>((const uint8_t*)W, (const uint8_t*)SC,
                                                                        (bf16_t*)out, ldo, N, K, Kp);
  return hipGetLastError();
}
