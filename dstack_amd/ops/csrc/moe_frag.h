// What the routed expert GEMMs over bf16 weights share (moe.hip: moe_gemm, few large experts;
// moe_fine.hip: moe_fine_gemm, many small ones): the argument block, the swizzle of the activation
// ring, a lane's weight loads of one K-step, the B-operand reads of one token block and the MFMA.
// Each file keeps its own tile, wave count, ring depth, K loop and activation issue.  moe_load_w
// carries a tag per instantiation (see the header of stream_frag.h).  Device code only: what the
// launch code of these two and of moe_w4.hip shares is in moe_host.h.
#pragma once

#include "stream_frag.h"

namespace dsa {
namespace moe {

using stream::f32x4;
using stream::i32x4;

constexpr int MOE_MAXR = 256;  // token rows
constexpr int MOE_PREFILL_MAXR = 2048;  // token rows of moe_prefill.hip, and of moe_swiglu / moe_combine after either
constexpr int MOE_MAXK = 8;    // experts per token
constexpr int MOE_BK = 128;    // K elements per step
constexpr int MOE_NF = 2;      // 16-row weight fragments per wave

struct MoeArgs {
  const bf16_t* X;    // bf16 [xrows][ldx]
  const bf16_t* W;    // bf16 [E][N][K]
  const int* counts;  // [E]
  const int* lists;   // [E][R]
  float* part;        // [S][P][N] fp32
  long ldx;           // elements
  int xrows, src_div, R, P, N, K, S;
};

// 16-byte chunk of a 256-byte activation row that holds K elements [8 c, 8 c + 8) of token `row`
__device__ __forceinline__ int moe_chunk(int row, int c) { return c ^ (row & 15); }

// a lane's A operands of one K-step: per fragment four 16-byte pieces 64 bytes apart in its weight row
template <int LB, int TB>
__device__ __forceinline__ void moe_load_w(__amdgpu_buffer_rsrc_t wrs, const unsigned (&woff)[MOE_NF], int so,
                                           i32x4 (&dst)[MOE_NF][4]) {
#pragma unroll
  for (int f = 0; f < MOE_NF; ++f)
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const auto a = __builtin_amdgcn_raw_buffer_load_b128(wrs, (int)woff[f] + 64 * kk, so, 2);  // 2: nontemporal
      dst[f][kk] = i32x4{(int)a[0], (int)a[1], (int)a[2], (int)a[3]};
    }
}

// the 4 MFMA steps' B operands of one token block: token r (`row` points at it), K chunks 4 kk + gq
__device__ __forceinline__ void moe_read_x(const char* row, int r, int gq, bf16x8 (&xf)[4]) {
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) xf[kk] = *reinterpret_cast<const bf16x8*>(row + moe_chunk(r, 4 * kk + gq) * 16);
}

__device__ __forceinline__ f32x4 moe_mfma(const i32x4& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), b, c, 0, 0, 0);
}

// silu(g) u in fp32: what moe_swiglu (moe.hip) and the gate/up epilogue of moe_prefill_gemm (moe_prefill.hip)
// round to bf16
__device__ __forceinline__ float moe_silu_mul(float g, float u) { return g / (1.f + expf(-g)) * u; }

}  // namespace moe
}  // namespace dsa
