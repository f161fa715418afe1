// MFMA operand helpers shared by the paged-KV-cache attention kernels (paged_attn.hip: decode,
// paged_prefill.hip: prefill of new tokens over a cached prefix).  Cache geometry: PAGE tokens per
// page, head_dim HDIM (see paged_attn.hip for the layouts).
#pragma once

#include "common.h"

namespace dsa {
namespace paged {

constexpr int PAGE = 64;
constexpr int HDIM = 128;

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x4_t mfma16(const bf16x8_t& a, const bf16x8_t& b, const f32x4_t& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ bf16x8_t ld8(const bf16_t* p) { return *reinterpret_cast<const bf16x8_t*>(p); }

// 8 e4m3 cache bytes (held raw while in flight: half the registers of bf16) -> the same bf16x8
// MFMA operand the bf16 cache gives, converted right before the MFMA that reads it
__device__ __forceinline__ bf16x8_t fp8x8_to_bf16(const u2_t w) {
  bf16x8_t r;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[h], false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[h], true);
    r[4 * h + 0] = (__bf16)lo[0];
    r[4 * h + 1] = (__bf16)lo[1];
    r[4 * h + 2] = (__bf16)hi[0];
    r[4 * h + 3] = (__bf16)hi[1];
  }
  return r;
}

}  // namespace paged
}  // namespace dsa
