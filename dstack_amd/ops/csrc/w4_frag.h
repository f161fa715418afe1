// What the W4A16 decode GEMMs share (w4.hip: w4_gemm; moe_w4.hip: moe_w4_gemm, the same weight stream
// per expert): the loads of a lane's scales and zero bytes, the expansion of a stored dword of codes
// to the bf16 values 128 + q, the conversion of a group's scales and zeros and the fold of a group's
// MFMA sums into the accumulator.  The stored form is ops.serving.w4_shuffle's; the arithmetic is
// described in the header of w4.hip.  Each file keeps its own K loop, activation ring and code loads.
// w4_load_sz carries a tag per kernel instantiation (see the header of stream_frag.h).
#pragma once

#include "stream_frag.h"

namespace dsa {
namespace w4 {

using stream::f32x4;
using stream::i32x4;

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
// and bias = 0x43004300 come in registers (the kernels hide their values from the compiler): as
// literals the compiler emits v_and_b32 + v_or_b32, the VOP3 v_and_or_b32 taking no literal
__device__ __forceinline__ bf16x8 w4_expand(int d, unsigned mask, unsigned bias) {
  const unsigned u = (unsigned)d;
  const i32x4 v{(int)((u & mask) | bias), (int)(((u >> 4) & mask) | bias), (int)(((u >> 8) & mask) | bias),
                (int)(((u >> 12) & mask) | bias)};
  return __builtin_bit_cast(bf16x8, v);
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

}  // namespace w4
}  // namespace dsa
