// What the weight-streaming decode GEMMs share (fp8_gemm.hip: fp8_stream_gemm with e4m3 weights,
// mxfp4.hip: mxfp4_gemm with FP4 weights; w4.hip: w4_gemm, bf16 MFMAs, takes the waits, the barrier, the
// stores and the reduce): fragment reads for v_mfma_scale_f32_16x16x128_f8f6f4
// from an LDS ring of 128-byte-row activation slots, a lane's accumulator holding 4 consecutive
// output columns of one token row, fp32 split-K partials [S][M][N] and their reduce.  Each file
// keeps its own swizzle, weight and scale loads and K-loop -- and its activation-offset loop, LDS-DMA
// issue and partial store: as helpers here, the offsets and the store reordered the scalar prologue of
// every mxfp4_gemm form, and the stream kernel's issue helper carries a tag per instantiation (below).
//
// Helpers are device functions, not lambdas, and each translation unit keeps one kernel template
// calling them: a lambda of a kernel template that uses these builtins made the host pass drop the
// template's launch stub (an undefined symbol at load time), and the host pass rejected a second
// kernel template calling an already-used device-function specialization ("substitution failure").
#pragma once

#include "mfma_tiles.h"

namespace dsa {
namespace stream {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

template <int N>
__device__ __forceinline__ void vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// a bare workgroup barrier: __syncthreads() is a release/acquire fence as well, for which the compiler
// drains vmcnt to 0 before the s_barrier -- every prefetch in flight would be waited for each step
__device__ __forceinline__ void barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// an 8-VGPR MFMA operand from its two 16-byte LDS pieces (two ds_read_b128)
__device__ __forceinline__ i32x8 frag(const char* p0, const char* p1) {
  const i32x4 a = *reinterpret_cast<const i32x4*>(p0);
  const i32x4 b = *reinterpret_cast<const i32x4*>(p1);
  return i32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// 4 consecutive output columns of one row, scaled by the row's xs (and the columns' ws) where there
// are such scales, and rounded to bf16: one 8-byte store
__device__ __forceinline__ void store_bf16x4(bf16_t* dst, const f32x4& v) {
  unsigned short o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e]);
  *reinterpret_cast<uint2*>(dst) =
      uint2{(unsigned)o[0] | ((unsigned)o[1] << 16), (unsigned)o[2] | ((unsigned)o[3] << 16)};
}
__device__ __forceinline__ void store_bf16x4(bf16_t* dst, const f32x4& v, float xs) {
  unsigned short o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e] * xs);
  *reinterpret_cast<uint2*>(dst) =
      uint2{(unsigned)o[0] | ((unsigned)o[1] << 16), (unsigned)o[2] | ((unsigned)o[3] << 16)};
}
__device__ __forceinline__ void store_bf16x4(bf16_t* dst, const f32x4& v, float xs, const f32x4& ws) {
  unsigned short o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = f2bf(v[e] * xs * ws[e]);
  *reinterpret_cast<uint2*>(dst) =
      uint2{(unsigned)o[0] | ((unsigned)o[1] << 16), (unsigned)o[2] | ((unsigned)o[3] << 16)};
}

// y[m][n] = bf16(xs[m] (ws[n]) sum_s part[s][m][n]) in the order s = 0, 1, .. (no atomics: a seeded
// request stays reproducible); 4 columns per thread.  WS: with per-column weight scales.  XS = false:
// without the per-row scales either (w4.hip: bf16 activations), xs and ws unused.
template <bool WS, bool XS = true>
__global__ __launch_bounds__(256) void reduce_kernel(const float* __restrict__ part, const float* __restrict__ xs,
                                                     const float* __restrict__ ws, bf16_t* __restrict__ Y, int M,
                                                     int N, long ldy, int S) {
  const long n4 = N / 4, total = (long)M * n4;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int m = (int)(i / n4), n = (int)(i % n4) * 4;
    f32x4 a = *reinterpret_cast<const f32x4*>(part + (long)m * N + n);
    for (int s2 = 1; s2 < S; ++s2) a += *reinterpret_cast<const f32x4*>(part + ((long)s2 * M + m) * N + n);
    if constexpr (!XS)
      store_bf16x4(Y + (long)m * ldy + n, a);
    else if constexpr (WS)
      store_bf16x4(Y + (long)m * ldy + n, a, xs[m], *reinterpret_cast<const f32x4*>(ws + n));
    else
      store_bf16x4(Y + (long)m * ldy + n, a, xs[m]);
  }
}

template <bool WS, bool XS = true>
inline hipError_t reduce(const float* part, const float* xs, const float* ws, void* Y, int M, int N, long ldy, int S,
                         hipStream_t st) {
  const long work = (long)M * (N / 4);
  const int g = (int)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096);
  reduce_kernel<WS, XS><<<g, 256, 0, st>>>(part, xs, ws, (bf16_t*)Y, M, N, ldy, S);
  return hipGetLastError();
}

}  // namespace stream
}  // namespace dsa
