// What the launch code of the routed expert GEMMs shares (moe.hip: moe_gemm, moe_w4.hip: moe_w4_gemm,
// moe_fine.hip: moe_fine_gemm): the form ladder, the check of the X operand, the rule for the K slices
// and the launch.  Host code only; each file includes it after its kernels' own headers.
#pragma once

#include "common.h"

namespace {

// 16-token blocks of the moe_gemm / moe_w4_gemm form that runs R rows: 1 (R <= 16), 2, 4, 8, 16
inline int moe_host_form(int R) { return R <= 16 ? 1 : R <= 32 ? 2 : R <= 64 ? 4 : R <= 128 ? 8 : 16; }

// X bf16 [xrows][K], row stride ldx elements: 16-byte rows, a row for every pair's p / src_div, all of it
// through a 32-bit buffer range
inline bool moe_host_x_ok(long ldx, int xrows, int src_div, int R, int k, int K) {
  return ldx % 8 == 0 && ldx >= K && src_div >= 1 && xrows >= 1 && (long)xrows * src_div >= (long)R * k &&
         ((long)(xrows - 1) * ldx + K) * 2 <= 0xffffffffL;
}

// K slices, from the shape alone (a launch inside a captured graph cannot look at the counts): the most,
// up to 16, that the K loop can run (`runs(S)`), that keep the grid of the experts that min(E, R k) pairs can
// reach (`wgs` workgroups over N each) within two workgroups per CU, and that keep the fp32 partials
// (written and read once) under a quarter of those experts' weight bytes, wnum / wden per weight:
// S * R k * N * 8 <= active * N * K * (wnum / wden) / 4
template <class Runs>
int moe_host_split(int R, int k, int E, int wgs, int K, long wnum, long wden, Runs runs) {
  const long active = (long)R * k < E ? (long)R * k : E;
  int best = 1;
  for (int s = 2; s <= 16; ++s)
    if (runs(s) && wgs * active * s <= 512 && (long)s * R * k * 32 * wden <= active * K * wnum) best = s;
  return best;
}

// KERNEL<<<grid, threads, LDS bytes of dynamic shared memory>>>(a); the kernel is allowed that much once
template <auto KERNEL, int LDS, class Args>
hipError_t moe_host_launch(dim3 grid, int threads, const Args& a, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    DSA_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
    attr = true;
  }
  KERNEL<<<grid, threads, LDS, st>>>(a);
  return hipGetLastError();
}

}  // namespace
