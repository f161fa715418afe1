// The page walk shared by the paged-KV-cache attention kernels (paged_attn.hip: decode,
// paged_prefill.hip: prefill of new tokens over a cached prefix) and its MFMA operand helpers.
// Cache geometry: PAGE tokens per page, head_dim HDIM (see paged_attn.hip for the layouts).
#pragma once

#include "common.h"

#include <type_traits>

namespace dsa {
namespace paged {

constexpr int PAGE = 64;
constexpr int HDIM = 128;

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u2_t __attribute__((ext_vector_type(2)));
typedef unsigned short us4 __attribute__((ext_vector_type(4)));

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

// ------------------------------------------------------------------------------------------------
// One wave walks pages bt[p0 .. p1) (p0 < p1) of one block-table row for KV head `kvh` and folds
// them into the online-softmax state of NT tiles of 16 query columns: running max m (log2 domain),
// the lane's share of the sum l (the caller adds lanes qc, qc+16, qc+32, qc+48) and the
// unnormalised O^T accumulators acc, where lane (qc, g) holds O[column qc][16n + 4g + i].
//
//  * qf[c][kk]: the Q^T operand of tile c, lane (qc, g) holding q[column qc][32kk + 8g .. +8].
//    S^T = K Q^T puts 4 keys' scores of ONE column on a lane, so the softmax max and sum are 16
//    in-register ops plus two xor-shuffles.
//  * The 4 key tiles of a page are ordered (tile t, lane row r: key 32(t>>1) + 8(r>>2) + 4(t&1)
//    + (r&3)) so that the S^T accumulators, packed to bf16, are directly the B operand of
//    O^T += V^T P^T with the keys in natural order (element j of lane group g = key 32mm + 8g + j),
//    and the V^T operand is one 16-byte load of the dim-major V page.  These offsets are lane
//    constants; one page = 16 K + 16 V loads per lane, each converted once (FP8: from the raw
//    8 e4m3 bytes held in flight) and used by NT MFMAs.
//  * keep(c, key): whether column qc of tile c attends to `key`; the other scores become -inf.
//    A column's first page must keep at least one key, so its max is finite from there on.
//  * Two-stage software pipeline, pinned with sched_barrier: V(p) is in flight during
//    S(p) = K(p) Q^T, and K(p+1) during softmax + P V(p).  (Left alone, hipcc interleaved
//    load -> wait -> MFMA with <= 3 loads in flight, which made decode latency-bound at ~1.8 TB/s
//    instead of HBM-bound.)  The K load after the last page is a redundant reload of that page:
//    unconditional, so the vmcnt counting stays static.
// ------------------------------------------------------------------------------------------------
template <int NT, bool FP8, class Keep>
__device__ __forceinline__ void walk_pages(const void* k_cache, const void* v_cache, const int* bt, int p0, int p1,
                                           int KVH, int kvh, int lane, const bf16x8_t (&qf)[NT][4],
                                           float scale_log2, Keep keep, float (&m)[NT], float (&l)[NT],
                                           f32x4_t (&acc)[NT][8]) {
  using ElemT = typename std::conditional<FP8, unsigned char, bf16_t>::type;  // one cache value
  using OpT = typename std::conditional<FP8, u2_t, bf16x8_t>::type;           // 8 of them, in flight
  const int r = lane & 15, g = lane >> 4;
  int koff[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) koff[t] = (32 * (t >> 1) + 8 * (r >> 2) + 4 * (t & 1) + (r & 3)) * HDIM + 8 * g;
  const int voff = r * PAGE + 8 * g;
  OpT kf[4][4], vf[2][8];
  auto op = [](const OpT& v) -> bf16x8_t {
    if constexpr (FP8)
      return fp8x8_to_bf16(v);
    else
      return v;
  };
  auto load_k = [&](long page) {
    const ElemT* kb = (const ElemT*)k_cache + (page * KVH + kvh) * (long)(PAGE * HDIM);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) kf[t][kk] = *reinterpret_cast<const OpT*>(kb + koff[t] + 32 * kk);
  };
  auto load_v = [&](long page) {
    const ElemT* vb = (const ElemT*)v_cache + (page * KVH + kvh) * (long)(PAGE * HDIM);
#pragma unroll
    for (int mm = 0; mm < 2; ++mm)
#pragma unroll
      for (int n = 0; n < 8; ++n) vf[mm][n] = *reinterpret_cast<const OpT*>(vb + voff + 16 * n * PAGE + 32 * mm);
  };
  long page = bt[p0];
  load_k(page);
  for (int p = p0; p < p1; ++p) {
    const long next = p + 1 < p1 ? bt[p + 1] : page;
    load_v(page);
    __builtin_amdgcn_sched_barrier(0);
    // S^T tiles: lane holds keys 32(t>>1) + 8g + 4(t&1) + i, i = 0..3, of column qc of tile c
    f32x4_t s[NT][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int c = 0; c < NT; ++c) s[c][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const bf16x8_t kop = op(kf[t][kk]);
#pragma unroll
        for (int c = 0; c < NT; ++c) s[c][t] = mfma16(kop, qf[c][kk], s[c][t]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    load_k(next);
    __builtin_amdgcn_sched_barrier(0);
    page = next;
    const int base = p * PAGE;
    bf16x8_t pf[NT][2];
#pragma unroll
    for (int c = 0; c < NT; ++c) {
      float mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = base + 32 * (t >> 1) + 8 * g + 4 * (t & 1) + i;
          const float v = keep(c, key) ? s[c][t][i] * scale_log2 : -INFINITY;
          s[c][t][i] = v;
          mx = fmaxf(mx, v);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m[c], mx);
      const float alpha = fexp2(m[c] - mn);
      m[c] = mn;
      float ls = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float e = fexp2(s[c][t][i] - mn);
          s[c][t][i] = e;
          ls += e;
        }
      l[c] = l[c] * alpha + ls;
#pragma unroll
      for (int n = 0; n < 8; ++n) acc[c][n] *= alpha;
      // P^T operand of PV step mm: element j of lane group g = key 32mm + 8g + j
#pragma unroll
      for (int mm = 0; mm < 2; ++mm)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          pf[c][mm][i] = (__bf16)s[c][2 * mm][i];
          pf[c][mm][4 + i] = (__bf16)s[c][2 * mm + 1][i];
        }
    }
#pragma unroll
    for (int mm = 0; mm < 2; ++mm)
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const bf16x8_t vop = op(vf[mm][n]);
#pragma unroll
        for (int c = 0; c < NT; ++c) acc[c][n] = mfma16(vop, pf[c][mm], acc[c][n]);
      }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// lane group g's 4 x 8 values of one 128-wide bf16 output row: o[16n + 4g + i] = acc[n][i] * inv
__device__ __forceinline__ void store_o_bf16(bf16_t* o, const f32x4_t (&acc)[8], float inv, int g) {
#pragma unroll
  for (int n = 0; n < 8; ++n) {
    us4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = f2bf(acc[n][i] * inv);
    *reinterpret_cast<us4*>(o + 16 * n + 4 * g) = v;
  }
}

}  // namespace paged
}  // namespace dsa
