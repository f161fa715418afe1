// Batched multi-LoRA projections for the serving engine's decode step (gfx950): every row (token)
// of a batch names its adapter slot in idx[row], and the two kernels add the adapter's low-rank
// update to a base projection's output,  y[r] += (x[r] A[s]^T) B[s]^T,  s = idx[r].
//
// idx int32 [T]: -1 (or any value outside [0, S)) means no adapter -- the row's workgroups return
// before any other access and before any barrier, and nothing of the row is written.  The grids
// depend on T, the shapes and S only, never on the contents of idx; nothing is allocated or read
// back and there are no atomics, so both launches are hipGraph-capturable and bitwise reproducible.
//
// Stacked weights of one base projection:  A [S][L][K] bf16 (K contiguous),  B [S][N][R] bf16 (R
// contiguous), R the padded rank (8, 16, 32 or 64) and L = nsl * R: a fused base projection (wqkv,
// wgu) takes nsl independent LoRAs on one input, slice j owning columns slice_end[j-1] .. slice_end[j]
// of y and rows j R .. (j + 1) R of A.  alpha / r is folded into B when an adapter is loaded.
//
// shrink  t[r][j] = sum_k x[r][k] A[s][j][k]   fp32, not rounded to bf16
//   The guide's "GEMV / M <= 16" form of gemv.hip: 16-byte loads of A straight to VGPRs, fp32 FMAs,
//   wave_sum.  A workgroup (4 waves) owns 8 outputs of one row: the waves deal the 512-column steps
//   of K among themselves (wave w takes steps w, w + 4, ...: 8 loads of A and one of x in flight per
//   lane and step; a row of x is never held in registers), and their partial sums meet in LDS,
//   added in wave order.  Rows that share an adapter re-read A through L2.
// expand  y[r][n] = bf16(float(y[r][n]) + sum_i t[r][j R + i] B[s][n][i])   (n in slice j)
//   R / 8 lanes per output column, each with one 16-byte load of B (a wave's loads are contiguous);
//   the lanes' partial sums meet by __shfl_xor in a fixed order, all in fp32, one rounding.
#include "common.h"

using namespace dsa;

namespace {

constexpr int NT = 256;      // threads per workgroup (4 waves)
constexpr int JW = 8;        // outputs of t per shrink workgroup (L % 8 == 0)
constexpr int EXP_ITERS = 4; // column groups per expand workgroup

__global__ __launch_bounds__(NT) void lora_shrink_kernel(const bf16_t* __restrict__ x, long ldx,
                                                         const bf16_t* __restrict__ A,
                                                         const int* __restrict__ idx, float* __restrict__ t,
                                                         int S, int L, int K) {
  const int row = blockIdx.y;
  const int s = idx[row];
  if (s < 0 || s >= S) return;  // row-uniform: before any other access and any barrier
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = blockIdx.x * JW;
  const bf16_t* xr = x + (long)row * ldx;
  const bf16_t* a = A + ((long)s * L + j0) * K;
  float acc[JW];
#pragma unroll
  for (int j = 0; j < JW; ++j) acc[j] = 0.f;
  for (int k0 = wave * 512 + lane * 8; k0 < K; k0 += 4 * 512) {  // K % 8 == 0: a chunk is whole or absent
    us8 av[JW];
#pragma unroll
    for (int j = 0; j < JW; ++j) av[j] = *reinterpret_cast<const us8*>(a + (long)j * K + k0);
    float x8[8];
    unpack8(*reinterpret_cast<const us8*>(xr + k0), x8);
#pragma unroll
    for (int j = 0; j < JW; ++j) {
      float a8[8];
      unpack8(av[j], a8);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[j] = fmaf(a8[i], x8[i], acc[j]);
    }
  }
  __shared__ float part[4][JW];
#pragma unroll
  for (int j = 0; j < JW; ++j) {
    const float v = wave_sum(acc[j]);
    if (lane == 0) part[wave][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < JW) {
    const int j = threadIdx.x;
    t[(long)row * L + j0 + j] = ((part[0][j] + part[1][j]) + part[2][j]) + part[3][j];
  }
}

// e0 / e1: the ends of slices 0 and 1 (N where there is no such slice), so a column's slice is
// (n >= e0) + (n >= e1)
template <int R>
__global__ __launch_bounds__(NT) void lora_expand_kernel(const float* __restrict__ t, const bf16_t* __restrict__ B,
                                                         const int* __restrict__ idx, bf16_t* __restrict__ y,
                                                         long ldy, int S, int L, int N, int e0, int e1) {
  constexpr int LPC = R / 8;        // lanes per column
  constexpr int COLS = NT / LPC;    // columns per step of the workgroup
  const int row = blockIdx.y;
  const int s = idx[row];
  if (s < 0 || s >= S) return;  // row-uniform: before any other access and any barrier
  __shared__ float ts[3 * 64];
  for (int i = threadIdx.x; i < L; i += NT) ts[i] = t[(long)row * L + i];
  __syncthreads();
  const int sub = threadIdx.x % LPC, col = threadIdx.x / LPC;
  const bf16_t* b = B + (long)s * N * R;
  bf16_t* yr = y + (long)row * ldy;
  const int n0 = blockIdx.x * (COLS * EXP_ITERS) + col;
  us8 bv[EXP_ITERS];
#pragma unroll
  for (int it = 0; it < EXP_ITERS; ++it) {
    const int n = n0 + it * COLS;
    if (n < N) bv[it] = *reinterpret_cast<const us8*>(b + (long)n * R + sub * 8);
  }
#pragma unroll
  for (int it = 0; it < EXP_ITERS; ++it) {
    const int n = n0 + it * COLS;
    const bool live = n < N;  // (the shuffles below are executed by every lane of the wave)
    float acc = 0.f;
    if (live) {
      const int j = (n >= e0) + (n >= e1);
      const float* tj = ts + j * R + sub * 8;
      float b8[8];
      unpack8(bv[it], b8);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc = fmaf(tj[i], b8[i], acc);
    }
#pragma unroll
    for (int o = 1; o < LPC; o <<= 1) acc += __shfl_xor(acc, o, 64);
    if (live && sub == 0) yr[n] = f2bf(bf2f(yr[n]) + acc);
  }
}

bool rank_ok(int R) { return R == 8 || R == 16 || R == 32 || R == 64; }

}  // namespace

extern "C" bool dsa_lora_shrink_supported(int T, int S, int L, int K) {
  return T >= 1 && T <= 65535 && S >= 1 && L >= 8 && L % 8 == 0 && L <= 3 * 64 && K >= 8 && K % 8 == 0;
}

extern "C" bool dsa_lora_expand_supported(int T, int S, int nsl, int R, int N) {
  return T >= 1 && T <= 65535 && S >= 1 && nsl >= 1 && nsl <= 3 && rank_ok(R) && N >= 1;
}

// x [T][ldx] bf16 (16-byte aligned rows), A [S][L][K] bf16, idx [T], t [T][L] fp32
extern "C" hipError_t dsa_lora_shrink(const void* x, long ldx, const void* A, const int* idx, float* t, int T, int S,
                                      int L, int K, hipStream_t st) {
  if (T <= 0) return hipSuccess;
  if (!dsa_lora_shrink_supported(T, S, L, K) || ldx < K || ldx % 8) return hipErrorInvalidValue;
  lora_shrink_kernel<<<dim3(L / JW, T), NT, 0, st>>>((const bf16_t*)x, ldx, (const bf16_t*)A, idx, t, S, L, K);
  return hipGetLastError();
}

// t [T][nsl * R] fp32, B [S][N][R] bf16, idx [T], y [T][ldy] bf16 in place; slice_ends [nsl] ascending,
// slice_ends[nsl - 1] == N
extern "C" hipError_t dsa_lora_expand(const float* t, const void* B, const int* idx, void* y, long ldy, int T, int S,
                                      int nsl, int R, int N, const int* slice_ends, hipStream_t st) {
  if (T <= 0) return hipSuccess;
  if (!dsa_lora_expand_supported(T, S, nsl, R, N) || ldy < N) return hipErrorInvalidValue;
  int prev = 0;
  for (int j = 0; j < nsl; ++j) {
    if (slice_ends[j] <= prev) return hipErrorInvalidValue;
    prev = slice_ends[j];
  }
  if (prev != N) return hipErrorInvalidValue;
  const int e0 = nsl > 1 ? slice_ends[0] : N, e1 = nsl > 2 ? slice_ends[1] : N;
  const int L = nsl * R;
#define DSA_LORA_EXPAND(RR)                                                                             \
  lora_expand_kernel<RR><<<dim3((N + cols - 1) / cols, T), NT, 0, st>>>(t, (const bf16_t*)B, idx, (bf16_t*)y, ldy, \
                                                                        S, L, N, e0, e1)
  const int cols = NT / (R / 8) * EXP_ITERS;
  switch (R) {
    case 8: DSA_LORA_EXPAND(8); break;
    case 16: DSA_LORA_EXPAND(16); break;
    case 32: DSA_LORA_EXPAND(32); break;
    default: DSA_LORA_EXPAND(64); break;
  }
#undef DSA_LORA_EXPAND
  return hipGetLastError();
}
