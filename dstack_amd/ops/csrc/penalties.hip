// Sampling penalties for the serving engine (gfx950): presence / frequency / repetition penalties
// and logit_bias applied in place to bf16 logits [rows][V] (row stride `stride` elements, any
// value) in front of the sampler, and the per-sequence token state the penalties read.  No
// allocation, no host read-back and no atomics (hipGraph-capturable).
//
// State: int32 [slots][V], state[s][v] = 2 * c[v] + in_prompt[v] with c[v] the number of times the
// sequence in slot s has generated token v and in_prompt[v] whether v occurs in its prompt.  A row
// names its slot in `slot[row]`; -1 means the row asks for nothing and is not touched.
//
// Per element, in fp32, every step one correctly rounded operation (contraction is off for this
// file: hipcc would otherwise fuse x - f * c into an FMA and change bits):
//   1. repetition (r != 1 and state != 0):  x = x > 0 ? x * inv_r : x * r     (inv_r = fp32(1 / r), host)
//   2. frequency:                           x = x - f * float(c)
//   3. presence (c > 0):                    x = x - p
//   4. bias (ids of the slot's list only):  x = x + bias
//   5. one rounding to bf16 (nearest even).  -inf stays -inf through all of it.
//
// Grid (spans of SPAN elements, rows): a streaming pass, 2 B + 4 B read and 2 B written per element.
// The bias list is sparse (at most MAXB ids per slot): the workgroup that owns a span first computes
// steps 1-5 for the listed ids inside its span from the RAW logits into registers (MAXB <= 2 * NT:
// two entries per thread), runs the dense pass, and after a barrier overwrites the listed ids, so
// they are rounded once like every other element.
#include "common.h"

#pragma clang fp contract(off)

using namespace dsa;

namespace {

constexpr int NT = 256;          // threads per workgroup
constexpr int SPAN = NT * 8 * 2; // elements of a row per workgroup: two 16-byte vectors per thread
constexpr int MAXB = 300;        // logit_bias entries per slot
constexpr int BPT = (MAXB + NT - 1) / NT;

typedef int i4 __attribute__((ext_vector_type(4)));

// steps 1-3 for one element with state word s
__device__ __forceinline__ float penalise(float x, int s, float r, float inv_r, float f, float p) {
  const int c = s >> 1;
  if (r != 1.f && s != 0) x = x > 0.f ? x * inv_r : x * r;
  const float m = f * (float)c;
  x = x - m;
  if (c > 0) x = x - p;
  return x;
}

__global__ __launch_bounds__(NT) void apply_penalties_kernel(bf16_t* __restrict__ logits, long stride, int V,
                                                             const int* __restrict__ state, int slots,
                                                             const int* __restrict__ slot,
                                                             const float* __restrict__ rep,
                                                             const float* __restrict__ inv_rep,
                                                             const float* __restrict__ freq,
                                                             const float* __restrict__ pres,
                                                             const int* __restrict__ bias_ids,
                                                             const float* __restrict__ bias_vals,
                                                             const int* __restrict__ bias_n) {
  const int row = blockIdx.y, tid = threadIdx.x;
  const int s = slot[row];
  if (s < 0 || s >= slots) return;  // row-uniform, before any other access and any barrier
  const float r = rep[row], inv_r = inv_rep[row], f = freq[row], p = pres[row];
  const int lo = blockIdx.x * SPAN, hi = min(V, lo + SPAN);
  bf16_t* x = logits + (long)row * stride;
  const int* st = state + (long)s * V;
  const int nb = max(0, min(bias_n[s], MAXB));  // block-uniform

  // the listed ids of this span, from the raw logits
  int bid[BPT];
  bf16_t bout[BPT];
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    bid[j] = -1;
    bout[j] = 0;
    const int e = tid + j * NT;
    if (e < nb) {
      const int id = bias_ids[(long)s * MAXB + e];
      if (id >= lo && id < hi) {
        bid[j] = id;
        bout[j] = f2bf(penalise(bf2f(x[id]), st[id], r, inv_r, f, p) + bias_vals[(long)s * MAXB + e]);
      }
    }
  }
  if (nb > 0) __syncthreads();

  // dense pass: 16-byte accesses when both rows start on 16 bytes, else element by element (an odd
  // row stride, a column slice, V % 4 != 0 for the state)
  const bool aligned = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(st)) & 15) == 0;
  for (int i0 = lo + tid * 8; i0 < hi; i0 += NT * 8) {
    if (aligned && i0 + 8 <= hi) {
      const us8 u = *reinterpret_cast<const us8*>(x + i0);
      const i4 a = *reinterpret_cast<const i4*>(st + i0);
      const i4 b = *reinterpret_cast<const i4*>(st + i0 + 4);
      us8 o;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o[k] = f2bf(penalise(bf2f((bf16_t)u[k]), a[k], r, inv_r, f, p));
        o[k + 4] = f2bf(penalise(bf2f((bf16_t)u[k + 4]), b[k], r, inv_r, f, p));
      }
      *reinterpret_cast<us8*>(x + i0) = o;
    } else {
      for (int k = 0; k < 8 && i0 + k < hi; ++k) x[i0 + k] = f2bf(penalise(bf2f(x[i0 + k]), st[i0 + k], r, inv_r, f, p));
    }
  }

  if (nb > 0) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < BPT; ++j)
      if (bid[j] >= 0) x[bid[j]] = bout[j];
  }
}

// state[slot[row]][tokens[row]] += 2 for the rows with a slot: slots are unique among the rows of a
// step, so a plain load and store suffice.
__global__ void penalties_update_kernel(int* __restrict__ state, int slots, int V, const int* __restrict__ slot,
                                        const int* __restrict__ tokens, int rows) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const int s = slot[row];
  if (s < 0 || s >= slots) return;
  const int t = tokens[row];
  if (t < 0 || t >= V) return;
  int* w = state + (long)s * V + t;
  *w = *w + 2;
}

}  // namespace

extern "C" int dsa_logit_bias_max() { return MAXB; }

extern "C" hipError_t dsa_apply_penalties(void* logits, long stride, int rows, int V, const int* state, int slots,
                                          const int* slot, const float* rep, const float* inv_rep,
                                          const float* freq, const float* pres, const int* bias_ids,
                                          const float* bias_vals, const int* bias_n, hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  if (V < 1 || slots < 1 || rows > 65535) return hipErrorInvalidValue;
  const dim3 grid((V + SPAN - 1) / SPAN, rows);
  apply_penalties_kernel<<<grid, NT, 0, st>>>((bf16_t*)logits, stride, V, state, slots, slot, rep, inv_rep, freq,
                                              pres, bias_ids, bias_vals, bias_n);
  return hipGetLastError();
}

extern "C" hipError_t dsa_penalties_update(int* state, int slots, int V, const int* slot, const int* tokens,
                                           int rows, hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  if (V < 1 || slots < 1) return hipErrorInvalidValue;
  penalties_update_kernel<<<(rows + 63) / 64, 64, 0, st>>>(state, slots, V, slot, tokens, rows);
  return hipGetLastError();
}
