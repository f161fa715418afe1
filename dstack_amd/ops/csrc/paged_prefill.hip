// Paged-prefix prefill attention for CDNA4 / gfx950: causal GQA attention (head_dim 128) of a
// chunk of NEW query tokens over the paged KV cache.  Used by the serving engine's automatic
// prefix caching: a prompt whose first `start` tokens are already cached computes only the rest,
// and those rows attend to keys 0 .. start + i through the sequence's block table.  All K and V
// come from the cache, the chunk's own tokens included (rope_cache_write has stored them on the
// same stream), so there is one operand path and `start` need not be a page multiple.
//
// The MFMA operand scheme and the page walk are shared with the decode kernel (paged_frag.h:
// walk_pages; S^T = K Q^T, O^T += V^T P^T, every operand one 16-byte load of the cache, no LDS),
// with the 16 query columns of a tile being 16 consecutive tokens of ONE query head instead of the
// <= 16 heads of one token:
//
//  * one wave = (segment, NT column tiles = 16 NT consecutive tokens, one query head): every K
//    and V fragment it loads is used by NT MFMAs -- the decode form would re-read the prefix once
//    per 16 tokens per head.  NT = 3: the most that fits the 512 registers of a wave without
//    spilling (NT = 4 spills 106 VGPRs with a bf16 cache), 1.33x the speed of NT = 2 at 512 new
//    tokens over 1536 cached ones (Llama-3-8B heads; tools/bench_paged_prefill.py);
//  * the waves of a workgroup (up to 4, one per SIMD) are the query heads that share the KV head
//    over the same tokens, so their page loads coincide in L1/L2 (G > 4: G / 4 such workgroups);
//  * the mask is per column: key <= start + i; a column at or past the segment's length has a
//    zero operand and is not stored; a tile's page loop ends at the page of its last valid row;
//  * the grid (tiles of the longest segment, KV heads x head groups, segments) is sized by the
//    host from the plan's lengths: prefill steps run eagerly, never from a captured graph.  Long
//    tiles (late tokens: most pages) are dealt first.
#include "common.h"
#include "paged_frag.h"

using namespace dsa;
using namespace dsa::paged;

namespace {

constexpr int NT = 3;            // column tiles (16 tokens each) per wave
constexpr int TOK = 16 * NT;     // query tokens per wave / workgroup
constexpr int MAX_WAVES = 4;     // query heads per workgroup

}  // namespace

// q row r is at q + r * q_stride with its H heads contiguous (the fused qkv output, read in
// place); out[r][h*128 + d] bf16, written for rows seg_offsets[s] + i, i < seg_lens[s], only.
// FP8: e4m3 cache; k_scale is folded into scale_log2 by the host, v_scale into the output.
template <bool FP8>
__global__ __launch_bounds__(64 * MAX_WAVES) void paged_prefill_kernel(
    const bf16_t* __restrict__ q, long q_stride, long rows, const void* __restrict__ k_cache,
    const void* __restrict__ v_cache, const int* __restrict__ block_tables, int bt_stride, int bt_width,
    const int* __restrict__ seg_offsets, const int* __restrict__ seg_starts, const int* __restrict__ seg_lens,
    bf16_t* __restrict__ out, int H, int KVH, int G, int hgroups, float scale_log2, float v_scale) {
  const int seg = blockIdx.z;
  const int kvh = blockIdx.y / hgroups, hg = blockIdx.y % hgroups;
  const int tile = gridDim.x - 1 - blockIdx.x;  // most pages first
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, qc = lane & 15, g = lane >> 4;
  const int hq = hg * MAX_WAVES + wave;  // query head within the KV head's group
  const int len = seg_lens[seg], start = seg_starts[seg];
  const int i0 = tile * TOK;
  if (i0 >= len || hq >= G || start < 0) return;  // (wave-uniform; the kernel has no barrier)
  const int h = kvh * G + hq;
  const long row0 = (long)seg_offsets[seg] + i0;

  // column c of the wave: token i0 + 16c + qc at position start + i0 + 16c + qc
  bool valid[NT];
  int limit[NT];  // last key the column attends to
#pragma unroll
  for (int c = 0; c < NT; ++c) {
    const int i = i0 + 16 * c + qc;
    const long row = row0 + 16 * c + qc;
    valid[c] = i < len && row >= 0 && row < rows;
    limit[c] = start + i;
  }
  const int last = start + min(i0 + TOK, len) - 1;  // position of the tile's last valid row
  const int p1 = min(last / PAGE + 1, bt_width);     // (the host checks the table covers it)

  float m[NT], l[NT];
  f32x4_t acc[NT][8];
#pragma unroll
  for (int c = 0; c < NT; ++c) {
    m[c] = -INFINITY;
    l[c] = 0.f;
#pragma unroll
    for (int n = 0; n < 8; ++n) acc[c][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  // Q^T operand: lane (qc, g) holds q[token][h][32kk + 8g .. +8] for k-step kk
  bf16x8_t qf[NT][4];
#pragma unroll
  for (int c = 0; c < NT; ++c) {
    const bf16_t* qrow = q + (valid[c] ? row0 + 16 * c + qc : 0L) * q_stride + (long)h * HDIM;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      qf[c][kk] = valid[c] ? ld8(qrow + 32 * kk + 8 * g) : bf16x8_t{};
    }
  }
  // each K and V fragment of a page feeds NT MFMAs; column c attends to keys 0 .. limit[c]
  walk_pages<NT, FP8>(k_cache, v_cache, block_tables + (long)seg * bt_stride, 0, p1, KVH, kvh, lane, qf, scale_log2,
                      [&](int c, int key) { return key <= limit[c]; }, m, l, acc);
  // O^T accumulator: lane (qc, g) holds O[token][h][16n + 4g + i]
#pragma unroll
  for (int c = 0; c < NT; ++c) {
    float lc = l[c];
    lc += __shfl_xor(lc, 16, 64);
    lc += __shfl_xor(lc, 32, 64);
    if (!valid[c]) continue;
    const float inv = lc > 0.f ? v_scale / lc : 0.f;
    store_o_bf16(out + (row0 + 16 * c + qc) * ((long)H * HDIM) + (long)h * HDIM, acc[c], inv, g);
  }
}

// ------------------------------------------------------------------------------------------------
extern "C" int dsa_paged_prefill_tile() { return TOK; }

// n segments; max_len = the longest seg_lens entry (host-side knowledge: it sizes the grid);
// rows = rows of q and out (a row outside [0, rows) is neither read nor written)
extern "C" hipError_t dsa_paged_prefill(const void* q, long q_stride, long rows, const void* k_cache,
                                        const void* v_cache, const int* block_tables, int bt_stride, int bt_width,
                                        const int* seg_offsets, const int* seg_starts, const int* seg_lens,
                                        void* out, int n, int max_len, int H, int KVH, float scale, int fp8,
                                        float k_scale, float v_scale, hipStream_t st) {
  if (n <= 0 || max_len <= 0) return hipSuccess;
  if (KVH <= 0 || H % KVH || H / KVH > 16 || bt_width < 1 || n > 65535) return hipErrorInvalidValue;
  const int G = H / KVH;
  const int waves = G < MAX_WAVES ? G : MAX_WAVES;
  const int hgroups = (G + MAX_WAVES - 1) / MAX_WAVES;
  if ((long)KVH * hgroups > 65535) return hipErrorInvalidValue;
  const float sl2 = scale * 1.4426950408889634f * (fp8 ? k_scale : 1.f);
  const float vs = fp8 ? v_scale : 1.f;
  const dim3 grid((max_len + TOK - 1) / TOK, KVH * hgroups, n);
  if (fp8)
    paged_prefill_kernel<true><<<grid, 64 * waves, 0, st>>>((const bf16_t*)q, q_stride, rows, k_cache, v_cache,
                                                            block_tables, bt_stride, bt_width, seg_offsets,
                                                            seg_starts, seg_lens, (bf16_t*)out, H, KVH, G, hgroups,
                                                            sl2, vs);
  else
    paged_prefill_kernel<false><<<grid, 64 * waves, 0, st>>>((const bf16_t*)q, q_stride, rows, k_cache, v_cache,
                                                             block_tables, bt_stride, bt_width, seg_offsets,
                                                             seg_starts, seg_lens, (bf16_t*)out, H, KVH, G, hgroups,
                                                             sl2, vs);
  return hipGetLastError();
}
