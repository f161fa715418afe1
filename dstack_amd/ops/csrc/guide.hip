// Structured outputs for the serving engine (gfx950): the token mask of a byte-level DFA applied in
// place to bf16 logits [rows][V] (row stride `stride` elements, any value) between the penalties and
// the sampler.  No allocation, no host read-back and no atomics (hipGraph-capturable).
//
// A row names its grammar in `guide[row]` (-1: the row asks for nothing and is not touched) and its
// automaton state in `state[row]`.  Grammar g is trans[g] uint16 [STATES][256] and accept[g] uint8
// [STATES]; state 0 is dead (all its transitions lead to 0).  Token v is KEPT iff
//   * v is one of the first n_eos[0] ids of eos_ids and accept[g][s] is set, or
//   * v has at least one byte and walking its bytes from s through trans[g] never reaches state 0.
// Every other logit becomes bf16 -inf; kept logits are stored back bit for bit.  Token v's bytes are
// tok_bytes[tok_off[v] .. tok_off[v + 1]) for v < ntok; ids from ntok on have none.
//
// Grid (spans of SPAN elements, rows), as penalties.hip.  A wave owns 512 neighbouring tokens and
// visits them twice, in two layouts:
//   * the walk, 8 passes: lane l of pass j walks token base + 64 j + l.  Neighbouring lanes hold
//     neighbouring tokens, so their offsets are one coalesced read and their bytes a few cache lines
//     of the blob; the first byte of every token reads the same 512-byte row trans[g][s], later
//     bytes gather within the grammar's table (at most 2 MiB, inside one XCD's 4 MiB L2).  The
//     gathers are what the kernel waits for, and a gather costs by the cache lines it touches, so
//     the byte reads are kept dense and only the table reads scatter.  The 64 verdicts of a pass are
//     one wave ballot: 8 wave-uniform 64-bit masks per wave.
//   * the store: lane l owns the 16-byte logit vector of tokens base + 8 l .. 8 l + 7, whose verdicts
//     are byte l % 8 of mask l / 8.
//
// Nothing here trusts the tables: a guide or state out of range leaves the row alone, offsets are
// checked against the blob, and a transition that names a state >= STATES counts as dead.
#include "common.h"

using namespace dsa;

namespace {

constexpr int NT = 128;           // threads per workgroup: two waves
constexpr int WAVE = 64;
constexpr int PER_WAVE = WAVE * 8;  // tokens of a wave: one 16-byte logit vector per lane
constexpr int SPAN = NT * 8;      // elements of a row per workgroup
constexpr int STATES = 4096;      // rows of one grammar's transition table
constexpr int EOS_MAX = 8;        // EOS ids looked at
constexpr unsigned short NEG_INF = 0xFF80;  // bf16 -inf

__global__ __launch_bounds__(NT) void apply_guide_kernel(bf16_t* __restrict__ logits, long stride, int V,
                                                         const int* __restrict__ guide,
                                                         const int* __restrict__ state, int G,
                                                         const unsigned short* __restrict__ trans,
                                                         const unsigned char* __restrict__ accept,
                                                         const int* __restrict__ tok_off, int ntok,
                                                         const unsigned char* __restrict__ tok_bytes, int nbytes,
                                                         const int* __restrict__ eos_ids, int eos_cap,
                                                         const int* __restrict__ n_eos) {
  const int row = blockIdx.y, lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int g = guide[row];
  if (g < 0 || g >= G) return;  // row-uniform, before any other access
  const int s = state[row];
  if (s < 0 || s >= STATES) return;
  const unsigned short* T = trans + (long)g * STATES * 256;
  const bool acc = accept[(long)g * STATES + s] != 0;
  const int ne = acc ? max(0, min(min(n_eos[0], eos_cap), EOS_MAX)) : 0;
  int eos[EOS_MAX];
#pragma unroll
  for (int e = 0; e < EOS_MAX; ++e) eos[e] = e < ne ? eos_ids[e] : -1;

  const int hi = min(V, (int)(blockIdx.x + 1) * SPAN);
  const int base = blockIdx.x * SPAN + wave * PER_WAVE;  // wave-uniform
  if (base >= hi) return;

  // the walk: mask[j] bit l = token base + 64 j + l is kept
  unsigned long long mask[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int v = base + j * WAVE + lane;
    bool keep = false;
    if (v < hi) {
#pragma unroll
      for (int e = 0; e < EOS_MAX; ++e) keep |= eos[e] == v;  // (unused entries are -1)
      if (!keep && v < ntok) {
        const int b0 = tok_off[v], b1 = tok_off[v + 1];
        if (b0 >= 0 && b1 > b0 && b1 <= nbytes) {  // no bytes (or a broken table): never kept by its bytes
          int cur = s;
          for (int i = b0; i < b1 && cur != 0; ++i) {
            cur = T[cur * 256 + tok_bytes[i]];
            if (cur >= STATES) cur = 0;
          }
          keep = cur != 0;
        }
      }
    }
    mask[j] = __ballot(keep);
  }

  // the store: 16-byte accesses when the row starts on 16 bytes, else element by element (an odd row
  // stride, a column slice) -- and for the tail of the row
  unsigned long long m = mask[0];
#pragma unroll
  for (int j = 1; j < 8; ++j) m = (lane >> 3) == j ? mask[j] : m;
  const unsigned kept = (unsigned)(m >> ((lane & 7) * 8)) & 0xFFu;
  const int i0 = base + lane * 8, n = min(8, hi - i0);
  if (n <= 0) return;
  unsigned short* x = reinterpret_cast<unsigned short*>(logits + (long)row * stride);
  const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  if (aligned && n == 8) {
    us8 u = *reinterpret_cast<const us8*>(x + i0);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (!(kept >> k & 1u)) u[k] = NEG_INF;
    *reinterpret_cast<us8*>(x + i0) = u;
  } else {
    for (int k = 0; k < n; ++k)
      if (!(kept >> k & 1u)) x[i0 + k] = NEG_INF;
  }
}

}  // namespace

extern "C" int dsa_guide_max_states() { return STATES; }

extern "C" hipError_t dsa_apply_guide(void* logits, long stride, int rows, int V, const int* guide, const int* state,
                                      int G, const void* trans, const void* accept, const int* tok_off, int ntok,
                                      const void* tok_bytes, int nbytes, const int* eos_ids, int eos_cap,
                                      const int* n_eos, hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  if (V < 1 || G < 1 || rows > 65535 || ntok < 0 || nbytes < 0 || eos_cap < 0) return hipErrorInvalidValue;
  const dim3 grid((V + SPAN - 1) / SPAN, rows);
  apply_guide_kernel<<<grid, NT, 0, st>>>((bf16_t*)logits, stride, V, guide, state, G, (const unsigned short*)trans,
                                          (const unsigned char*)accept, tok_off, ntok,
                                          (const unsigned char*)tok_bytes, nbytes, eos_ids, eos_cap, n_eos);
  return hipGetLastError();
}
