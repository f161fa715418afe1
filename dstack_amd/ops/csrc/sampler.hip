// Truncated sampling for the serving engine (gfx950): top-k / top-p / min-p thresholds, the masked
// Gumbel-max draw and the top-N log-probabilities, all per row of bf16 logits [rows][V] (row stride
// `stride` elements, any value), one 256-thread workgroup per row, no allocation and no host
// read-back (hipGraph-capturable).
//
// Every truncation is a threshold on the logit VALUE: the kept set of a row is {x >= tau}, so equal
// logits are kept or dropped together.  A bf16 logit has one of 65536 bit patterns; a monotone 16-bit
// key of the pattern turns "the k-th largest value" and "the value where the cumulative mass crosses
// p" into a search over a two-level histogram (the key's high 12 bits, then the low 4 bits inside
// the crossing bin) -- no sort.  Masses are summed as 64-bit fixed point (w = exp(z - zmax) in
// (0, 1], scaled by 2^40), so the sums do not depend on the order the atomics arrive in and a seeded
// request is reproducible.
//
//   z = x * invT, invT = 1/T for T > 0 else 1 (the greedy convention of sample_kernel).
//   top-k (0 < k < V): keep v iff fewer than k finite tokens are strictly greater than v.
//   top-p (p < 1), on the survivors of top-k: keep v iff the mass of survivors strictly greater
//       than v is at most p times the survivors' total mass.
//   min-p (min_p > 0): keep v iff z >= zmax + ln(min_p).
//   Each active rule gives the smallest value of the row it keeps; tau is the largest of them and
//   -inf when no rule is active.  -inf logits are never counted and never kept.
#include "common.h"

using namespace dsa;

namespace {

constexpr int NT = 256;            // threads per workgroup
constexpr int L2B = 4;             // low key bits resolved by the second level
constexpr int NB1 = 1 << (16 - L2B);  // first-level bins (sign, exponent, 3 mantissa bits)
constexpr int NB2 = 1 << L2B;
constexpr int BPT = NB1 / NT;      // first-level bins searched per thread
constexpr int MAXN = 20;           // top_logprobs cap
constexpr bf16_t NEG_INF = 0xFF80;
constexpr float MASS_ONE = 1099511627776.f;  // 2^40

typedef unsigned long long u64;

// Monotone key: a larger float has a larger key; -0 shares +0's key (equal values, one threshold).
__device__ __forceinline__ uint32_t key_of(bf16_t u) {
  if (u == 0x8000) u = 0;
  return (u & 0x8000) ? (uint32_t)(uint16_t)~u : (uint32_t)(u | 0x8000);
}
__device__ __forceinline__ float val_of(uint32_t key) {
  return bf2f((key & 0x8000) ? (bf16_t)(key & 0x7FFF) : (bf16_t)(~key & 0xFFFF));
}

// f(index, raw bf16) for every element of the row, each thread in ascending index order.  A row
// that does not start on 16 bytes (an odd row stride, a column slice) is read with 2-byte loads:
// that path is there for correctness and was not tuned; the engine's logits rows are aligned.
template <typename F>
__device__ __forceinline__ void for_each(const bf16_t* __restrict__ x, int V, int tid, F&& f) {
  const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  for (int i0 = tid * 8; i0 < V; i0 += NT * 8) {
    if (aligned && i0 + 8 <= V) {
      const us8 u = *reinterpret_cast<const us8*>(x + i0);
#pragma unroll
      for (int k = 0; k < 8; ++k) f(i0 + k, (bf16_t)u[k]);
    } else {
      for (int k = 0; k < 8 && i0 + k < V; ++k) f(i0 + k, x[i0 + k]);
    }
  }
}

// Sum of `v` over the threads above this one: a suffix scan inside each wave, then the totals of
// the waves above (`sh`: one entry per wave; ends with a barrier, so `sh` may be reused).  Integer
// adds only, so the result does not depend on the order.
template <typename T>
__device__ __forceinline__ T sum_above(T v, T* sh, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  T s = v;  // inclusive suffix sum over the lanes of this wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_down(s, o, 64);
    if (lane + o < 64) s += t;
  }
  if (lane == 0) sh[wave] = s;
  __syncthreads();
  T above = s - v;
  for (int j = wave + 1; j < NT / 64; ++j) above += sh[j];
  __syncthreads();
  return above;
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

// ------------------------------------------------------------------------------------------------
// tau [rows]
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void threshold_kernel(const bf16_t* __restrict__ logits, long stride, int V,
                                                       const float* __restrict__ temps,
                                                       const int* __restrict__ top_k,
                                                       const float* __restrict__ top_p,
                                                       const float* __restrict__ min_p,
                                                       float* __restrict__ tau) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const int k = top_k[row];
  const float p = fmaxf(top_p[row], 0.f), mp = min_p[row];
  const bool want_k = k > 0 && k < V, want_p = p < 1.f, want_m = mp > 0.f;
  if (!(want_k || want_p || want_m)) {  // row-uniform, before any barrier
    if (tid == 0) tau[row] = -INFINITY;
    return;
  }
  __shared__ uint32_t cnt1[NB1];
  __shared__ u64 mass1[NB1];
  __shared__ uint32_t cnt2[NB2];
  __shared__ u64 mass2[NB2];
  __shared__ u64 sh_m[NT / 64];
  __shared__ uint32_t sh_c[NT / 64];
  __shared__ uint32_t s_kmax, s_kminp, s_keyk, s_keyp;
  __shared__ int s_bin;
  __shared__ uint32_t s_cabove;
  __shared__ u64 s_mabove, s_total;

  const bf16_t* x = logits + (long)row * stride;
  const float T = temps[row];
  const float invT = T > 0.f ? 1.f / T : 1.f;

  for (int b = tid; b < NB1; b += NT) {
    cnt1[b] = 0;
    mass1[b] = 0;
  }
  if (tid == 0) {
    s_kmax = 0;
    s_kminp = 0xFFFFu;
  }
  __syncthreads();

  // pass 0: the row maximum
  uint32_t kmax = 0;
  for_each(x, V, tid, [&](int, bf16_t u) {
    if (u != NEG_INF) kmax = max(kmax, key_of(u));
  });
  atomicMax(&s_kmax, kmax);
  __syncthreads();
  kmax = s_kmax;
  if (kmax == 0) {  // no finite logit (block-uniform)
    if (tid == 0) tau[row] = -INFINITY;
    return;
  }
  const float zmax = val_of(kmax) * invT;
  const float zthr = want_m ? zmax + logf(mp) : 0.f;

  // pass 1: first-level histogram of counts and masses, and the smallest key min-p keeps
  uint32_t kminp = kmax;
  const bool hist = want_k || want_p;
  for_each(x, V, tid, [&](int, bf16_t u) {
    if (u == NEG_INF) return;
    const uint32_t key = key_of(u);
    const float z = bf2f(u) * invT;
    if (want_m && z >= zthr) kminp = min(kminp, key);
    if (hist) {
      atomicAdd(&cnt1[key >> L2B], 1u);
      atomicAdd(&mass1[key >> L2B], (u64)(__expf(z - zmax) * MASS_ONE));
    }
  });
  if (want_m) atomicMin(&s_kminp, kminp);
  __syncthreads();
  uint32_t tkey = want_m ? s_kminp : 0u;

  if (hist) {
    // per-thread totals of its BPT bins and the totals of the bins above them
    uint32_t c_loc = 0;
    u64 m_loc = 0;
    for (int b = tid * BPT; b < tid * BPT + BPT; ++b) {
      c_loc += cnt1[b];
      m_loc += mass1[b];
    }
    const uint32_t c_above = sum_above(c_loc, sh_c, tid);
    const u64 m_above = sum_above(m_loc, sh_m, tid);
    if (tid == 0) {
      s_total = m_above + m_loc;
      s_bin = NB1;
    }
    __syncthreads();

    // second level of bin B (elements whose key lies in it)
    auto level2 = [&](int B) {
      if (tid < NB2) {
        cnt2[tid] = 0;
        mass2[tid] = 0;
      }
      __syncthreads();
      for_each(x, V, tid, [&](int, bf16_t u) {
        if (u == NEG_INF) return;
        const uint32_t key = key_of(u);
        if ((int)(key >> L2B) != B) return;
        atomicAdd(&cnt2[key & (NB2 - 1)], 1u);
        atomicAdd(&mass2[key & (NB2 - 1)], (u64)(__expf(bf2f(u) * invT - zmax) * MASS_ONE));
      });
      __syncthreads();
    };
    // the owner of bin B publishes the count and mass of the bins above B
    auto publish_above = [&](int B) {
      if (tid == B / BPT) {
        uint32_t c = c_above;
        u64 m = m_above;
        for (int b = tid * BPT + BPT - 1; b > B; --b) {
          c += cnt1[b];
          m += mass1[b];
        }
        s_cabove = c;
        s_mabove = m;
      }
      __syncthreads();
    };

    int Bk = -1;  // first-level bin of the top-k threshold (its second level is in cnt2 / mass2)
    uint32_t keyk = 0;
    u64 S = s_total;
    if (want_k) {
      // the lowest non-empty bin with fewer than k tokens above it
      int cand = NB1;
      uint32_t g = c_above;
      for (int b = tid * BPT + BPT - 1; b >= tid * BPT; --b) {
        if (cnt1[b] > 0 && g < (uint32_t)k) cand = b;
        g += cnt1[b];
      }
      if (cand < NB1) atomicMin(&s_bin, cand);
      __syncthreads();
      Bk = s_bin;  // exists: the bin of the maximum has nothing above it
      publish_above(Bk);
      level2(Bk);
      if (tid == 0) {
        uint32_t g2 = s_cabove;
        int sel = NB2 - 1;
        for (int s = NB2 - 1; s >= 0; --s) {
          if (cnt2[s] > 0 && g2 < (uint32_t)k) sel = s;
          g2 += cnt2[s];
        }
        u64 m = s_mabove;
        for (int s = NB2 - 1; s >= sel; --s) m += mass2[s];
        s_keyk = ((uint32_t)Bk << L2B) | (uint32_t)sel;
        s_total = m;   // the survivors' mass
        s_bin = NB1;
      }
      __syncthreads();
      keyk = s_keyk;
      S = s_total;
      tkey = max(tkey, keyk);
    }
    if (want_p) {
      const double lim = (double)p * (double)S;
      const int lo = want_k ? Bk : 0;
      int cand = NB1;
      u64 g = m_above;
      for (int b = tid * BPT + BPT - 1; b >= tid * BPT && b >= lo; --b) {
        if (cnt1[b] > 0 && (double)g <= lim) cand = b;
        g += mass1[b];
      }
      if (cand < NB1) atomicMin(&s_bin, cand);
      __syncthreads();
      const int Bp = s_bin;  // exists: the bin of the maximum has no mass above it
      publish_above(Bp);
      if (Bp != Bk) level2(Bp);
      if (tid == 0) {
        u64 g2 = s_mabove;
        uint32_t sel = kmax;
        for (int s = NB2 - 1; s >= 0; --s) {
          const uint32_t key = ((uint32_t)Bp << L2B) | (uint32_t)s;
          if (key < keyk) break;
          if (cnt2[s] > 0 && (double)g2 <= lim) sel = key;
          g2 += mass2[s];
        }
        s_keyp = sel;
      }
      __syncthreads();
      tkey = max(tkey, s_keyp);
    }
  }
  if (tid == 0) tau[row] = tkey ? val_of(tkey) : -INFINITY;
}

// ------------------------------------------------------------------------------------------------
// sample_kernel's pass over the kept set {x >= tau}: the same hash, the same Gumbel noise per
// (seed, step, index), the same tie-break on the lower index and the same reduction order, so
// tau = -inf returns what sample_kernel returns.  The log-probability is under the kept set.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void sample_masked_kernel(const bf16_t* __restrict__ logits, long stride, int V,
                                                           const float* __restrict__ temps,
                                                           const int64_t* __restrict__ seeds,
                                                           const int* __restrict__ steps,
                                                           const float* __restrict__ tau,
                                                           int* __restrict__ tokens,
                                                           float* __restrict__ logprobs) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const bf16_t* x = logits + (long)row * stride;
  const float T = temps[row];
  const bool greedy = !(T > 0.f);
  const float invT = greedy ? 1.f : 1.f / T;
  const float tv = tau[row];
  const uint64_t key = mix64((uint64_t)seeds[row] * 0x9e3779b97f4a7c15ULL + (uint64_t)steps[row]);
  float best = -INFINITY, mx = -INFINITY, sum = 0.f, bestx = -INFINITY;
  int bi = 0x7fffffff;
  for_each(x, V, tid, [&](int i, bf16_t u) {
    const float xv = bf2f(u);
    if (xv < tv) return;  // truncated
    const float z = xv * invT;
    if (z == -INFINITY) return;  // masked logit (e.g. a banned token)
    if (z > mx) {
      sum = sum * __expf(mx - z) + 1.f;
      mx = z;
    } else {
      sum += __expf(z - mx);
    }
    float score = z;
    if (!greedy) {
      const uint64_t hsh = mix64(key ^ ((uint64_t)i * 0xd1b54a32d192ed03ULL));
      const float un = ((float)(hsh >> 40) + 0.5f) * (1.0f / 16777216.0f);
      score = z - __logf(-__logf(un));
    }
    if (score > best || (score == best && i < bi)) {
      best = score;
      bi = i;
      bestx = z;
    }
  });
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    const float ox = __shfl_xor(bestx, o, 64);
    if (ob > best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
      bestx = ox;
    }
    const float om = __shfl_xor(mx, o, 64), os = __shfl_xor(sum, o, 64);
    const float nm = fmaxf(mx, om);
    sum = (mx > -INFINITY ? sum * __expf(mx - nm) : 0.f) + (om > -INFINITY ? os * __expf(om - nm) : 0.f);
    mx = nm;
  }
  __shared__ float sb[4], sx[4], sm[4], ss[4];
  __shared__ int si[4];
  const int w = tid >> 6;
  if ((tid & 63) == 0) {
    sb[w] = best;
    si[w] = bi;
    sx[w] = bestx;
    sm[w] = mx;
    ss[w] = sum;
  }
  __syncthreads();
  if (tid == 0) {
    for (int j = 1; j < 4; ++j) {
      if (sb[j] > best || (sb[j] == best && si[j] < bi)) {
        best = sb[j];
        bi = si[j];
        bestx = sx[j];
      }
      const float nm = fmaxf(mx, sm[j]);
      sum = (mx > -INFINITY ? sum * __expf(mx - nm) : 0.f) + (sm[j] > -INFINITY ? ss[j] * __expf(sm[j] - nm) : 0.f);
      mx = nm;
    }
    tokens[row] = bi;
    if (logprobs) logprobs[row] = bestx - (mx + __logf(sum));
  }
}

// ------------------------------------------------------------------------------------------------
// ids / lps [rows][MAXN]: the kept tokens with the top_n largest values, by value descending then
// token id ascending; lp = z - logsumexp(z over the kept set); unused entries -1 / -inf.  Rows with
// top_n <= 0 are not written.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void top_logprobs_kernel(const bf16_t* __restrict__ logits, long stride, int V,
                                                          const float* __restrict__ temps,
                                                          const float* __restrict__ tau,
                                                          const int* __restrict__ top_n,
                                                          int* __restrict__ ids, float* __restrict__ lps) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const int n = min(top_n[row], MAXN);
  if (n <= 0) return;  // row-uniform, before any barrier
  __shared__ uint32_t cnt1[NB1];
  __shared__ uint32_t cnt2[NB2];
  __shared__ uint32_t sh_c[NT / 64];
  __shared__ int tie[MAXN][NT];  // each thread's first ties at the boundary value, ascending id
  __shared__ int tie_out[MAXN];
  __shared__ uint32_t ab_key[MAXN];
  __shared__ int ab_id[MAXN];
  __shared__ float sm[4], ss[4];
  __shared__ int s_bin, s_min, s_nab;
  __shared__ uint32_t s_cabove, s_keyn;

  const bf16_t* x = logits + (long)row * stride;
  const float T = temps[row];
  const float invT = T > 0.f ? 1.f / T : 1.f;
  const float tv = tau[row];
  for (int b = tid; b < NB1; b += NT) cnt1[b] = 0;
  if (tid < NB2) cnt2[tid] = 0;
  if (tid == 0) {
    s_bin = NB1;
    s_nab = 0;
  }
  __syncthreads();

  // pass 1: first-level counts of the kept set and its log-sum-exp
  float mx = -INFINITY, sum = 0.f;
  for_each(x, V, tid, [&](int, bf16_t u) {
    const float xv = bf2f(u);
    if (u == NEG_INF || xv < tv) return;
    atomicAdd(&cnt1[key_of(u) >> L2B], 1u);
    const float z = xv * invT;
    if (z > mx) {
      sum = sum * __expf(mx - z) + 1.f;
      mx = z;
    } else {
      sum += __expf(z - mx);
    }
  });
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o, 64), os = __shfl_xor(sum, o, 64);
    const float nm = fmaxf(mx, om);
    sum = (mx > -INFINITY ? sum * __expf(mx - nm) : 0.f) + (om > -INFINITY ? os * __expf(om - nm) : 0.f);
    mx = nm;
  }
  if ((tid & 63) == 0) {
    sm[tid >> 6] = mx;
    ss[tid >> 6] = sum;
  }
  __syncthreads();
  mx = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  if (mx == -INFINITY) {  // nothing kept (block-uniform)
    if (tid < MAXN) {
      ids[(long)row * MAXN + tid] = -1;
      lps[(long)row * MAXN + tid] = -INFINITY;
    }
    return;
  }
  sum = 0.f;
  for (int j = 0; j < 4; ++j) sum += sm[j] > -INFINITY ? ss[j] * __expf(sm[j] - mx) : 0.f;
  const float lse = mx + __logf(sum);

  // the lowest non-empty bin with fewer than n kept tokens above it, then the key inside it
  uint32_t c_loc = 0;
  for (int b = tid * BPT; b < tid * BPT + BPT; ++b) c_loc += cnt1[b];
  const uint32_t c_above = sum_above(c_loc, sh_c, tid);
  int cand = NB1;
  uint32_t g = c_above;
  for (int b = tid * BPT + BPT - 1; b >= tid * BPT; --b) {
    if (cnt1[b] > 0 && g < (uint32_t)n) cand = b;
    g += cnt1[b];
  }
  if (cand < NB1) atomicMin(&s_bin, cand);
  __syncthreads();
  const int Bn = s_bin;
  if (tid == Bn / BPT) {
    uint32_t c = c_above;
    for (int b = tid * BPT + BPT - 1; b > Bn; --b) c += cnt1[b];
    s_cabove = c;
  }
  for_each(x, V, tid, [&](int, bf16_t u) {
    if (u == NEG_INF || bf2f(u) < tv) return;
    const uint32_t key = key_of(u);
    if ((int)(key >> L2B) == Bn) atomicAdd(&cnt2[key & (NB2 - 1)], 1u);
  });
  __syncthreads();
  if (tid == 0) {
    uint32_t g2 = s_cabove, above = g2;
    int sel = NB2 - 1;
    for (int s = NB2 - 1; s >= 0; --s) {
      if (cnt2[s] > 0 && g2 < (uint32_t)n) {
        sel = s;
        above = g2;
      }
      g2 += cnt2[s];
    }
    s_keyn = ((uint32_t)Bn << L2B) | (uint32_t)sel;
    s_cabove = above;  // kept tokens strictly above the boundary value (< n)
  }
  __syncthreads();
  const uint32_t keyn = s_keyn;
  const int m = n - (int)s_cabove;  // entries left for the boundary value's ties (>= 1)

  // gather: everything above the boundary, and each thread's first m ties at it
  int mine = 0;
  for_each(x, V, tid, [&](int i, bf16_t u) {
    if (u == NEG_INF || bf2f(u) < tv) return;
    const uint32_t key = key_of(u);
    if (key > keyn) {
      const int s = atomicAdd(&s_nab, 1);
      if (s < MAXN) {
        ab_key[s] = key;
        ab_id[s] = i;
      }
    } else if (key == keyn && mine < m) {
      tie[mine++][tid] = i;
    }
  });
  __syncthreads();
  // merge the per-thread tie lists: the m lowest ids, one per round
  int head = 0, ntie = 0;
  for (int j = 0; j < m; ++j) {
    if (tid == 0) s_min = 0x7fffffff;
    __syncthreads();
    const int h = head < mine ? tie[head][tid] : 0x7fffffff;
    if (h != 0x7fffffff) atomicMin(&s_min, h);
    __syncthreads();
    const int cur = s_min;
    if (cur == 0x7fffffff) break;  // block-uniform
    if (h == cur) {
      ++head;
      tie_out[j] = cur;
    }
    ++ntie;
    __syncthreads();
  }
  __syncthreads();
  const int nab = min(s_nab, MAXN);
  if (tid < MAXN) {
    int* oi = ids + (long)row * MAXN;
    float* ol = lps + (long)row * MAXN;
    if (tid < nab) {
      const uint32_t ke = ab_key[tid];
      const int ie = ab_id[tid];
      int rank = 0;
      for (int f = 0; f < nab; ++f) rank += (ab_key[f] > ke || (ab_key[f] == ke && ab_id[f] < ie)) ? 1 : 0;
      oi[rank] = ie;
      ol[rank] = val_of(ke) * invT - lse;
    }
    if (tid >= nab && tid < nab + ntie) {
      oi[tid] = tie_out[tid - nab];
      ol[tid] = val_of(keyn) * invT - lse;
    }
    if (tid >= nab + ntie) {
      oi[tid] = -1;
      ol[tid] = -INFINITY;
    }
  }
}

}  // namespace

extern "C" int dsa_top_logprobs_max() { return MAXN; }

extern "C" hipError_t dsa_sample_threshold(const void* logits, long stride, int rows, int V, const float* temps,
                                           const int* top_k, const float* top_p, const float* min_p, float* tau,
                                           hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  if (V < 1) return hipErrorInvalidValue;
  threshold_kernel<<<rows, NT, 0, st>>>((const bf16_t*)logits, stride, V, temps, top_k, top_p, min_p, tau);
  return hipGetLastError();
}

extern "C" hipError_t dsa_sample_masked(const void* logits, long stride, int rows, int V, const float* temps,
                                        const int64_t* seeds, const int* steps, const float* tau, int* tokens,
                                        float* logprobs, hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  if (V < 1) return hipErrorInvalidValue;
  sample_masked_kernel<<<rows, NT, 0, st>>>((const bf16_t*)logits, stride, V, temps, seeds, steps, tau, tokens,
                                            logprobs);
  return hipGetLastError();
}

extern "C" hipError_t dsa_top_logprobs(const void* logits, long stride, int rows, int V, const float* temps,
                                       const float* tau, const int* top_n, int* ids, float* lps, hipStream_t st) {
  if (rows <= 0) return hipSuccess;
  if (V < 1) return hipErrorInvalidValue;
  top_logprobs_kernel<<<rows, NT, 0, st>>>((const bf16_t*)logits, stride, V, temps, tau, top_n, ids, lps);
  return hipGetLastError();
}
