// cc_sample.hip — seeded temperature / top-k sampling tail (include/coldcompress.h, cc_sample_topk): the reference's
// logits_to_probs (generation_utils.py:125-133) followed by a STATELESS Gumbel-max draw, so that one (logits, temperature, top_k,
// seed, position) has one answer in eager launches, under hipGraph replay and on every tensor-parallel rank.
// Launches over a fixed grid of kSpBlocks workgroups, every one a pure function of what the launches before it left in the workspace
// (no atomics on global memory, no tickets: per-workgroup partials folded in a fixed order):
//   select    one launch per 8-bit digit of the scaled value's orderable pattern, most significant first (two for bf16 / f16, four for
//             fp32; none without top_k): a 256-bin LDS histogram per workgroup of the elements that match the digits chosen so far.
//             The next launch folds the 128 histograms itself and walks the counts from the top to the digit that holds the k-th
//             largest element.  The first of them also leaves the per-workgroup maxima (the largest kept value IS the global maximum).
//   draw      folds the last histogram into the pivot; per workgroup the sum of exp(x - m) over the kept set and the best Gumbel key.
//   write     folds the sums, writes the probabilities (exactly 0 outside the kept set); workgroup 0 folds the keys into the token.
// cc_sample_nucleus (top-p, min-p) adds, between select and draw:
//   mass      one launch per digit again, over the top-k kept set: 256 bins of 64-bit INTEGER masses floor(exp(x - m) * 2^40) per
//             workgroup (LDS atomics; integer sums do not depend on their order), folded and walked by the next launch to the digit at
//             which the running mass reaches ceil(top_p * Z); the first pass's histogram sums to Z.  min-p is a compare in draw and write.
#include "cc_common.h"

namespace {
constexpr int kSpThreads = 256;
constexpr int kSpBlocks = 128;
constexpr int kSpWaves = kSpThreads / CC_WAVE;

struct SpWs {  // caller-provided scratch (cc_sample_topk_workspace_bytes); nothing in it is read before a launch of the call wrote it
  unsigned int hist[2][kSpBlocks][256];  // digit counts of select pass P in hist[P & 1]
  float maxpart[kSpBlocks];
  float sumpart[kSpBlocks];
  unsigned long long keypart[kSpBlocks];
  unsigned int prefix[4], krem[4];  // after pass P: the digits chosen so far, and the rank of the pivot among the elements that match them
};

// Rows (cc_sample_rows): every kernel runs on a (kSpBlocks, T) grid and blockIdx.y is the row: its logits at row * row_stride, its
// probs at row * V, its token / kept count / position at [row], its seed from the by-value array, its workspace record at
// row * ws_stride BYTES (sizeof(SpWs) or sizeof(SpNucWs): the record type of the entry point that was called).  Nothing else in a
// kernel looks at blockIdx.y or at T, so a row's arithmetic is the single-row launch's; the single-row entry points are T = 1.
struct SpSeeds {
  unsigned long long s[CC_SAMPLE_MAX_ROWS];
};
template <typename T>
__device__ __forceinline__ const T* sp_row_logits(const T* logits, long long row_stride) {
  return logits + (size_t)blockIdx.y * (size_t)row_stride;
}
__device__ __forceinline__ SpWs* sp_row_ws(SpWs* ws, size_t ws_stride) {
  return reinterpret_cast<SpWs*>(reinterpret_cast<char*>(ws) + (size_t)blockIdx.y * ws_stride);
}

template <typename T>
__device__ __forceinline__ float sp_exp(float x) {  // cc_softmax_argmax's accuracy class (cc_glue.hip, sm_exp)
  if constexpr (sizeof(T) == 4) return expf(x);
  return __builtin_amdgcn_exp2f(x * 1.4426950408889634f);
}

// "larger is better" orderable pattern of a scaled value (already rounded to T), NB bits; -0 is +0 (they compare equal)
template <typename T>
struct SpKey;
template <>
struct SpKey<float> {
  static constexpr int NB = 32;
  __device__ static __forceinline__ uint32_t key(float x) {
    const uint32_t u = __float_as_uint(x == 0.f ? 0.f : x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
};
__device__ __forceinline__ uint32_t sp_key16(uint32_t b) {
  if ((b & 0x7fffu) == 0u) b = 0u;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
template <>
struct SpKey<bf16_t> {
  static constexpr int NB = 16;
  __device__ static __forceinline__ uint32_t key(float x) { return sp_key16(__float_as_uint(x) >> 16); }
};
template <>
struct SpKey<f16_t> {
  static constexpr int NB = 16;
  __device__ static __forceinline__ uint32_t key(float x) { return sp_key16(f32_to_f16_bits(x)); }
};

__device__ __forceinline__ void sp_slice(int V, int& lo, int& hi) {
  const long long per = (((long long)V + kSpBlocks - 1) / kSpBlocks + 7) & ~7ll;
  lo = (int)min((long long)V, (long long)blockIdx.x * per);
  hi = (int)min((long long)V, (long long)lo + per);
}

// step 1 of the contract: one IEEE fp32 division, then the model dtype's rounding
template <typename T>
__device__ __forceinline__ float sp_scaled(const T* logits, int i, float tmax) {
  return ElemTraits<T>::rnd(__fdiv_rn(ElemTraits<T>::load(logits, (size_t)i), tmax));
}

// Fold the 128 histograms of select pass P (thread t owns digit t) and walk the counts from digit 255 down to the digit that holds
// the element of rank krem: -> the digits chosen so far including this one, and the pivot's rank among the elements that match them.
// Every workgroup computes the same pair; workgroup 0 leaves it for the NEXT launch's fold.  s_w: kSpWaves + 2 words.
__device__ __forceinline__ void sp_fold(SpWs* ws, int P, int k, unsigned int* s_w, uint32_t& prefix, uint32_t& krem) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t pfx = 0u, kr = (uint32_t)k;
  if (P > 0) {
    pfx = ws->prefix[P - 1];
    kr = ws->krem[P - 1];
  }
  uint32_t c = 0u;
  for (int g = 0; g < kSpBlocks; g++) c += ws->hist[P & 1][g][threadIdx.x];
  uint32_t s = c;  // inclusive suffix sum over the wave's digits (digit = threadIdx.x: higher lanes hold larger values)
#pragma unroll
  for (int off = 1; off < CC_WAVE; off <<= 1) {
    const uint32_t o = __shfl_down(s, off, CC_WAVE);
    if (lane + off < CC_WAVE) s += o;
  }
  if (lane == 0) s_w[wave] = s;
  if (threadIdx.x == 0) {  // (unreachable fall-back: the matching elements number at least kr)
    s_w[kSpWaves] = pfx << 8;
    s_w[kSpWaves + 1] = 1u;
  }
  __syncthreads();
  uint32_t above = 0u;
  for (int w = wave + 1; w < kSpWaves; w++) above += s_w[w];
  const uint32_t incl = s + above, excl = incl - c;
  if (excl < kr && kr <= incl) {  // exactly one digit
    s_w[kSpWaves] = (pfx << 8) | (uint32_t)threadIdx.x;
    s_w[kSpWaves + 1] = kr - excl;
  }
  __syncthreads();
  prefix = s_w[kSpWaves];
  krem = s_w[kSpWaves + 1];
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ws->prefix[P] = prefix;
    ws->krem[P] = krem;
  }
}

// select pass P (k > 0), and for P == 0 the per-workgroup maxima (k == 0: those alone)
template <typename T, int P>
__global__ __launch_bounds__(kSpThreads) void sample_hist_kernel(const T* logits, long long row_stride, int V, float tmax, int k, SpWs* ws,
                                                                 size_t ws_stride) {
  constexpr int NB = SpKey<T>::NB;
  logits = sp_row_logits(logits, row_stride);
  ws = sp_row_ws(ws, ws_stride);
  __shared__ unsigned int sh[256];
  __shared__ unsigned int s_w[kSpWaves + 2];
  __shared__ float s_f[kSpWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int lo, hi;
  sp_slice(V, lo, hi);
  uint32_t prefix = 0u, krem = 0u;
  if constexpr (P > 0) sp_fold(ws, P - 1, k, s_w, prefix, krem);
  sh[threadIdx.x] = 0u;
  __syncthreads();
  float mx = -INFINITY;
  for (int i = lo + threadIdx.x; i < hi; i += kSpThreads) {
    const float x = sp_scaled<T>(logits, i, tmax);
    if constexpr (P == 0) mx = fmaxf(mx, x);
    if (k > 0) {
      const uint32_t key = SpKey<T>::key(x);
      bool match = true;
      if constexpr (P > 0) match = (key >> (NB - 8 * P)) == prefix;
      if (match) atomicAdd(&sh[(key >> (NB - 8 * (P + 1))) & 0xffu], 1u);
    }
  }
  __syncthreads();
  if (k > 0) ws->hist[P & 1][blockIdx.x][threadIdx.x] = sh[threadIdx.x];
  if constexpr (P == 0) {
    mx = wave_max_f32(mx);
    if (lane == 0) s_f[wave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) ws->maxpart[blockIdx.x] = fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));
  }
}

// the global maximum of the scaled values from the per-workgroup maxima (NaN never counts: fmaxf); valid in every thread
__device__ __forceinline__ float sp_fold_max(const SpWs* ws, float* s_f) {
  if (threadIdx.x < CC_WAVE) {
    float m = -INFINITY;
    for (int g = threadIdx.x; g < kSpBlocks; g += CC_WAVE) m = fmaxf(m, ws->maxpart[g]);
    m = wave_max_f32(m);
    if (threadIdx.x == 0) s_f[0] = m;
  }
  __syncthreads();
  return s_f[0];
}

// steps 4 and 5 of the contract.  -log(u) through log1pf for u > 1/2 (1 - u is exact there): libm-grade where the winners come from
__device__ __forceinline__ float sp_gumbel_key(float d, uint64_t seed, int32_t pos, int i) {
  const uint64_t h = cc_mix64(cc_mix64((seed ^ 0x53414D504C45ull) + (uint64_t)(uint32_t)pos * 0x9E3779B97F4A7C15ull + (uint64_t)(uint32_t)i));
  const float u = (float)(uint32_t)(2u * (uint32_t)(h >> 41) + 1u) * 5.9604644775390625e-08f;  // odd multiple of 2^-24: exact, never 0 or 1
  const float e = u > 0.5f ? -log1pf(__fsub_rn(u, 1.0f)) : -logf(u);
  return __fsub_rn(d, logf(e));
}

template <typename T, int NP>  // NP: select passes that ran (0: everything is kept)
__global__ __launch_bounds__(kSpThreads) void sample_draw_kernel(const T* logits, long long row_stride, int V, float tmax, int k, SpSeeds seeds,
                                                                 const int32_t* input_pos, SpWs* ws, size_t ws_stride) {
  __shared__ unsigned int s_w[kSpWaves + 2];
  __shared__ float s_f[kSpWaves];
  __shared__ unsigned long long s_k[kSpWaves + 1];
  logits = sp_row_logits(logits, row_stride);
  ws = sp_row_ws(ws, ws_stride);
  input_pos += blockIdx.y;
  const unsigned long long seed = seeds.s[blockIdx.y];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int lo, hi;
  sp_slice(V, lo, hi);
  uint32_t pivot = 0u, krem = 0u;
  if constexpr (NP > 0) sp_fold(ws, NP - 1, k, s_w, pivot, krem);
  const float m = sp_fold_max(ws, s_f);
  __syncthreads();
  const int32_t pos = *input_pos;
  float sum = 0.f;
  unsigned long long best = ~0ull;
  for (int i = lo + threadIdx.x; i < hi; i += kSpThreads) {
    const float x = sp_scaled<T>(logits, i, tmax);
    unsigned long long cand = ~0ull;
    if (x != x) {
      cand = (unsigned long long)(unsigned)i;  // upper half 0 beats every number: the first NaN's index (cc_softmax_argmax's rule)
    } else if (SpKey<T>::key(x) >= pivot) {
      const float d = __fsub_rn(x, m);
      sum += sp_exp<T>(d);
      cand = ((unsigned long long)(~orderable_f32(sp_gumbel_key(d, seed, pos, i))) << 32) | (unsigned)i;
    }
    best = cand < best ? cand : best;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, CC_WAVE);
  if (lane == 0) s_f[wave] = sum;
  best = block_min_u64(best, s_k);  // (its barriers also publish s_f)
  if (threadIdx.x == 0) {
    ws->sumpart[blockIdx.x] = (s_f[0] + s_f[1]) + (s_f[2] + s_f[3]);
    ws->keypart[blockIdx.x] = best;
  }
}

template <typename T, int NP>
__global__ __launch_bounds__(kSpThreads) void sample_write_kernel(const T* logits, long long row_stride, int V, float tmax, T* probs,
                                                                  int32_t* idx_out, SpWs* ws, size_t ws_stride) {
  __shared__ float s_f[kSpWaves];
  __shared__ float s_sum;
  logits = sp_row_logits(logits, row_stride);
  ws = sp_row_ws(ws, ws_stride);
  probs += (size_t)blockIdx.y * (size_t)V;
  idx_out += blockIdx.y;
  int lo, hi;
  sp_slice(V, lo, hi);
  const float m = sp_fold_max(ws, s_f);
  if (threadIdx.x < CC_WAVE) {  // one wave folds the sums in a fixed order
    float s = 0.f;
    for (int g = threadIdx.x; g < kSpBlocks; g += CC_WAVE) s += ws->sumpart[g];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, CC_WAVE);
    if (threadIdx.x == 0) s_sum = s;
  }
  __syncthreads();
  const float sum = s_sum;
  uint32_t pivot = 0u;
  if constexpr (NP > 0) pivot = ws->prefix[NP - 1];
  for (int i = lo + threadIdx.x; i < hi; i += kSpThreads) {
    const float x = sp_scaled<T>(logits, i, tmax);
    float p = 0.f;
    if (x != x || SpKey<T>::key(x) >= pivot) p = ElemTraits<T>::rnd(__fdiv_rn(sp_exp<T>(__fsub_rn(x, m)), sum));
    ElemTraits<T>::store(probs, (size_t)i, p);
  }
  if (blockIdx.x == 0 && threadIdx.x < CC_WAVE) {
    unsigned long long b = ~0ull;
    for (int g = threadIdx.x; g < kSpBlocks; g += CC_WAVE) {
      const unsigned long long o = ws->keypart[g];
      b = o < b ? o : b;
    }
    b = wave_min_u64(b);
    if (threadIdx.x == 0) *idx_out = b == ~0ull ? 0 : (int32_t)(b & 0xffffffffull);  // (no candidate at all cannot happen for V > 0: a valid index anyway)
  }
}

template <typename T>
void sp_launch(const void* logits_, int rows, long long rs, int V, float tmax, int k, const SpSeeds& seeds, const int32_t* input_pos,
               void* probs_, int32_t* idx_out, SpWs* ws, size_t wss, hipStream_t st) {
  const T* logits = (const T*)logits_;
  T* probs = (T*)probs_;
  dim3 grid(kSpBlocks, rows), block(kSpThreads);
  hipLaunchKernelGGL((sample_hist_kernel<T, 0>), grid, block, 0, st, logits, rs, V, tmax, k, ws, wss);
  if (k <= 0) {
    hipLaunchKernelGGL((sample_draw_kernel<T, 0>), grid, block, 0, st, logits, rs, V, tmax, k, seeds, input_pos, ws, wss);
    hipLaunchKernelGGL((sample_write_kernel<T, 0>), grid, block, 0, st, logits, rs, V, tmax, probs, idx_out, ws, wss);
    return;
  }
  hipLaunchKernelGGL((sample_hist_kernel<T, 1>), grid, block, 0, st, logits, rs, V, tmax, k, ws, wss);
  constexpr int NP = SpKey<T>::NB / 8;
  if constexpr (NP == 4) {
    hipLaunchKernelGGL((sample_hist_kernel<T, 2>), grid, block, 0, st, logits, rs, V, tmax, k, ws, wss);
    hipLaunchKernelGGL((sample_hist_kernel<T, 3>), grid, block, 0, st, logits, rs, V, tmax, k, ws, wss);
  }
  hipLaunchKernelGGL((sample_draw_kernel<T, NP>), grid, block, 0, st, logits, rs, V, tmax, k, seeds, input_pos, ws, wss);
  hipLaunchKernelGGL((sample_write_kernel<T, NP>), grid, block, 0, st, logits, rs, V, tmax, probs, idx_out, ws, wss);
}

// ---- top-p / min-p (cc_sample_nucleus): a second radix select over the same key, after the top-k one, whose bins hold 64-bit masses
struct SpNucWs {  // cc_sample_nucleus_workspace_bytes; as SpWs, nothing is read before a launch of the call wrote it
  SpWs base;
  unsigned long long mass[2][kSpBlocks][256];  // digit masses of nucleus pass Q in mass[Q & 1]
  unsigned long long mrem[4];                  // after pass Q: the mass still to collect among the elements that match mprefix[Q]
  unsigned int mprefix[4];
  unsigned int cntpart[kSpBlocks];
};

// step 2a's integer mass of an element d = x - m below the maximum: floor(exp(d) * 2^40), the exp being the softmax's (sp_exp<T>)
template <typename T>
__device__ __forceinline__ unsigned long long sp_mass(float d) {
  return (unsigned long long)(sp_exp<T>(d) * 1099511627776.0f);  // (the scaling by 2^40 is exact; the conversion truncates)
}

// sp_fold for masses: fold the 128 mass histograms of nucleus pass Q (thread t owns digit t) and walk them from digit 255 down to the
// digit at which the running mass reaches what is still to collect; pass 0's histogram sums to Z, so the target is computed here.
// Integer sums: the same in every workgroup whatever order the LDS atomics ran in.  s_m: kSpWaves + 1 words, s_w: 1 word.
__device__ __forceinline__ uint32_t sp_fold_mass(SpNucWs* nws, int Q, float top_p, unsigned long long* s_m, unsigned int* s_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t pfx = 0u;
  unsigned long long rem = 0ull;
  if (Q > 0) {
    pfx = nws->mprefix[Q - 1];
    rem = nws->mrem[Q - 1];
  }
  unsigned long long c = 0ull;
  for (int g = 0; g < kSpBlocks; g++) c += nws->mass[Q & 1][g][threadIdx.x];
  unsigned long long s = c;  // inclusive suffix sum over the wave's digits
#pragma unroll
  for (int off = 1; off < CC_WAVE; off <<= 1) {
    const unsigned long long o = __shfl_down(s, off, CC_WAVE);
    if (lane + off < CC_WAVE) s += o;
  }
  if (lane == 0) s_m[wave] = s;
  if (threadIdx.x == 0) {  // (no digit reaches the target only when Z is 0: no finite element at all.  Digit 0: everything stays)
    s_w[0] = pfx << 8;
    s_m[kSpWaves] = 0ull;
  }
  __syncthreads();
  if (Q == 0) {
    const unsigned long long Z = (s_m[0] + s_m[1]) + (s_m[2] + s_m[3]);
    rem = (unsigned long long)ceil(__dmul_rn((double)top_p, (double)Z));
    rem = rem < Z ? rem : Z;
  }
  unsigned long long above = 0ull;
  for (int w = wave + 1; w < kSpWaves; w++) above += s_m[w];
  const unsigned long long incl = s + above, excl = incl - c;
  if (excl < rem && rem <= incl) {  // exactly one digit (its own mass is not 0)
    s_w[0] = (pfx << 8) | (uint32_t)threadIdx.x;
    s_m[kSpWaves] = rem - excl;
  }
  __syncthreads();
  const uint32_t prefix = s_w[0];
  rem = s_m[kSpWaves];
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    nws->mprefix[Q] = prefix;
    nws->mrem[Q] = rem;
  }
  return prefix;
}

// nucleus pass Q over K = the top-k kept set without NaNs (NPK: top-k select passes that ran; pass 0 folds the last of them)
template <typename T, int NPK, int Q>
__global__ __launch_bounds__(kSpThreads) void sample_mass_kernel(const T* logits, long long row_stride, int V, float tmax, int k, float top_p,
                                                                 SpNucWs* nws) {
  constexpr int NB = SpKey<T>::NB;
  __shared__ unsigned long long shm[256];
  __shared__ unsigned long long s_m[kSpWaves + 1];
  __shared__ unsigned int s_w[kSpWaves + 2];
  __shared__ float s_f[kSpWaves];
  logits = sp_row_logits(logits, row_stride);
  nws += blockIdx.y;
  SpWs* ws = &nws->base;
  int lo, hi;
  sp_slice(V, lo, hi);
  uint32_t kpivot = 0u, mprefix = 0u;
  if constexpr (NPK > 0) {
    if constexpr (Q == 0) {
      uint32_t krem;
      sp_fold(ws, NPK - 1, k, s_w, kpivot, krem);
    } else {
      kpivot = ws->prefix[NPK - 1];
    }
  }
  if constexpr (Q > 0) mprefix = sp_fold_mass(nws, Q - 1, top_p, s_m, s_w);
  const float m = sp_fold_max(ws, s_f);
  shm[threadIdx.x] = 0ull;
  __syncthreads();
  for (int i = lo + threadIdx.x; i < hi; i += kSpThreads) {
    const float x = sp_scaled<T>(logits, i, tmax);
    if (x != x) continue;
    const uint32_t key = SpKey<T>::key(x);
    bool match = key >= kpivot;
    if constexpr (Q > 0) match = match && (key >> (NB - 8 * Q)) == mprefix;
    if (match) atomicAdd(&shm[(key >> (NB - 8 * (Q + 1))) & 0xffu], sp_mass<T>(__fsub_rn(x, m)));
  }
  __syncthreads();
  nws->mass[Q & 1][blockIdx.x][threadIdx.x] = shm[threadIdx.x];
}

// the draw launch with the two filters (NPQ: nucleus passes that ran; 0: top-p is off) and the per-workgroup count of kept elements
template <typename T, int NPK, int NPQ>
__global__ __launch_bounds__(kSpThreads) void sample_draw_nucleus_kernel(const T* logits, long long row_stride, int V, float tmax, int k,
                                                                         float top_p, float dmin, SpSeeds seeds, const int32_t* input_pos,
                                                                         SpNucWs* nws) {
  __shared__ unsigned int s_w[kSpWaves + 2];
  __shared__ float s_f[kSpWaves];
  __shared__ unsigned long long s_k[kSpWaves + 1];
  __shared__ unsigned int s_c[kSpWaves];
  logits = sp_row_logits(logits, row_stride);
  nws += blockIdx.y;
  input_pos += blockIdx.y;
  const unsigned long long seed = seeds.s[blockIdx.y];
  SpWs* ws = &nws->base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int lo, hi;
  sp_slice(V, lo, hi);
  uint32_t pivot = 0u;
  if constexpr (NPQ > 0) {  // (the nucleus pivot is a key of K: never below the top-k pivot)
    pivot = sp_fold_mass(nws, NPQ - 1, top_p, s_k, s_w);
  } else if constexpr (NPK > 0) {
    uint32_t krem;
    sp_fold(ws, NPK - 1, k, s_w, pivot, krem);
  }
  const float m = sp_fold_max(ws, s_f);
  __syncthreads();
  const int32_t pos = *input_pos;
  float sum = 0.f;
  unsigned int cnt = 0u;
  unsigned long long best = ~0ull;
  for (int i = lo + threadIdx.x; i < hi; i += kSpThreads) {
    const float x = sp_scaled<T>(logits, i, tmax);
    unsigned long long cand = ~0ull;
    if (x != x) {
      cand = (unsigned long long)(unsigned)i;
    } else if (SpKey<T>::key(x) >= pivot) {
      const float d = __fsub_rn(x, m);
      if (d >= dmin) {
        sum += sp_exp<T>(d);
        cnt++;
        cand = ((unsigned long long)(~orderable_f32(sp_gumbel_key(d, seed, pos, i))) << 32) | (unsigned)i;
      }
    }
    best = cand < best ? cand : best;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_xor(sum, off, CC_WAVE);
    cnt += __shfl_xor(cnt, off, CC_WAVE);
  }
  if (lane == 0) {
    s_f[wave] = sum;
    s_c[wave] = cnt;
  }
  best = block_min_u64(best, s_k);  // (its barriers also publish s_f and s_c)
  if (threadIdx.x == 0) {
    ws->sumpart[blockIdx.x] = (s_f[0] + s_f[1]) + (s_f[2] + s_f[3]);
    ws->keypart[blockIdx.x] = best;
    nws->cntpart[blockIdx.x] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
  }
}

template <typename T, int NPK, int NPQ>
__global__ __launch_bounds__(kSpThreads) void sample_write_nucleus_kernel(const T* logits, long long row_stride, int V, float tmax, float dmin,
                                                                          T* probs, int32_t* idx_out, int32_t* n_kept_out, SpNucWs* nws) {
  __shared__ float s_f[kSpWaves];
  __shared__ float s_sum;
  logits = sp_row_logits(logits, row_stride);
  nws += blockIdx.y;
  probs += (size_t)blockIdx.y * (size_t)V;
  idx_out += blockIdx.y;
  if (n_kept_out) n_kept_out += blockIdx.y;
  SpWs* ws = &nws->base;
  int lo, hi;
  sp_slice(V, lo, hi);
  const float m = sp_fold_max(ws, s_f);
  if (threadIdx.x < CC_WAVE) {  // one wave folds the sums in a fixed order
    float s = 0.f;
    for (int g = threadIdx.x; g < kSpBlocks; g += CC_WAVE) s += ws->sumpart[g];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, CC_WAVE);
    if (threadIdx.x == 0) s_sum = s;
  }
  __syncthreads();
  const float sum = s_sum;
  uint32_t pivot = 0u;
  if constexpr (NPQ > 0) pivot = nws->mprefix[NPQ - 1];
  else if constexpr (NPK > 0) pivot = ws->prefix[NPK - 1];
  for (int i = lo + threadIdx.x; i < hi; i += kSpThreads) {
    const float x = sp_scaled<T>(logits, i, tmax);
    const float d = __fsub_rn(x, m);
    float p = 0.f;
    if (x != x || (SpKey<T>::key(x) >= pivot && d >= dmin)) p = ElemTraits<T>::rnd(__fdiv_rn(sp_exp<T>(d), sum));
    ElemTraits<T>::store(probs, (size_t)i, p);
  }
  if (blockIdx.x == 0 && threadIdx.x < CC_WAVE) {
    unsigned long long b = ~0ull;
    unsigned int n = 0u;
    for (int g = threadIdx.x; g < kSpBlocks; g += CC_WAVE) {
      const unsigned long long o = ws->keypart[g];
      b = o < b ? o : b;
      n += nws->cntpart[g];
    }
    b = wave_min_u64(b);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, CC_WAVE);
    if (threadIdx.x == 0) {
      *idx_out = b == ~0ull ? 0 : (int32_t)(b & 0xffffffffull);
      if (n_kept_out) *n_kept_out = (int32_t)n;
    }
  }
}

struct SpnArgs {  // one call's rows and settings, as the launch helpers pass them on
  int rows;
  long long rs;
  int V;
  float tmax;
  int k;
  bool with_p;
  float top_p, dmin;
  SpSeeds seeds;
  const int32_t* input_pos;
  int32_t *idx_out, *n_kept_out;
  SpNucWs* nws;
  hipStream_t st;
};

template <typename T, int NPK>
void spn_tail(const T* logits, T* probs, const SpnArgs& a) {
  constexpr int NP = SpKey<T>::NB / 8;
  dim3 grid(kSpBlocks, a.rows), block(kSpThreads);
  if (!a.with_p) {
    hipLaunchKernelGGL((sample_draw_nucleus_kernel<T, NPK, 0>), grid, block, 0, a.st, logits, a.rs, a.V, a.tmax, a.k, a.top_p, a.dmin, a.seeds,
                       a.input_pos, a.nws);
    hipLaunchKernelGGL((sample_write_nucleus_kernel<T, NPK, 0>), grid, block, 0, a.st, logits, a.rs, a.V, a.tmax, a.dmin, probs, a.idx_out,
                       a.n_kept_out, a.nws);
    return;
  }
  hipLaunchKernelGGL((sample_mass_kernel<T, NPK, 0>), grid, block, 0, a.st, logits, a.rs, a.V, a.tmax, a.k, a.top_p, a.nws);
  hipLaunchKernelGGL((sample_mass_kernel<T, NPK, 1>), grid, block, 0, a.st, logits, a.rs, a.V, a.tmax, a.k, a.top_p, a.nws);
  if constexpr (NP == 4) {
    hipLaunchKernelGGL((sample_mass_kernel<T, NPK, 2>), grid, block, 0, a.st, logits, a.rs, a.V, a.tmax, a.k, a.top_p, a.nws);
    hipLaunchKernelGGL((sample_mass_kernel<T, NPK, 3>), grid, block, 0, a.st, logits, a.rs, a.V, a.tmax, a.k, a.top_p, a.nws);
  }
  hipLaunchKernelGGL((sample_draw_nucleus_kernel<T, NPK, NP>), grid, block, 0, a.st, logits, a.rs, a.V, a.tmax, a.k, a.top_p, a.dmin, a.seeds,
                     a.input_pos, a.nws);
  hipLaunchKernelGGL((sample_write_nucleus_kernel<T, NPK, NP>), grid, block, 0, a.st, logits, a.rs, a.V, a.tmax, a.dmin, probs, a.idx_out,
                     a.n_kept_out, a.nws);
}

template <typename T>
void spn_launch(const void* logits_, void* probs_, const SpnArgs& a) {
  const T* logits = (const T*)logits_;
  T* probs = (T*)probs_;
  constexpr int NP = SpKey<T>::NB / 8;
  constexpr size_t wss = sizeof(SpNucWs);
  dim3 grid(kSpBlocks, a.rows), block(kSpThreads);
  hipLaunchKernelGGL((sample_hist_kernel<T, 0>), grid, block, 0, a.st, logits, a.rs, a.V, a.tmax, a.k, &a.nws->base, wss);  // (k == 0: the maxima alone)
  if (a.k <= 0) {
    spn_tail<T, 0>(logits, probs, a);
    return;
  }
  hipLaunchKernelGGL((sample_hist_kernel<T, 1>), grid, block, 0, a.st, logits, a.rs, a.V, a.tmax, a.k, &a.nws->base, wss);
  if constexpr (NP == 4) {
    hipLaunchKernelGGL((sample_hist_kernel<T, 2>), grid, block, 0, a.st, logits, a.rs, a.V, a.tmax, a.k, &a.nws->base, wss);
    hipLaunchKernelGGL((sample_hist_kernel<T, 3>), grid, block, 0, a.st, logits, a.rs, a.V, a.tmax, a.k, &a.nws->base, wss);
  }
  spn_tail<T, NP>(logits, probs, a);
}

// cc_sample_nucleus's value refusals and its launches for `rows` rows whose workspace records are SpNucWs (both entry points)
int spn_rows(const void* logits, int rows, int V, long long rs, int dtype, float temperature, int top_k, float top_p, float min_p,
             const SpSeeds& seeds, const int32_t* input_pos, void* probs, int32_t* idx_out, int32_t* n_kept_out, void* workspace,
             size_t workspace_bytes, hipStream_t st) {
  if (!logits || !probs || !idx_out || !input_pos || !workspace || V <= 0 || !cc_dt_ok(dtype) || !(temperature > 0.f)) return CC_ERR_BAD_ARG;
  if (!(top_p > 0.f) || !(min_p <= 1.f)) return CC_ERR_BAD_ARG;  // (NaN fails both comparisons)
  const bool with_p = top_p < 1.f, with_min = min_p > 0.f;
  if (with_p && V > CC_SAMPLE_NUCLEUS_MAX_V) return CC_ERR_BAD_ARG;
  if (workspace_bytes < (size_t)rows * sizeof(SpNucWs)) return CC_ERR_WORKSPACE;
  if (((uintptr_t)workspace & 7u) != 0) return CC_ERR_BAD_ARG;
  SpNucWs* nws = reinterpret_cast<SpNucWs*>(workspace);
  const float tmax = temperature > 1e-5f ? temperature : 1e-5f;
  const int k = (top_k <= 0 || top_k >= V) ? 0 : top_k;
  if (!with_p && !with_min && !n_kept_out) {  // both filters off: cc_sample_topk's own launches
    switch (dtype) {
      case CC_DT_F32: sp_launch<float>(logits, rows, rs, V, tmax, k, seeds, input_pos, probs, idx_out, &nws->base, sizeof(SpNucWs), st); break;
      case CC_DT_BF16: sp_launch<bf16_t>(logits, rows, rs, V, tmax, k, seeds, input_pos, probs, idx_out, &nws->base, sizeof(SpNucWs), st); break;
      default: sp_launch<f16_t>(logits, rows, rs, V, tmax, k, seeds, input_pos, probs, idx_out, &nws->base, sizeof(SpNucWs), st); break;
    }
    CC_LAUNCH_CHECK();
    return CC_OK;
  }
  const float dmin = with_min ? (float)log((double)min_p) : -INFINITY;
  const SpnArgs a{rows, rs, V, tmax, k, with_p, top_p, dmin, seeds, input_pos, idx_out, n_kept_out, nws, st};
  switch (dtype) {
    case CC_DT_F32: spn_launch<float>(logits, probs, a); break;
    case CC_DT_BF16: spn_launch<bf16_t>(logits, probs, a); break;
    default: spn_launch<f16_t>(logits, probs, a); break;
  }
  CC_LAUNCH_CHECK();
  return CC_OK;
}
}  // namespace

extern "C" size_t cc_sample_topk_workspace_bytes(void) { return sizeof(SpWs); }

extern "C" int cc_sample_topk(const void* logits, int32_t V, int32_t dtype, float temperature, int32_t top_k, uint64_t seed,
                              const int32_t* input_pos, void* probs, int32_t* idx_out, void* workspace, size_t workspace_bytes,
                              cc_stream_t stream) {
  CC_ENTRY();
  if (!logits || !probs || !idx_out || !input_pos || !workspace || V <= 0 || !cc_dt_ok(dtype) || !(temperature > 0.f)) return CC_ERR_BAD_ARG;
  if (workspace_bytes < sizeof(SpWs)) return CC_ERR_WORKSPACE;
  if (((uintptr_t)workspace & 7u) != 0) return CC_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  SpWs* ws = reinterpret_cast<SpWs*>(workspace);
  const float tmax = temperature > 1e-5f ? temperature : 1e-5f;
  const int k = (top_k <= 0 || top_k >= V) ? 0 : top_k;  // k = min(top_k, V) = V keeps everything, as no top_k does
  SpSeeds seeds{};
  seeds.s[0] = seed;
  switch (dtype) {
    case CC_DT_F32: sp_launch<float>(logits, 1, V, V, tmax, k, seeds, input_pos, probs, idx_out, ws, sizeof(SpWs), st); break;
    case CC_DT_BF16: sp_launch<bf16_t>(logits, 1, V, V, tmax, k, seeds, input_pos, probs, idx_out, ws, sizeof(SpWs), st); break;
    default: sp_launch<f16_t>(logits, 1, V, V, tmax, k, seeds, input_pos, probs, idx_out, ws, sizeof(SpWs), st); break;
  }
  CC_LAUNCH_CHECK();
  return CC_OK;
}

extern "C" size_t cc_sample_nucleus_workspace_bytes(void) { return sizeof(SpNucWs); }

extern "C" int cc_sample_nucleus(const void* logits, int32_t V, int32_t dtype, float temperature, int32_t top_k, float top_p, float min_p,
                                 uint64_t seed, const int32_t* input_pos, void* probs, int32_t* idx_out, int32_t* n_kept_out,
                                 void* workspace, size_t workspace_bytes, cc_stream_t stream) {
  CC_ENTRY();
  SpSeeds seeds{};
  seeds.s[0] = seed;
  return spn_rows(logits, 1, V, V, dtype, temperature, top_k, top_p, min_p, seeds, input_pos, probs, idx_out, n_kept_out, workspace,
                  workspace_bytes, (hipStream_t)stream);
}

extern "C" size_t cc_sample_rows_workspace_bytes(int32_t T) { return T < 1 || T > CC_SAMPLE_MAX_ROWS ? 0 : (size_t)T * sizeof(SpNucWs); }

extern "C" int cc_sample_rows(const void* logits, int32_t T, int32_t V, int64_t row_stride, int32_t dtype, float temperature, int32_t top_k,
                              float top_p, float min_p, const uint64_t* seeds, const int32_t* input_pos, void* probs, int32_t* idx_out,
                              int32_t* n_kept_out, void* workspace, size_t workspace_bytes, cc_stream_t stream) {
  CC_ENTRY();
  if (T < 1 || T > CC_SAMPLE_MAX_ROWS || !seeds || row_stride < (int64_t)V) return CC_ERR_BAD_ARG;
  SpSeeds sd{};
  for (int r = 0; r < T; r++) sd.s[r] = seeds[r];  // by value: the caller's array is not read after the call returns
  return spn_rows(logits, T, V, (long long)row_stride, dtype, temperature, top_k, top_p, min_p, sd, input_pos, probs, idx_out, n_kept_out,
                  workspace, workspace_bytes, (hipStream_t)stream);
}

