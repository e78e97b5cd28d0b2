// cc_logprob.hip — per-token log-probabilities of up to CC_LOGPROB_MAX_ROWS rows of logits (include/coldcompress.h, cc_logprob_rows):
// logprob = log_softmax(row)[target] in fp32 from the row's own values, the row's log-sum-exp, and the target's rank (how many
// logits are strictly larger).  The target of a row is read on the device — a forced token, or the token a sampler just wrote — so a
// captured step scores what it chose.  Two launches, every one a pure function of its row (no atomics on global memory, no tickets):
//   partial   grid (kLpSlices, T): the slice's maximum m_g, then s_g = sum of exp(x - m_g) and the count of x > x_t over the slice.
//             The slice is walked in groups of 16 bytes; group j belongs to thread j mod 256 and is summed in element order, whether it
//             arrives as one 16-byte load (the row's base is 16-byte aligned) or element by element (it is not): the same row gives the
//             same bits at any alignment, alone or as row r of T.
//   fold      T workgroups of one wave: M = max m_g, S = sum s_g * exp(m_g - M) in a fixed order, the counts, and the three results.
// cc_logprob_topn adds the row's N best alternatives (N <= CC_LOGPROB_MAX_TOPN) to the same two launches.  Every non-NaN element has
// a 64-bit key, (its value as an orderable pattern, +0 and -0 alike) << 32 | ~index: a larger key comes earlier in the contract's total
// order and no two elements share one, so "the next in the order" is the largest key below the previous pick — no taken flags.
//   partial   as above (the same code: the three results keep their bits), then N rounds leave the slice's N largest keys, 0 where
//             the slice has no more, in the workspace: the whole top-N may sit in one slice.
//   fold      as above, then one wave merges the 128 sorted lists through LDS in N rounds, and lanes 0..N-1 write (id, (x_id - M) - log S)
//             with x_id read from the row itself, which is what the row's logprob is made of.
#include "cc_common.h"

namespace {
constexpr int kLpThreads = 256;
constexpr int kLpSlices = 128;
constexpr int kLpWaves = kLpThreads / CC_WAVE;

struct LpPart {
  float m, s;
  unsigned int above, pad;
};
struct LpWs {  // caller-provided scratch (cc_logprob_rows_workspace_bytes); row r's launch writes part[r] before its fold reads it
  LpPart part[CC_LOGPROB_MAX_ROWS][kLpSlices];
};
typedef unsigned long long lp_key_t;
struct LpTopWs {  // cc_logprob_topn_workspace_bytes: the partials, and per slice its N largest keys in descending order (0: no more)
  LpWs lp;
  lp_key_t cand[CC_LOGPROB_MAX_ROWS][kLpSlices][CC_LOGPROB_MAX_TOPN];
};

__device__ __forceinline__ void lp_slice(int V, int& lo, int& hi) {  // multiples of 8 elements: slice starts are 16 bytes apart
  const long long per = (((long long)V + kLpSlices - 1) / kLpSlices + 7) & ~7ll;
  lo = (int)min((long long)V, (long long)blockIdx.x * per);
  hi = (int)min((long long)V, (long long)lo + per);
}

// step 2 of the contract: the row's target, or -1 (none, or outside [0, V): no address is formed from it)
__device__ __forceinline__ int lp_target(const int32_t* targets, const int32_t* fallback, int r, int V) {
  int t = -1;
  if (targets) t = targets[r];
  if (t < 0 && fallback) t = fallback[r];
  return (t >= 0 && t < V) ? t : -1;
}

// elements [base, base + n) of the row as floats, n <= N; one 16-byte load for a whole group of an aligned row
template <typename T>
__device__ __forceinline__ void lp_group(const T* row, int base, int n, bool aligned, float* x) {
  constexpr int N = Vec16<T>::N;
  if (aligned && n == N) {
    Vec16<T> v;
    v.load(row + base);
    v.unpack(x);
  } else {
#pragma unroll
    for (int e = 0; e < N; e++)
      if (e < n) x[e] = ElemTraits<T>::load(row, (size_t)(base + e));
  }
}

// exp(x - m) of libm grade; exactly 1 at the maximum itself, also where the maximum is infinite (inf - inf is NaN)
__device__ __forceinline__ float lp_exp(float x, float m) { return x == m ? 1.0f : expf(__fsub_rn(x, m)); }

// the place of element (x, i) in the total order as a key: larger x first (+0 and -0 alike), then lower i; 0 for a NaN (never listed).
// The smallest key of a real element is -inf's, 0x007fffff << 32: 0 is free to mean "none".
__device__ __forceinline__ lp_key_t lp_key(float x, int i) {
  if (x != x) return 0ull;
  unsigned int u = x == 0.f ? 0u : __float_as_uint(x);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((lp_key_t)u << 32) | (lp_key_t)(0xffffffffu - (unsigned int)i);
}
__device__ __forceinline__ int lp_key_index(lp_key_t k) { return (int)(0xffffffffu - (unsigned int)(k & 0xffffffffull)); }
__device__ __forceinline__ lp_key_t lp_key_max(lp_key_t a, lp_key_t b) { return a > b ? a : b; }
// the key of another lane of the same row of 16 lanes, by a DPP move of each half (no trip through the LDS crossbar)
template <int kCtrl>
__device__ __forceinline__ lp_key_t lp_key_dpp(lp_key_t v) {
  const unsigned int lo = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)(unsigned int)v, kCtrl, 0xf, 0xf, false);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)(unsigned int)(v >> 32), kCtrl, 0xf, 0xf, false);
  return ((lp_key_t)hi << 32) | (lp_key_t)lo;
}
__device__ __forceinline__ lp_key_t lp_key_lane(lp_key_t v, int lane) {
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)v, lane);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(v >> 32), lane);
  return ((lp_key_t)hi << 32) | (lp_key_t)lo;
}
// The wave's largest key, uniform; all 64 lanes must be active.  A round of the selection is one of these and little else, so it
// stays off ds_bpermute: quad_perm [1,0,3,2] and [2,3,0,1] give every lane its quad's maximum, row_ror 4 and 8 its row's, and the
// four rows meet through v_readlane.
__device__ __forceinline__ lp_key_t wave_max_key(lp_key_t v) {
  v = lp_key_max(v, lp_key_dpp<0xb1>(v));
  v = lp_key_max(v, lp_key_dpp<0x4e>(v));
  v = lp_key_max(v, lp_key_dpp<0x124>(v));
  v = lp_key_max(v, lp_key_dpp<0x128>(v));
  return lp_key_max(lp_key_max(lp_key_lane(v, 0), lp_key_lane(v, 16)), lp_key_max(lp_key_lane(v, 32), lp_key_lane(v, 48)));
}

// kTop: cc_logprob_topn's launch, which goes on to the slice's `topn` largest keys (tws); the LpPart is the same code either way
template <typename T, bool kTop>
__global__ __launch_bounds__(kLpThreads) void logprob_partial_kernel(const T* logits, int V, long long row_stride, const int32_t* targets,
                                                                     const int32_t* fallback, LpWs* ws, int topn, LpTopWs* tws) {
  constexpr int N = Vec16<T>::N;
  __shared__ float s_f[kLpWaves];
  __shared__ unsigned int s_c[kLpWaves];
  __shared__ float s_xt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = blockIdx.y;
  const T* row = logits + (size_t)r * (size_t)row_stride;
  const bool aligned = ((uintptr_t)row & 15u) == 0;
  int lo, hi;
  lp_slice(V, lo, hi);
  if (threadIdx.x == 0) {
    const int t = lp_target(targets, fallback, r, V);
    s_xt = t >= 0 ? ElemTraits<T>::load(row, (size_t)t) : __uint_as_float(0x7fc00000u);  // (NaN: nothing compares greater)
  }
  __syncthreads();
  const float xt = s_xt;
  const int ngroups = (hi - lo + N - 1) / N;
  float first[N];  // the thread's first group stays in registers for the second walk (at V = 128256 no thread has another)
  float mx = -INFINITY;
  unsigned int above = 0u;
  for (int j = threadIdx.x; j < ngroups; j += kLpThreads) {
    const int base = lo + j * N, n = min(N, hi - base);
    float x[N];
    lp_group<T>(row, base, n, aligned, x);
#pragma unroll
    for (int e = 0; e < N; e++) {
      if (e < n) {
        mx = fmaxf(mx, x[e]);
        above += x[e] > xt ? 1u : 0u;
      }
      if (j == (int)threadIdx.x) first[e] = x[e];
    }
  }
  mx = wave_max_f32(mx);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) above += __shfl_xor(above, off, CC_WAVE);
  if (lane == 0) {
    s_f[wave] = mx;
    s_c[wave] = above;
  }
  __syncthreads();
  mx = fmaxf(fmaxf(s_f[0], s_f[1]), fmaxf(s_f[2], s_f[3]));  // (NaN never counts: fmaxf)
  above = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
  __syncthreads();
  float sum = 0.f;
  for (int j = threadIdx.x; j < ngroups; j += kLpThreads) {
    const int base = lo + j * N, n = min(N, hi - base);
    float x[N];
    if (j == (int)threadIdx.x) {
#pragma unroll
      for (int e = 0; e < N; e++) x[e] = first[e];
    } else {
      lp_group<T>(row, base, n, aligned, x);
    }
#pragma unroll
    for (int e = 0; e < N; e++)
      if (e < n) sum = __fadd_rn(sum, lp_exp(x[e], mx));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum = __fadd_rn(sum, __shfl_xor(sum, off, CC_WAVE));
  if (lane == 0) s_f[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {  // an empty slice leaves (-inf, 0, 0): it contributes nothing
    LpPart p;
    p.m = mx;
    p.s = (s_f[0] + s_f[1]) + (s_f[2] + s_f[3]);
    p.above = above;
    p.pad = 0u;
    ws->part[r][blockIdx.x] = p;
  }
  if constexpr (kTop) {
    // round j: the largest key of the slice below round j - 1's pick.  The thread's first group waits in registers as keys;
    // a further group (V > 128 * 256 * N) is read again
    __shared__ lp_key_t s_k[2][kLpWaves];
    lp_key_t kf[N];
#pragma unroll
    for (int e = 0; e < N; e++) {
      const int i = lo + (int)threadIdx.x * N + e;
      kf[e] = ((int)threadIdx.x < ngroups && i < hi) ? lp_key(first[e], i) : 0ull;
    }
    lp_key_t prev = ~0ull, mine = 0ull;
    for (int j = 0; j < topn; j++) {
      lp_key_t best = 0ull;
#pragma unroll
      for (int e = 0; e < N; e++)
        if (kf[e] < prev) best = lp_key_max(best, kf[e]);
      for (int g = threadIdx.x + kLpThreads; g < ngroups; g += kLpThreads) {
        const int base = lo + g * N, n = min(N, hi - base);
        float x[N];
        lp_group<T>(row, base, n, aligned, x);
#pragma unroll
        for (int e = 0; e < N; e++) {
          const lp_key_t k = e < n ? lp_key(x[e], base + e) : 0ull;
          if (k < prev) best = lp_key_max(best, k);
        }
      }
      best = wave_max_key(best);
      if (lane == 0) s_k[j & 1][wave] = best;
      __syncthreads();  // (two buffers: round j + 1's barrier stands between these reads and round j + 2's writes)
      prev = lp_key_max(lp_key_max(s_k[j & 1][0], s_k[j & 1][1]), lp_key_max(s_k[j & 1][2], s_k[j & 1][3]));
      if ((int)threadIdx.x == j) mine = prev;  // (0 once the slice is exhausted, and from then on)
    }
    // thread j kept round j's pick: one coalesced store behind the rounds
    if ((int)threadIdx.x < topn) tws->cand[r][blockIdx.x][threadIdx.x] = mine;
  }
}

// the fold of one row by one wave: lane 0 writes the three results (each may be NULL); M and log S are returned in every lane
struct LpFolded {
  float M, logS;
};
template <typename T>
__device__ __forceinline__ LpFolded lp_fold_row(const T* logits, int V, long long row_stride, const int32_t* targets, const int32_t* fallback,
                                                float* logprob, float* lse, int32_t* rank, const LpWs* ws) {
  static_assert(kLpSlices == 2 * CC_WAVE, "lane l folds slices l and l + 64");
  const int lane = threadIdx.x, r = blockIdx.x;
  const LpPart a = ws->part[r][lane], b = ws->part[r][lane + CC_WAVE];
  const float M = wave_max_f32(fmaxf(a.m, b.m));
  float S = 0.f;  // (s == 0: an empty slice, or one of -inf alone under a larger maximum; a NaN sum is kept)
  if (a.s != 0.f) S = __fmul_rn(a.s, lp_exp(a.m, M));
  if (b.s != 0.f) S = __fadd_rn(S, __fmul_rn(b.s, lp_exp(b.m, M)));
  unsigned int above = a.above + b.above;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    S = __fadd_rn(S, __shfl_xor(S, off, CC_WAVE));
    above += __shfl_xor(above, off, CC_WAVE);
  }
  LpFolded f;
  f.M = M;
  f.logS = logf(S);  // (the butterfly leaves the same S in every lane)
  if (lane != 0) return f;
  const float nan = __uint_as_float(0x7fc00000u);
  if (lse) lse[r] = __fadd_rn(M, f.logS);
  const int t = lp_target(targets, fallback, r, V);
  float lp = nan;
  int32_t rk = -1;
  if (t >= 0) {
    const float xt = ElemTraits<T>::load(logits + (size_t)r * (size_t)row_stride, (size_t)t);
    // a +inf in the row: exp(inf - inf) makes the softmax's sum NaN, and with it every element's log-probability (torch.log_softmax)
    if (M != INFINITY) lp = __fsub_rn(__fsub_rn(xt, M), f.logS);
    if (xt == xt) rk = (int32_t)above;
  }
  if (logprob) logprob[r] = lp;
  if (rank) rank[r] = rk;
  return f;
}

template <typename T>
__global__ __launch_bounds__(CC_WAVE) void logprob_fold_kernel(const T* logits, int V, long long row_stride, const int32_t* targets,
                                                               const int32_t* fallback, float* logprob, float* lse, int32_t* rank,
                                                               const LpWs* ws) {
  lp_fold_row<T>(logits, V, row_stride, targets, fallback, logprob, lse, rank, ws);
}

// the fold, then the merge of the row's 128 sorted candidate lists: lane l holds the heads of slices l and l + 64; round j's winner is
// the wave's largest head, and the lane that held it moves on in that list
template <typename T>
__global__ __launch_bounds__(CC_WAVE) void logprob_topn_fold_kernel(const T* logits, int V, long long row_stride, const int32_t* targets,
                                                                    const int32_t* fallback, int topn, float* logprob, float* lse,
                                                                    int32_t* rank, int32_t* top_ids, float* top_logprobs,
                                                                    const LpTopWs* tws) {
  __shared__ lp_key_t s_c[kLpSlices * CC_LOGPROB_MAX_TOPN];
  const int lane = threadIdx.x, r = blockIdx.x;
  // the lane's two lists, every load in flight before the first is waited for (a loop of load-then-store pays the whole latency
  // of a global load per trip: 40 trips at N = 20), then into LDS, where the merge can index them
  lp_key_t ra[CC_LOGPROB_MAX_TOPN], rb[CC_LOGPROB_MAX_TOPN];
#pragma unroll
  for (int j = 0; j < CC_LOGPROB_MAX_TOPN; j++) {
    ra[j] = j < topn ? tws->cand[r][lane][j] : 0ull;
    rb[j] = j < topn ? tws->cand[r][lane + CC_WAVE][j] : 0ull;
  }
  const LpFolded f = lp_fold_row<T>(logits, V, row_stride, targets, fallback, logprob, lse, rank, &tws->lp);
  lp_key_t* la = s_c + lane * topn;
  lp_key_t* lb = s_c + (lane + CC_WAVE) * topn;
#pragma unroll
  for (int j = 0; j < CC_LOGPROB_MAX_TOPN; j++)
    if (j < topn) {
      la[j] = ra[j];
      lb[j] = rb[j];
    }
  __syncthreads();
  int pa = 0, pb = 0;
  lp_key_t ka = la[0], kb = lb[0], mine = 0ull;
  for (int j = 0; j < topn; j++) {
    const lp_key_t w = wave_max_key(lp_key_max(ka, kb));
    if (lane == j) mine = w;
    if (w == 0ull) break;  // (uniform: fewer than N non-NaN elements in the row)
    if (ka == w) {
      pa++;
      ka = pa < topn ? la[pa] : 0ull;
    } else if (kb == w) {
      pb++;
      kb = pb < topn ? lb[pb] : 0ull;
    }
  }
  if (lane >= topn) return;
  int32_t id = -1;
  float lp = __uint_as_float(0x7fc00000u);
  if (mine != 0ull) {
    id = lp_key_index(mine);
    const float x = ElemTraits<T>::load(logits + (size_t)r * (size_t)row_stride, (size_t)id);
    if (f.M != INFINITY) lp = __fsub_rn(__fsub_rn(x, f.M), f.logS);
  }
  top_ids[(size_t)r * topn + lane] = id;
  top_logprobs[(size_t)r * topn + lane] = lp;
}

template <typename T>
void lp_launch(const void* logits_, int T_rows, int V, long long row_stride, const int32_t* targets, const int32_t* fallback, float* logprob,
               float* lse, int32_t* rank, LpWs* ws, hipStream_t st) {
  const T* logits = (const T*)logits_;
  hipLaunchKernelGGL((logprob_partial_kernel<T, false>), dim3(kLpSlices, T_rows), dim3(kLpThreads), 0, st, logits, V, row_stride, targets, fallback, ws,
                     0, (LpTopWs*)nullptr);
  hipLaunchKernelGGL(logprob_fold_kernel<T>, dim3(T_rows), dim3(CC_WAVE), 0, st, logits, V, row_stride, targets, fallback, logprob, lse, rank,
                     (const LpWs*)ws);
}

template <typename T>
void lp_topn_launch(const void* logits_, int T_rows, int V, long long row_stride, const int32_t* targets, const int32_t* fallback, int topn,
                    float* logprob, float* lse, int32_t* rank, int32_t* top_ids, float* top_logprobs, LpTopWs* tws, hipStream_t st) {
  const T* logits = (const T*)logits_;
  hipLaunchKernelGGL((logprob_partial_kernel<T, true>), dim3(kLpSlices, T_rows), dim3(kLpThreads), 0, st, logits, V, row_stride, targets, fallback,
                     &tws->lp, topn, tws);
  hipLaunchKernelGGL(logprob_topn_fold_kernel<T>, dim3(T_rows), dim3(CC_WAVE), 0, st, logits, V, row_stride, targets, fallback, topn, logprob, lse,
                     rank, top_ids, top_logprobs, (const LpTopWs*)tws);
}
}  // namespace

extern "C" size_t cc_logprob_rows_workspace_bytes(void) { return sizeof(LpWs); }

extern "C" int cc_logprob_rows(const void* logits, int32_t T, int32_t V, int64_t row_stride, int32_t dtype, const int32_t* targets,
                               const int32_t* fallback, float* logprob, float* lse, int32_t* rank, void* workspace, size_t workspace_bytes,
                               cc_stream_t stream) {
  CC_ENTRY();
  if (!logits || !logprob || !workspace || T < 1 || T > CC_LOGPROB_MAX_ROWS || V < 1 || row_stride < (int64_t)V || !cc_dt_ok(dtype))
    return CC_ERR_BAD_ARG;
  if (workspace_bytes < sizeof(LpWs)) return CC_ERR_WORKSPACE;
  if (((uintptr_t)workspace & 15u) != 0 || ((uintptr_t)logits & (cc_dt_size(dtype) - 1)) != 0) return CC_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  LpWs* ws = reinterpret_cast<LpWs*>(workspace);
  switch (dtype) {
    case CC_DT_F32: lp_launch<float>(logits, T, V, row_stride, targets, fallback, logprob, lse, rank, ws, st); break;
    case CC_DT_BF16: lp_launch<bf16_t>(logits, T, V, row_stride, targets, fallback, logprob, lse, rank, ws, st); break;
    default: lp_launch<f16_t>(logits, T, V, row_stride, targets, fallback, logprob, lse, rank, ws, st); break;
  }
  CC_LAUNCH_CHECK();
  return CC_OK;
}

extern "C" size_t cc_logprob_topn_workspace_bytes(void) { return sizeof(LpTopWs); }

extern "C" int cc_logprob_topn(const void* logits, int32_t T, int32_t V, int64_t row_stride, int32_t dtype, const int32_t* targets,
                               const int32_t* fallback, int32_t N, float* logprob, float* lse, int32_t* rank, int32_t* top_ids,
                               float* top_logprobs, void* workspace, size_t workspace_bytes, cc_stream_t stream) {
  CC_ENTRY();
  if (!logits || !top_ids || !top_logprobs || !workspace || N < 1 || N > CC_LOGPROB_MAX_TOPN || T < 1 || T > CC_LOGPROB_MAX_ROWS || V < 1 ||
      row_stride < (int64_t)V || !cc_dt_ok(dtype))
    return CC_ERR_BAD_ARG;
  if (workspace_bytes < sizeof(LpTopWs)) return CC_ERR_WORKSPACE;
  if (((uintptr_t)workspace & 15u) != 0 || ((uintptr_t)logits & (cc_dt_size(dtype) - 1)) != 0) return CC_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  LpTopWs* tws = reinterpret_cast<LpTopWs*>(workspace);
  switch (dtype) {
    case CC_DT_F32: lp_topn_launch<float>(logits, T, V, row_stride, targets, fallback, N, logprob, lse, rank, top_ids, top_logprobs, tws, st); break;
    case CC_DT_BF16: lp_topn_launch<bf16_t>(logits, T, V, row_stride, targets, fallback, N, logprob, lse, rank, top_ids, top_logprobs, tws, st); break;
    default: lp_topn_launch<f16_t>(logits, T, V, row_stride, targets, fallback, N, logprob, lse, rank, top_ids, top_logprobs, tws, st); break;
  }
  CC_LAUNCH_CHECK();
  return CC_OK;
}
