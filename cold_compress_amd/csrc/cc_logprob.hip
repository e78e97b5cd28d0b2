// cc_logprob.hip — per-token log-probabilities of up to CC_LOGPROB_MAX_ROWS rows of logits (include/coldcompress.h, cc_logprob_rows):
// logprob = log_softmax(row)[target] in fp32 from the row's own values, the row's log-sum-exp, and the target's rank (how many
// logits are strictly larger).  The target of a row is read on the device — a forced token, or the token a sampler just wrote — so a
// captured step scores what it chose.  Two launches, every one a pure function of its row (no atomics on global memory, no tickets):
//   partial   grid (kLpSlices, T): the slice's maximum m_g, then s_g = sum of exp(x - m_g) and the count of x > x_t over the slice.
//             The slice is walked in groups of 16 bytes; group j belongs to thread j mod 256 and is summed in element order, whether it
//             arrives as one 16-byte load (the row's base is 16-byte aligned) or element by element (it is not): the same row gives the
//             same bits at any alignment, alone or as row r of T.
//   fold      T workgroups of one wave: M = max m_g, S = sum s_g * exp(m_g - M) in a fixed order, the counts, and the three results.
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

template <typename T>
__global__ __launch_bounds__(kLpThreads) void logprob_partial_kernel(const T* logits, int V, long long row_stride, const int32_t* targets,
                                                                     const int32_t* fallback, LpWs* ws) {
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
}

template <typename T>
__global__ __launch_bounds__(CC_WAVE) void logprob_fold_kernel(const T* logits, int V, long long row_stride, const int32_t* targets,
                                                               const int32_t* fallback, float* logprob, float* lse, int32_t* rank,
                                                               const LpWs* ws) {
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
  if (lane != 0) return;
  const float nan = __uint_as_float(0x7fc00000u);
  const float logS = logf(S);
  if (lse) lse[r] = __fadd_rn(M, logS);
  const int t = lp_target(targets, fallback, r, V);
  float lp = nan;
  int32_t rk = -1;
  if (t >= 0) {
    const float xt = ElemTraits<T>::load(logits + (size_t)r * (size_t)row_stride, (size_t)t);
    // a +inf in the row: exp(inf - inf) makes the softmax's sum NaN, and with it every element's log-probability (torch.log_softmax)
    if (M != INFINITY) lp = __fsub_rn(__fsub_rn(xt, M), logS);
    if (xt == xt) rk = (int32_t)above;
  }
  logprob[r] = lp;
  if (rank) rank[r] = rk;
}

template <typename T>
void lp_launch(const void* logits_, int T_rows, int V, long long row_stride, const int32_t* targets, const int32_t* fallback, float* logprob,
               float* lse, int32_t* rank, LpWs* ws, hipStream_t st) {
  const T* logits = (const T*)logits_;
  hipLaunchKernelGGL(logprob_partial_kernel<T>, dim3(kLpSlices, T_rows), dim3(kLpThreads), 0, st, logits, V, row_stride, targets, fallback, ws);
  hipLaunchKernelGGL(logprob_fold_kernel<T>, dim3(T_rows), dim3(CC_WAVE), 0, st, logits, V, row_stride, targets, fallback, logprob, lse, rank,
                     (const LpWs*)ws);
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
