// cc_penalty.hip — token-history state and the logit penalties in front of the sampling tail (include/coldcompress.h,
// cc_token_counts_add and cc_logits_penalize).  The state is two int32 histograms over the vocabulary and one position word, all in
// device memory, so a captured decode step advances through them.
//   counts_add  one thread per token: an integer atomicAdd into the histogram its position selects (exact in any order).
//   penalize    one thread per group of 16 bytes of the model dtype (4 fp32 / 8 16-bit elements) and all T rows of it: the group's
//               counts stay in registers while the rows go by, row t seeing the inputs of steps <= t.  No atomics, no workspace: an
//               element has one owner.  A group arrives as 16-byte loads where the base it is read from is 16-byte aligned and element
//               by element where it is not (row t of an odd V); the arithmetic is per element, so the bits do not depend on it.
//   penalize_streams  the same for T rows of DIFFERENT sequences (cc_logits_penalize_streams): grid (groups, T), blockIdx.y selects the
//               row's record (its own tables, gen_start, bias and settings, carried in the kernel arguments by value); the per-element
//               formula, the loads and the stores are penalize's own, so a row carries the bits penalize gives it at T = 1.
#include "cc_common.h"

namespace {
constexpr int kPenThreads = 256;

__global__ __launch_bounds__(kPenThreads) void token_counts_add_kernel(int32_t* prompt_count, int32_t* gen_count, int V,
                                                                       const int32_t* tokens, int n, int first_pos,
                                                                       const int32_t* gen_start) {
  const int i = blockIdx.x * kPenThreads + threadIdx.x;
  if (i >= n) return;
  const int tok = tokens[i];
  if (tok < 0 || tok >= V) return;  // (counts nothing: no address is formed from it)
  const bool gen = (long long)first_pos + i >= (long long)*gen_start;
  atomicAdd((gen ? gen_count : prompt_count) + tok, 1);
}

// elements [base, base + n) of the row as floats, n <= N (cc_logprob.hip's lp_group)
template <typename T>
__device__ __forceinline__ void pen_load(const T* row, int base, int n, bool aligned, float* x) {
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

// N 32-bit words from p[base ..): 16-byte loads where p is 16-byte aligned and the group is whole
template <int N, typename W>
__device__ __forceinline__ void pen_load_words(const W* p, int base, int n, bool aligned, W* w) {
  static_assert(sizeof(W) == 4 && N % 4 == 0, "groups of whole 16-byte vectors");
  if (aligned && n == N) {
#pragma unroll
    for (int q = 0; q < N / 4; q++) {
      const uint4 v = *reinterpret_cast<const uint4*>(p + base + 4 * q);
      const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; e++) __builtin_memcpy(&w[4 * q + e], &u[e], 4);
    }
  } else {
#pragma unroll
    for (int e = 0; e < N; e++)
      if (e < n) w[e] = p[base + e];
  }
}

// the group rounded to T (one rounding per element) and stored: one 16-byte store where the row's base allows it
template <typename T>
__device__ __forceinline__ void pen_store(T* row, int base, int n, bool aligned, const float* x) {
  constexpr int N = Vec16<T>::N;
  if (aligned && n == N) {
    uint32_t w[4];
    if constexpr (ElemTraits<T>::code == CC_DT_F32) {
#pragma unroll
      for (int e = 0; e < 4; e++) w[e] = __float_as_uint(x[e]);
    } else if constexpr (ElemTraits<T>::code == CC_DT_BF16) {
#pragma unroll
      for (int e = 0; e < 4; e++) w[e] = (uint32_t)f32_to_bf16_bits(x[2 * e]) | ((uint32_t)f32_to_bf16_bits(x[2 * e + 1]) << 16);
    } else {
#pragma unroll
      for (int e = 0; e < 4; e++) w[e] = (uint32_t)f32_to_f16_bits(x[2 * e]) | ((uint32_t)f32_to_f16_bits(x[2 * e + 1]) << 16);
    }
    *reinterpret_cast<uint4*>(row + base) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int e = 0; e < N; e++)
      if (e < n) ElemTraits<T>::store(row, (size_t)(base + e), x[e]);
  }
}

// the header's per-element formula on one group: x[e] penalised against (cp[e], cg[e]) and, with `biased`, b[e]
template <int N>
__device__ __forceinline__ void pen_group(float* x, const int32_t* cp, const int32_t* cg, const float* b, bool biased, int n, float r,
                                          float f, float p) {
#pragma unroll
  for (int e = 0; e < N; e++) {
    if (e < n) {
      float v = x[e];
      if (r != 1.0f && cp[e] + cg[e] > 0) v = v > 0.f ? __fdiv_rn(v, r) : __fmul_rn(v, r);
      if (f != 0.0f) v = __fsub_rn(v, cc_opaque_f32(__fmul_rn(f, (float)cg[e])));
      if (p != 0.0f && cg[e] > 0) v = __fsub_rn(v, p);
      if (biased) v = __fadd_rn(v, b[e]);
      x[e] = cc_opaque_f32(v);  // (fp32 first, then ONE rounding to T)
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kPenThreads) void logits_penalize_kernel(const T* logits, T* out, int T_rows, int V, long long row_stride,
                                                                      int32_t* prompt_count, int32_t* gen_count, const int32_t* tokens,
                                                                      const int32_t* pos, const int32_t* gen_start, float r, float f,
                                                                      float p, const float* bias) {
  constexpr int N = Vec16<T>::N;
  const long long g = (long long)blockIdx.x * kPenThreads + threadIdx.x;
  if (g * N >= (long long)V) return;
  const int base = (int)(g * N), n = min(N, V - base);
  int32_t cp[N], cg[N];
  float b[N];
  pen_load_words<N>(prompt_count, base, n, ((uintptr_t)prompt_count & 15u) == 0, cp);
  pen_load_words<N>(gen_count, base, n, ((uintptr_t)gen_count & 15u) == 0, cg);
  if (bias) pen_load_words<N>(bias, base, n, ((uintptr_t)bias & 15u) == 0, b);
  const int gs = *gen_start;
  unsigned int moved_p = 0u, moved_g = 0u;  // bit e: element e's count changed in this launch
  for (int t = 0; t < T_rows; t++) {
    if (tokens) {  // row t sees the inputs of steps <= t; a token outside [0, V) matches no element
      const int e = tokens[t] - base;
      if (e >= 0 && e < n) {
        const bool gen = pos[t] >= gs;
#pragma unroll
        for (int k = 0; k < N; k++) {
          if (k == e) {
            if (gen) cg[k] += 1;
            else cp[k] += 1;
          }
        }
        if (gen) moved_g |= 1u << e;
        else moved_p |= 1u << e;
      }
    }
    const T* row = logits + (size_t)t * (size_t)row_stride;
    T* orow = out + (size_t)t * (size_t)row_stride;
    float x[N];
    pen_load<T>(row, base, n, ((uintptr_t)row & 15u) == 0, x);
    pen_group<N>(x, cp, cg, b, bias != nullptr, n, r, f, p);
    pen_store<T>(orow, base, n, ((uintptr_t)orow & 15u) == 0, x);
  }
#pragma unroll
  for (int e = 0; e < N; e++) {  // stored only where it changed
    if (moved_p & (1u << e)) prompt_count[base + e] = cp[e];
    if (moved_g & (1u << e)) gen_count[base + e] = cg[e];
  }
}

template <typename T>
void pen_launch(const void* logits, void* out, int T_rows, int V, long long row_stride, int32_t* prompt_count, int32_t* gen_count,
                const int32_t* tokens, const int32_t* pos, const int32_t* gen_start, float r, float f, float p, const float* bias,
                hipStream_t st) {
  constexpr int N = Vec16<T>::N;
  const long long groups = ((long long)V + N - 1) / N;
  const unsigned int blocks = (unsigned int)((groups + kPenThreads - 1) / kPenThreads);
  hipLaunchKernelGGL(logits_penalize_kernel<T>, dim3(blocks), dim3(kPenThreads), 0, st, (const T*)logits, (T*)out, T_rows, V, row_stride,
                     prompt_count, gen_count, tokens, pos, gen_start, r, f, p, bias);
}
// ---- rows of DIFFERENT sequences (cc_logits_penalize_streams): blockIdx.y is the row and selects its record; a row's arithmetic is
//      the T = 1 launch's of logits_penalize_kernel on that record's state (pen_group, the same loads and stores)
struct PenRows {
  cc_penalty_row_t row[CC_GEMV_MULTI_MAX_T];
};

// elements [base, base + n) of a row as words of sizeof(U) bytes, bit for bit (no conversion: a NaN keeps its payload)
template <typename U>
__device__ __forceinline__ void pen_copy_bits(const void* row, void* orow, int base, int n) {
  constexpr int N = 16 / sizeof(U);
  const U* src = reinterpret_cast<const U*>(row);
  U* dst = reinterpret_cast<U*>(orow);
  if (n == N && (((uintptr_t)row | (uintptr_t)orow) & 15u) == 0) {
    *reinterpret_cast<uint4*>(dst + base) = *reinterpret_cast<const uint4*>(src + base);
  } else {
#pragma unroll
    for (int e = 0; e < N; e++)
      if (e < n) dst[base + e] = src[base + e];
  }
}

template <typename T>
__global__ __launch_bounds__(kPenThreads) void logits_penalize_streams_kernel(const T* logits, T* out, int V, long long row_stride,
                                                                              PenRows rows, const int32_t* tokens, const int32_t* pos) {
  constexpr int N = Vec16<T>::N;
  const long long g = (long long)blockIdx.x * kPenThreads + threadIdx.x;
  if (g * N >= (long long)V) return;
  const int base = (int)(g * N), n = min(N, V - base);
  const int t = blockIdx.y;
  const cc_penalty_row_t s = rows.row[t];
  const T* row = logits + (size_t)t * (size_t)row_stride;
  T* orow = out + (size_t)t * (size_t)row_stride;
  if (!s.prompt_count) {  // no penalties for this stream: the row's bits as they are
    if (orow == row) return;
    if constexpr (sizeof(T) == 4) pen_copy_bits<uint32_t>(row, orow, base, n);
    else pen_copy_bits<uint16_t>(row, orow, base, n);
    return;
  }
  int32_t cp[N], cg[N];
  float b[N];
  pen_load_words<N>(s.prompt_count, base, n, ((uintptr_t)s.prompt_count & 15u) == 0, cp);
  pen_load_words<N>(s.gen_count, base, n, ((uintptr_t)s.gen_count & 15u) == 0, cg);
  if (s.bias) pen_load_words<N>(s.bias, base, n, ((uintptr_t)s.bias & 15u) == 0, b);
  if (tokens) {  // the row's own input, counted before the row is computed; a token outside [0, V) matches no element
    const int e = tokens[t] - base;
    if (e >= 0 && e < n) {
      const bool gen = pos[t] >= *s.gen_start;
#pragma unroll
      for (int k = 0; k < N; k++) {
        if (k == e) {
          if (gen) cg[k] += 1;
          else cp[k] += 1;
        }
      }
      if (gen) s.gen_count[base + e] = cg[e];  // stored only where it changed: this one element
      else s.prompt_count[base + e] = cp[e];
    }
  }
  float x[N];
  pen_load<T>(row, base, n, ((uintptr_t)row & 15u) == 0, x);
  pen_group<N>(x, cp, cg, b, s.bias != nullptr, n, s.r, s.f, s.p);
  pen_store<T>(orow, base, n, ((uintptr_t)orow & 15u) == 0, x);
}

template <typename T>
void pen_streams_launch(const void* logits, void* out, int T_rows, int V, long long row_stride, const PenRows& rows, const int32_t* tokens,
                        const int32_t* pos, hipStream_t st) {
  constexpr int N = Vec16<T>::N;
  const long long groups = ((long long)V + N - 1) / N;
  const unsigned int blocks = (unsigned int)((groups + kPenThreads - 1) / kPenThreads);
  hipLaunchKernelGGL(logits_penalize_streams_kernel<T>, dim3(blocks, (unsigned int)T_rows), dim3(kPenThreads), 0, st, (const T*)logits,
                     (T*)out, V, row_stride, rows, tokens, pos);
}
}  // namespace

extern "C" int cc_token_counts_add(int32_t* prompt_count, int32_t* gen_count, int32_t V, const int32_t* tokens, int32_t n,
                                   int32_t first_pos, const int32_t* gen_start, cc_stream_t stream) {
  CC_ENTRY();
  if (!prompt_count || !gen_count || !gen_start || V <= 0 || n < 0 || (n > 0 && !tokens)) return CC_ERR_BAD_ARG;
  if ((((uintptr_t)prompt_count | (uintptr_t)gen_count | (uintptr_t)gen_start | (uintptr_t)tokens) & 3u) != 0) return CC_ERR_BAD_ARG;
  if (n == 0) return CC_OK;
  const unsigned int blocks = (unsigned int)(((long long)n + kPenThreads - 1) / kPenThreads);
  hipLaunchKernelGGL(token_counts_add_kernel, dim3(blocks), dim3(kPenThreads), 0, (hipStream_t)stream, prompt_count, gen_count, V, tokens, n,
                     first_pos, gen_start);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

extern "C" int cc_logits_penalize(const void* logits, void* out, int32_t T, int32_t V, int64_t row_stride, int32_t dtype,
                                  int32_t* prompt_count, int32_t* gen_count, const int32_t* tokens, const int32_t* pos,
                                  const int32_t* gen_start, float repetition_penalty, float frequency_penalty, float presence_penalty,
                                  const float* bias, cc_stream_t stream) {
  CC_ENTRY();
  if (!logits || !out || !prompt_count || !gen_count || !gen_start || (tokens && !pos) || T < 1 || T > CC_GEMV_MULTI_MAX_T || V <= 0 ||
      row_stride < (int64_t)V)
    return CC_ERR_BAD_ARG;
  if (!__builtin_isfinite(repetition_penalty) || !(repetition_penalty > 0.f) || !__builtin_isfinite(frequency_penalty) ||
      !__builtin_isfinite(presence_penalty))
    return CC_ERR_BAD_ARG;
  if (!cc_dt_ok(dtype)) return CC_ERR_UNSUPPORTED;
  if ((((uintptr_t)logits | (uintptr_t)out) & (cc_dt_size(dtype) - 1)) != 0 ||
      (((uintptr_t)prompt_count | (uintptr_t)gen_count | (uintptr_t)gen_start | (uintptr_t)tokens | (uintptr_t)pos | (uintptr_t)bias) & 3u) != 0)
    return CC_ERR_BAD_ARG;
  if (out != logits) {  // the same rows in place, or rows that share nothing
    const uintptr_t a = (uintptr_t)logits, b = (uintptr_t)out;
    const uintptr_t span = (uintptr_t)(((size_t)(T - 1) * (size_t)row_stride + (size_t)V) * cc_dt_size(dtype));
    if (a < b + span && b < a + span) return CC_ERR_BAD_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case CC_DT_F32:
      pen_launch<float>(logits, out, T, V, row_stride, prompt_count, gen_count, tokens, pos, gen_start, repetition_penalty,
                        frequency_penalty, presence_penalty, bias, st);
      break;
    case CC_DT_BF16:
      pen_launch<bf16_t>(logits, out, T, V, row_stride, prompt_count, gen_count, tokens, pos, gen_start, repetition_penalty,
                         frequency_penalty, presence_penalty, bias, st);
      break;
    default:
      pen_launch<f16_t>(logits, out, T, V, row_stride, prompt_count, gen_count, tokens, pos, gen_start, repetition_penalty,
                        frequency_penalty, presence_penalty, bias, st);
      break;
  }
  CC_LAUNCH_CHECK();
  return CC_OK;
}

extern "C" int cc_logits_penalize_streams(const void* logits, void* out, int32_t T, int32_t V, int64_t row_stride, int32_t dtype,
                                          const cc_penalty_row_t* rows, const int32_t* tokens, const int32_t* pos, cc_stream_t stream) {
  CC_ENTRY();
  if (!logits || !out || !rows || (tokens && !pos) || T < 1 || T > CC_GEMV_MULTI_MAX_T || V <= 0 || row_stride < (int64_t)V)
    return CC_ERR_BAD_ARG;
  PenRows pr{};
  for (int t = 0; t < T; t++) {  // cc_logits_penalize's refusals, per record; prompt_count NULL: no penalties for that row
    const cc_penalty_row_t& s = rows[t];
    if (!s.prompt_count) continue;
    if (!s.gen_count || !s.gen_start) return CC_ERR_BAD_ARG;
    if (!__builtin_isfinite(s.r) || !(s.r > 0.f) || !__builtin_isfinite(s.f) || !__builtin_isfinite(s.p)) return CC_ERR_BAD_ARG;
    if ((((uintptr_t)s.prompt_count | (uintptr_t)s.gen_count | (uintptr_t)s.gen_start | (uintptr_t)s.bias) & 3u) != 0) return CC_ERR_BAD_ARG;
    for (int u = 0; u < t; u++) {  // two rows on one table would race
      const cc_penalty_row_t& o = rows[u];
      if (o.prompt_count && (o.prompt_count == s.prompt_count || o.prompt_count == s.gen_count || o.gen_count == s.prompt_count ||
                             o.gen_count == s.gen_count))
        return CC_ERR_BAD_ARG;
    }
    pr.row[t] = s;
  }
  if (!cc_dt_ok(dtype)) return CC_ERR_UNSUPPORTED;
  if ((((uintptr_t)logits | (uintptr_t)out) & (cc_dt_size(dtype) - 1)) != 0 || (((uintptr_t)tokens | (uintptr_t)pos) & 3u) != 0)
    return CC_ERR_BAD_ARG;
  if (out != logits) {  // the same rows in place, or rows that share nothing
    const uintptr_t a = (uintptr_t)logits, b = (uintptr_t)out;
    const uintptr_t span = (uintptr_t)(((size_t)(T - 1) * (size_t)row_stride + (size_t)V) * cc_dt_size(dtype));
    if (a < b + span && b < a + span) return CC_ERR_BAD_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case CC_DT_F32:
      pen_streams_launch<float>(logits, out, T, V, row_stride, pr, tokens, pos, st);
      break;
    case CC_DT_BF16:
      pen_streams_launch<bf16_t>(logits, out, T, V, row_stride, pr, tokens, pos, st);
      break;
    default:
      pen_streams_launch<f16_t>(logits, out, T, V, row_stride, pr, tokens, pos, st);
      break;
  }
  CC_LAUNCH_CHECK();
  return CC_OK;
}
