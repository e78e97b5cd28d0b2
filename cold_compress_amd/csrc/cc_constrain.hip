// cc_constrain.hip — sequence rules in front of the sampling tail (include/coldcompress.h, cc_token_history_write and
// cc_logits_constrain): n-gram blocking, banned sequences and a minimum length.  The state is the POSITIONAL token history hist[cap]
// in device memory (hist[q] = the input token at position q), so a captured decode step advances through it, and a step reads only
// positions in front of its own: nothing has to be put back behind a rewind.
//   history_write  one thread per token: hist[first_pos + i] = tokens[i] where that position is inside [0, cap).
//   copy           (out != logits only) one thread per group of 16 bytes and row: the bits as they are, 16 bytes at a time where the
//                  base is 16-byte aligned, element by element where it is not.
//   ban            grid (slices + 1, T).  A workgroup x < slices walks slices x, x + slices, .. of CC_CONSTRAIN_SLICE candidate starts
//                  of row blockIdx.y: a thread compares the LAST element of the candidate's prefix with the tail's (a cheap reject),
//                  then the rest against the tail held in LDS, and on a match stores -inf to the element the candidate continues
//                  with.  The last workgroup of a row does the terminators and the banned sequences, and that of row 0 stores the T
//                  history words.  Several threads may store -inf to one element: the same value, so no atomics; no workgroup waits
//                  for another.
//   ban_streams    the ban pass for T rows of DIFFERENT sequences (cc_logits_constrain_streams): grid (largest slice count of the rows
//                  + 1, T), blockIdx.y selects the row's record (its own history, cap, gen_start and rules, carried in the kernel
//                  arguments by value) and the row sits at its own pos[t]; both passes end in con_row, the bans of one row.
// A token read from hist or tokens is compared as an integer and becomes an address only behind the [0, V) check.
#include "cc_common.h"

namespace {
constexpr int kConThreads = 256;
constexpr int kConMaxSlices = 1024;  // (workgroups per row: longer histories are walked in strides)

__global__ __launch_bounds__(kConThreads) void token_history_write_kernel(int32_t* hist, int cap, const int32_t* tokens, int n,
                                                                          int first_pos) {
  const int i = blockIdx.x * kConThreads + threadIdx.x;
  if (i >= n) return;
  const long long q = (long long)first_pos + i;
  if (q < 0 || q >= (long long)cap) return;
  hist[q] = tokens[i];
}

// T rows of V elements of sizeof(U) bytes, bit for bit
template <typename U>
__global__ __launch_bounds__(kConThreads) void constrain_copy_kernel(const U* src, U* dst, int V, long long row_stride) {
  constexpr int N = 16 / sizeof(U);
  const long long g = (long long)blockIdx.x * kConThreads + threadIdx.x;
  if (g * N >= (long long)V) return;
  const int base = (int)(g * N), n = min(N, V - base);
  const U* row = src + (size_t)blockIdx.y * (size_t)row_stride;
  U* orow = dst + (size_t)blockIdx.y * (size_t)row_stride;
  U w[N];
  if (n == N && ((uintptr_t)row & 15u) == 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(row + base);
    __builtin_memcpy(w, &v, 16);
  } else {
#pragma unroll
    for (int e = 0; e < N; e++)
      if (e < n) w[e] = row[base + e];
  }
  if (n == N && ((uintptr_t)orow & 15u) == 0) {
    uint4 v;
    __builtin_memcpy(&v, w, 16);
    *reinterpret_cast<uint4*>(orow + base) = v;
  } else {
#pragma unroll
    for (int e = 0; e < N; e++)
      if (e < n) orow[base + e] = w[e];
  }
}

template <typename U>
__device__ __forceinline__ U con_neg_inf();
template <>
__device__ __forceinline__ uint32_t con_neg_inf<uint32_t>() { return 0xff800000u; }
struct con_bf16 { uint16_t x; };
struct con_f16 { uint16_t x; };
template <>
__device__ __forceinline__ con_bf16 con_neg_inf<con_bf16>() { return con_bf16{0xff80}; }
template <>
__device__ __forceinline__ con_f16 con_neg_inf<con_f16>() { return con_f16{0xfc00}; }

struct ConArgs {
  int T, V, cap, ngram, ngram_from_gen, min_new_tokens, n_term, n_bw, slices;
  long long row_stride;
  int32_t* hist;
  const int32_t *tokens, *pos, *gen_start, *term_ids, *bw_tokens, *bw_offsets;
};

// element j of the history of the block's rows: hist in front of the block, the block's own inputs from pos0 on
__device__ __forceinline__ int con_elem(const ConArgs& a, int pos0, long long j) {
  return (a.tokens && j >= (long long)pos0) ? a.tokens[j - pos0] : a.hist[j];
}

// The bans of ONE row at position p of the sequence `a` describes (a.tokens: the inputs from position pos0 on), by the workgroup x of
// a.slices + 1 that work on the row: both entry points' kernels end here, so a row's bits are the same from either.
template <typename U>
__device__ __forceinline__ void con_row(U* row, const ConArgs& a, int pos0, long long p, int x, int* tail) {
  const bool misc = x == a.slices;
  if (p < 0 || p >= (long long)a.cap) return;  // (block-uniform) a position outside the history: the row stays as it is
  const U ninf = con_neg_inf<U>();
  if (misc) {
    const long long gs = a.gen_start[0];
    if (p + 1 - gs < (long long)a.min_new_tokens) {
      for (int k = threadIdx.x; k < a.n_term; k += kConThreads) {
        const int w = a.term_ids[k];
        if (w >= 0 && w < a.V) row[w] = ninf;
      }
    }
    for (int b = threadIdx.x; b < a.n_bw; b += kConThreads) {  // one banned sequence per thread
      const int o0 = a.bw_offsets[b], o1 = a.bw_offsets[b + 1];
      const int k = o1 - o0 - 1;  // the prefix's length
      if (o0 < 0 || k < 0 || k >= CC_CONSTRAIN_MAX_NGRAM || o1 > CC_CONSTRAIN_MAX_BW_TOKENS || (long long)k > p + 1) continue;
      bool same = true;
      for (int e = k - 1; e >= 0 && same; e--) same = con_elem(a, pos0, p - k + 1 + e) == a.bw_tokens[o0 + e];
      if (!same) continue;
      const int w = a.bw_tokens[o0 + k];
      if (w >= 0 && w < a.V) row[w] = ninf;
    }
    return;
  }
  // n-gram blocking: candidates i0 <= i <= p - n + 1 whose n - 1 elements equal the tail s[p-n+2 .. p] ban s[i+n-1]
  const int n = a.ngram;
  long long i0 = 0;
  if (a.ngram_from_gen) {
    i0 = a.gen_start[0];
    if (i0 < 0) i0 = 0;
  }
  const long long last = p - n + 1;
  if (last < i0) return;  // (block-uniform: in front of the barrier)
  if ((int)threadIdx.x < n - 1) tail[threadIdx.x] = con_elem(a, pos0, p - n + 2 + threadIdx.x);
  __syncthreads();
  for (long long s0 = i0 + (long long)x * CC_CONSTRAIN_SLICE; s0 <= last; s0 += (long long)a.slices * CC_CONSTRAIN_SLICE) {
#pragma unroll
    for (int c = 0; c < CC_CONSTRAIN_SLICE / kConThreads; c++) {
      const long long i = s0 + c * kConThreads + threadIdx.x;
      if (i > last) continue;
      bool same = n < 2 || con_elem(a, pos0, i + n - 2) == tail[n - 2];
      for (int e = n - 3; e >= 0 && same; e--) same = con_elem(a, pos0, i + e) == tail[e];
      if (!same) continue;
      const int w = con_elem(a, pos0, i + n - 1);
      if (w >= 0 && w < a.V) row[w] = ninf;
    }
  }
}

template <typename U>
__global__ __launch_bounds__(kConThreads) void logits_constrain_kernel(U* out, ConArgs a) {
  __shared__ int tail[CC_CONSTRAIN_MAX_NGRAM];
  const int t = blockIdx.y, pos0 = a.pos[0];
  const long long p = (long long)pos0 + t;  // the row's position: its history is s[0 .. p]
  if ((int)blockIdx.x == a.slices && t == 0 && a.tokens && (int)threadIdx.x < a.T) {  // hist[pos0 + k] = tokens[k]: positions no row of
    const long long q = (long long)pos0 + threadIdx.x;                                // this launch reads from hist
    if (q >= 0 && q < (long long)a.cap) a.hist[q] = a.tokens[threadIdx.x];
  }
  con_row<U>(out + (size_t)t * (size_t)a.row_stride, a, pos0, p, (int)blockIdx.x, tail);
}

template <typename U>
void con_launch(void* out, const ConArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(logits_constrain_kernel<U>, dim3((unsigned int)a.slices + 1u, (unsigned int)a.T), dim3(kConThreads), 0, st, (U*)out, a);
}

// ---- rows of DIFFERENT sequences (cc_logits_constrain_streams): blockIdx.y is the row and selects its record; the row sits at its own
//      position pos[t] over its own history, whose last element is tokens[t].  The grid's x extent is the largest slice count of the
//      rows + 1; a row with fewer slices lets the workgroups it has no use for return, and its last workgroup in use does the rest.
struct ConRows {
  cc_constraint_row_t row[CC_GEMV_MULTI_MAX_T];
};

__host__ __device__ __forceinline__ int con_slices(int cap, int ngram) {  // (from cap, not *pos: a captured launch keeps its grid as the
  const long long slices = ((long long)cap + CC_CONSTRAIN_SLICE - 1) / CC_CONSTRAIN_SLICE;  //  history grows)
  return ngram > 0 ? (int)(slices < kConMaxSlices ? slices : kConMaxSlices) : 0;
}

template <typename U>
__global__ __launch_bounds__(kConThreads) void logits_constrain_streams_kernel(U* out, int V, long long row_stride, ConRows rows,
                                                                               const int32_t* tokens, const int32_t* pos) {
  __shared__ int tail[CC_CONSTRAIN_MAX_NGRAM];
  const int t = blockIdx.y;
  const cc_constraint_row_t s = rows.row[t];
  if (!s.hist) return;  // no rules for this stream: the row as it is
  ConArgs a;
  a.T = 1, a.V = V, a.cap = s.cap, a.ngram = s.ngram, a.ngram_from_gen = s.ngram_from_gen, a.min_new_tokens = s.min_new_tokens;
  a.n_term = s.min_new_tokens > 0 ? s.n_term : 0, a.n_bw = s.n_bw, a.slices = con_slices(s.cap, s.ngram);
  a.row_stride = row_stride, a.hist = s.hist, a.tokens = tokens ? tokens + t : nullptr, a.pos = pos + t, a.gen_start = s.gen_start;
  a.term_ids = s.term_ids, a.bw_tokens = s.bw_tokens, a.bw_offsets = s.bw_offsets;
  if ((int)blockIdx.x > a.slices) return;  // (block-uniform) more workgroups than this row's history has slices
  const int pos0 = pos[t];
  if ((int)blockIdx.x == a.slices && tokens && threadIdx.x == 0 && pos0 >= 0 && pos0 < s.cap) s.hist[pos0] = tokens[t];
  con_row<U>(out + (size_t)t * (size_t)row_stride, a, pos0, (long long)pos0, (int)blockIdx.x, tail);
}

template <typename U>
void con_streams_launch(void* out, int T, int V, long long row_stride, const ConRows& rows, int slices, const int32_t* tokens,
                        const int32_t* pos, hipStream_t st) {
  hipLaunchKernelGGL(logits_constrain_streams_kernel<U>, dim3((unsigned int)slices + 1u, (unsigned int)T), dim3(kConThreads), 0, st,
                     (U*)out, V, row_stride, rows, tokens, pos);
}

template <typename U>
void con_copy_launch(const void* logits, void* out, int T, int V, long long row_stride, hipStream_t st) {
  constexpr int N = 16 / sizeof(U);
  const long long groups = ((long long)V + N - 1) / N;
  const unsigned int blocks = (unsigned int)((groups + kConThreads - 1) / kConThreads);
  hipLaunchKernelGGL(constrain_copy_kernel<U>, dim3(blocks, (unsigned int)T), dim3(kConThreads), 0, st, (const U*)logits, (U*)out, V, row_stride);
}
}  // namespace

extern "C" int cc_token_history_write(int32_t* hist, int32_t cap, const int32_t* tokens, int32_t n, int32_t first_pos, cc_stream_t stream) {
  CC_ENTRY();
  if (!hist || cap <= 0 || n < 0 || (n > 0 && !tokens)) return CC_ERR_BAD_ARG;
  if ((((uintptr_t)hist | (uintptr_t)tokens) & 3u) != 0) return CC_ERR_BAD_ARG;
  if (n == 0) return CC_OK;
  const unsigned int blocks = (unsigned int)(((long long)n + kConThreads - 1) / kConThreads);
  hipLaunchKernelGGL(token_history_write_kernel, dim3(blocks), dim3(kConThreads), 0, (hipStream_t)stream, hist, cap, tokens, n, first_pos);
  CC_LAUNCH_CHECK();
  return CC_OK;
}

extern "C" int cc_logits_constrain(const void* logits, void* out, int32_t T, int32_t V, int64_t row_stride, int32_t dtype, int32_t* hist,
                                   int32_t cap, const int32_t* tokens, const int32_t* pos, const int32_t* gen_start, int32_t ngram,
                                   int32_t ngram_from_gen, int32_t min_new_tokens, const int32_t* term_ids, int32_t n_term,
                                   const int32_t* bw_tokens, const int32_t* bw_offsets, int32_t n_bw, cc_stream_t stream) {
  CC_ENTRY();
  if (!logits || !out || !hist || !pos || !gen_start || T < 1 || T > CC_GEMV_MULTI_MAX_T || V <= 0 || row_stride < (int64_t)V || cap <= 0)
    return CC_ERR_BAD_ARG;
  if (ngram < 0 || ngram > CC_CONSTRAIN_MAX_NGRAM || min_new_tokens < 0 || n_term < 0 || n_term > CC_CONSTRAIN_MAX_TERMINATORS ||
      (n_term > 0 && !term_ids) || n_bw < 0 || n_bw > CC_CONSTRAIN_MAX_BW || (n_bw > 0 && (!bw_tokens || !bw_offsets)))
    return CC_ERR_BAD_ARG;
  if ((((uintptr_t)hist | (uintptr_t)tokens | (uintptr_t)pos | (uintptr_t)gen_start | (uintptr_t)term_ids | (uintptr_t)bw_tokens |
        (uintptr_t)bw_offsets) & 3u) != 0)
    return CC_ERR_BAD_ARG;
  const size_t esz = cc_dt_ok(dtype) ? cc_dt_size(dtype) : 2;  // (an unknown dtype: the smallest element, so that every bad argument
  if ((((uintptr_t)logits | (uintptr_t)out) & (esz - 1)) != 0) return CC_ERR_BAD_ARG;  //  is named before the dtype)
  if (out != logits) {  // the same rows in place, or rows that share nothing
    const uintptr_t a = (uintptr_t)logits, b = (uintptr_t)out;
    const uintptr_t span = (uintptr_t)(((size_t)(T - 1) * (size_t)row_stride + (size_t)V) * esz);
    if (a < b + span && b < a + span) return CC_ERR_BAD_ARG;
  }
  if (!cc_dt_ok(dtype)) return CC_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (out != logits) {
    if (dtype == CC_DT_F32) con_copy_launch<uint32_t>(logits, out, T, V, row_stride, st);
    else con_copy_launch<uint16_t>(logits, out, T, V, row_stride, st);
    CC_LAUNCH_CHECK();
  }
  ConArgs a;
  a.T = T, a.V = V, a.cap = cap, a.ngram = ngram, a.ngram_from_gen = ngram_from_gen != 0, a.min_new_tokens = min_new_tokens;
  a.n_term = min_new_tokens > 0 ? n_term : 0, a.n_bw = n_bw;
  a.slices = con_slices(cap, ngram);
  a.row_stride = row_stride, a.hist = hist, a.tokens = tokens, a.pos = pos, a.gen_start = gen_start, a.term_ids = term_ids;
  a.bw_tokens = bw_tokens, a.bw_offsets = bw_offsets;
  switch (dtype) {
    case CC_DT_F32:
      con_launch<uint32_t>(out, a, st);
      break;
    case CC_DT_BF16:
      con_launch<con_bf16>(out, a, st);
      break;
    default:
      con_launch<con_f16>(out, a, st);
      break;
  }
  CC_LAUNCH_CHECK();
  return CC_OK;
}

extern "C" int cc_logits_constrain_streams(const void* logits, void* out, int32_t T, int32_t V, int64_t row_stride, int32_t dtype,
                                           const cc_constraint_row_t* rows, const int32_t* tokens, const int32_t* pos, cc_stream_t stream) {
  CC_ENTRY();
  if (!logits || !out || !rows || !pos || T < 1 || T > CC_GEMV_MULTI_MAX_T || V <= 0 || row_stride < (int64_t)V) return CC_ERR_BAD_ARG;
  ConRows cr{};
  int slices = 0;
  for (int t = 0; t < T; t++) {  // cc_logits_constrain's refusals, per record; hist NULL: no rules for that row
    const cc_constraint_row_t& s = rows[t];
    if (!s.hist) continue;
    if (!s.gen_start || s.cap <= 0) return CC_ERR_BAD_ARG;
    if (s.ngram < 0 || s.ngram > CC_CONSTRAIN_MAX_NGRAM || s.min_new_tokens < 0 || s.n_term < 0 || s.n_term > CC_CONSTRAIN_MAX_TERMINATORS ||
        (s.n_term > 0 && !s.term_ids) || s.n_bw < 0 || s.n_bw > CC_CONSTRAIN_MAX_BW || (s.n_bw > 0 && (!s.bw_tokens || !s.bw_offsets)))
      return CC_ERR_BAD_ARG;
    if ((((uintptr_t)s.hist | (uintptr_t)s.gen_start | (uintptr_t)s.term_ids | (uintptr_t)s.bw_tokens | (uintptr_t)s.bw_offsets) & 3u) != 0)
      return CC_ERR_BAD_ARG;
    for (int u = 0; u < t; u++)  // two rows on one history would race
      if (rows[u].hist == s.hist) return CC_ERR_BAD_ARG;
    cr.row[t] = s;
    cr.row[t].ngram_from_gen = s.ngram_from_gen != 0;
    const int sl = con_slices(s.cap, s.ngram);
    slices = sl > slices ? sl : slices;
  }
  if ((((uintptr_t)tokens | (uintptr_t)pos) & 3u) != 0) return CC_ERR_BAD_ARG;
  const size_t esz = cc_dt_ok(dtype) ? cc_dt_size(dtype) : 2;  // (an unknown dtype: the smallest element, so that every bad argument
  if ((((uintptr_t)logits | (uintptr_t)out) & (esz - 1)) != 0) return CC_ERR_BAD_ARG;  //  is named before the dtype)
  if (out != logits) {  // the same rows in place, or rows that share nothing
    const uintptr_t a = (uintptr_t)logits, b = (uintptr_t)out;
    const uintptr_t span = (uintptr_t)(((size_t)(T - 1) * (size_t)row_stride + (size_t)V) * esz);
    if (a < b + span && b < a + span) return CC_ERR_BAD_ARG;
  }
  if (!cc_dt_ok(dtype)) return CC_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (out != logits) {
    if (dtype == CC_DT_F32) con_copy_launch<uint32_t>(logits, out, T, V, row_stride, st);
    else con_copy_launch<uint16_t>(logits, out, T, V, row_stride, st);
    CC_LAUNCH_CHECK();
  }
  switch (dtype) {
    case CC_DT_F32:
      con_streams_launch<uint32_t>(out, T, V, row_stride, cr, slices, tokens, pos, st);
      break;
    case CC_DT_BF16:
      con_streams_launch<con_bf16>(out, T, V, row_stride, cr, slices, tokens, pos, st);
      break;
    default:
      con_streams_launch<con_f16>(out, T, V, row_stride, cr, slices, tokens, pos, st);
      break;
  }
  CC_LAUNCH_CHECK();
  return CC_OK;
}
