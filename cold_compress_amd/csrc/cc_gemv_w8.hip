// cc_gemv_w8.hip — the int8 weight-only counterpart of cc_gemv.hip: the same five decode-layer forms (plain, RMSNorm(x + delta)
// prologue with h_out, SwiGLU pair, RoPE epilogue, bias) over W stored as int8 [N, K] with one scale per output row (the weight-only
// int8 checkpoint format; ref: quantize.py WeightOnlyInt8Linear, forward = F.linear(x, W.to(dtype)) * scales (+ bias)).
//
// Layout (cc_gemv.hip's, at half the bytes): one non-temporal 16-byte load per lane now carries 16 weights, so a wave still covers a
// 1 KiB segment of a row per load instruction (1024 weights); the four waves of a workgroup split a row's segments, RB rows and CU
// segments per wave are in flight together, and the FIRST tile's weights are requested before the input vector is touched.  Each
// lane keeps the 32 bytes of `in` (16 elements) it multiplies.  The int8 codes widen EXACTLY to the activation dtype and go through
// the same packed dot2 instructions as the 16-bit kernel (fp32 accumulation, fixed order):
//   f16 : bytes ^ 0x80 placed under a 0x64 exponent byte (v_perm) = 1024 + (q + 128) in f16, minus 1152 (v_pk_add_f16): exact
//   bf16: v_cvt_f32_i32 of the sign-extended byte (exact), the high halves of two such floats are the bf16 pair (v_perm)
// About 2.5 VALU operations per weight byte, against the ~12 per byte the CU can issue at the HBM rate.
//
// The RMSNorm prologue runs in the 16-bit kernel's layout (8 elements per lane and chunk, the same chunk order, the same fp32
// chains and the same LDS reduction): h_out and the normalised input are bit-identical to cc_gemv_fused's.  The normalised vector
// is passed to the lanes that multiply it through LDS (K * 2 bytes, norm forms only).
//
// TWO COPIES: gemv_w8_multi_kernel further down (the same product for up to four input vectors) repeats gemv_w8_kernel's prologue,
// row loop and epilogue, token by token, and promises the same bits; the weight tile, and with it the chunk ownership, is ONE function
// for both (gv_plain_tile, cc_gemv_core.h, shared with the dense kernels).  A change to a chain's order, a reduction or a rounding
// point here has to be made there too (tests/test_gpu_gemv_wo_multi.py compares the two bit for bit).  The copies stay because
// moving those steps into shared functions changes the single-vector kernels' machine code.  Launcher, switch table
// and argument checks exist once, for every token count (NT = 1: the single-vector kernel).
#include <cstdio>
#include <cstdlib>

#include "cc_common.h"
#include "cc_gemv_core.h"

namespace {

struct GemvW8Args {
  const int8_t* W;
  const int8_t* W3;     // second matrix of the SwiGLU pair, or null
  const void* scales;   // [N] model dtype
  const void* scales3;  // [N] model dtype (with W3)
  const void* x;        // [K]
  const void* delta;    // [K] pending residual, or null
  const void* norm_w;   // [K] RMSNorm weight, or null (no norm prologue)
  const void* bias;     // [N] or null
  const void* freqs;    // [head_dim/2, 2] (cos, sin) of this position, or null
  void* h_out;          // [K] x + delta, or null
  void* y;              // [N]
  float eps;
  int N, K, rope_rows, head_dim;
};

constexpr int kW8Threads = 256;
constexpr int kW8Waves = kW8Threads / 64;

template <typename T>
struct DotW8;  // acc += <16 int8 weights, 16 elements of x (two 16-byte halves)>
template <>
struct DotW8<bf16_t> {
  __device__ static __forceinline__ uint32_t pair(uint32_t w, int b) {  // bytes b, b + 1 of w -> packed bf16 (exact)
    const float lo = (float)(int)(int8_t)(w >> (8 * b));
    const float hi = (float)(int)(int8_t)(w >> (8 * b + 8));
    return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
  }
  __device__ static __forceinline__ float word(uint32_t w, uint32_t x0, uint32_t x1, float acc) {
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, pair(w, 0)), __builtin_bit_cast(bf16x2_t, x0), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, pair(w, 2)), __builtin_bit_cast(bf16x2_t, x1), acc, false);
    return acc;
  }
};
template <>
struct DotW8<f16_t> {
  __device__ static __forceinline__ float word(uint32_t w, uint32_t x0, uint32_t x1, float acc) {
    const uint32_t u = w ^ 0x80808080u;  // q + 128 in every byte
    const f16x2_t bias = __builtin_bit_cast(f16x2_t, 0x64806480u);  // 1152 = 1024 + 128
    const f16x2_t lo = __builtin_bit_cast(f16x2_t, __builtin_amdgcn_perm(0x64646464u, u, 0x04010400u)) - bias;
    const f16x2_t hi = __builtin_bit_cast(f16x2_t, __builtin_amdgcn_perm(0x64646464u, u, 0x04030402u)) - bias;
    acc = __builtin_amdgcn_fdot2(lo, __builtin_bit_cast(f16x2_t, x0), acc, false);
    acc = __builtin_amdgcn_fdot2(hi, __builtin_bit_cast(f16x2_t, x1), acc, false);
    return acc;
  }
};
template <typename T>
__device__ __forceinline__ float dot_w8(uint4 w, uint4 xa, uint4 xb, float acc) {  // weights 0..7 x xa, 8..15 x xb
  acc = DotW8<T>::word(w.x, xa.x, xa.y, acc);
  acc = DotW8<T>::word(w.y, xa.z, xa.w, acc);
  acc = DotW8<T>::word(w.z, xb.x, xb.y, acc);
  acc = DotW8<T>::word(w.w, xb.z, xb.w, acc);
  return acc;
}

template <typename T, bool SWIGLU, int RB, int CU, int XS>
__global__ __launch_bounds__(kW8Threads) void gemv_w8_kernel(GemvW8Args a) {
  constexpr int VEC = 8;   // 16-bit elements per 16-byte chunk of the input
  constexpr int WVEC = 16; // int8 weights per 16-byte load
  extern __shared__ uint4 sm_in[];  // the normalised input, norm forms only (K / 8 chunks)
  __shared__ float sm_red[kW8Waves];
  __shared__ float sm_part[kW8Waves][2][RB];
  const int K = a.K, N = a.N;
  const int nch = K / WVEC;                       // 16-byte weight chunks per row
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nseg = (nch + 63) / 64;
  const int nstep = (nseg + kW8Waves - 1) / kW8Waves;  // segments per wave (<= XS, checked by the launcher)
  const uint4* Wv = reinterpret_cast<const uint4*>(a.W);
  const uint4* W3v = reinterpret_cast<const uint4*>(a.W3);
  uint4 w[RB][CU], w3[RB][CU];
  auto issue = gv_plain_tile<SWIGLU>(w, w3, Wv, W3v, N, nch, nstep, lane, wave);
  const int row_first = blockIdx.x * RB;
  if (row_first < N) issue(row_first, 0);

  // ---- the input vector: lane keeps elements [16 c, 16 c + 16) of every chunk c = (j * 4 + wave) * 64 + lane it multiplies
  uint4 xa[XS], xb[XS];
  if (a.norm_w != nullptr) {
    // cc_gemv.hip's prologue, operation for operation: 8-element chunks c8 = (j * 4 + wave) * 64 + lane, the same sum-of-squares
    // chain per lane, the same wave and workgroup reductions
    constexpr int XP = 2 * XS;
    const int nch8 = K / VEC;
    const int nstep8 = ((nch8 + 63) / 64 + kW8Waves - 1) / kW8Waves;
    const T* xg = reinterpret_cast<const T*>(a.x);
    const T* dg = reinterpret_cast<const T*>(a.delta);
    const T* wg = reinterpret_cast<const T*>(a.norm_w);
    // (h goes through LDS rather than registers between the two passes: the long-K instantiations stay within the register file)
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < XP; j++) {
      const int c = (j * kW8Waves + wave) * 64 + lane;
      if (j < nstep8 && c < nch8) {
        Vec16<T> xv, dv;
        float h[VEC];
        xv.load(xg + (size_t)c * VEC);
        xv.unpack(h);
        if (dg != nullptr) {
          float d[VEC];
          dv.load(dg + (size_t)c * VEC);
          dv.unpack(d);
#pragma unroll
          for (int e = 0; e < VEC; e++) h[e] = ElemTraits<T>::rnd(__fadd_rn(h[e], d[e]));  // model-dtype residual add
        }
#pragma unroll
        for (int e = 0; e < VEC; e++) ss = fmaf(h[e], h[e], ss);
        const uint4 hp = pack16<T>(h);
        sm_in[c] = hp;
        if (a.h_out != nullptr && blockIdx.x == 0) reinterpret_cast<uint4*>(a.h_out)[c] = hp;
      }
    }
    ss = gv_wave_sum(ss);
    if (lane == 0) sm_red[wave] = ss;
    __syncthreads();
    const float tot = (sm_red[0] + sm_red[1]) + (sm_red[2] + sm_red[3]);
    const float rs = rsqrtf(tot / (float)K + a.eps);
#pragma unroll
    for (int j = 0; j < XP; j++) {
      const int c = (j * kW8Waves + wave) * 64 + lane;
      if (j < nstep8 && c < nch8) {  // (each lane rewrites only the chunks it wrote)
        Vec16<T> hv, nv;
        float h[VEC], wf[VEC], o[VEC];
        hv.raw = sm_in[c];
        nv.load(wg + (size_t)c * VEC);
        hv.unpack(h);
        nv.unpack(wf);
#pragma unroll
        for (int e = 0; e < VEC; e++) o[e] = ElemTraits<T>::rnd(__fmul_rn(ElemTraits<T>::rnd(cc_opaque_f32(__fmul_rn(h[e], rs))), wf[e]));
        sm_in[c] = pack16<T>(o);
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < XS; j++) {
      const int c = (j * kW8Waves + wave) * 64 + lane;
      const bool in = j < nstep && c < nch;
      xa[j] = in ? sm_in[2 * c] : make_uint4(0, 0, 0, 0);
      xb[j] = in ? sm_in[2 * c + 1] : make_uint4(0, 0, 0, 0);
    }
  } else {
    const uint4* xg = reinterpret_cast<const uint4*>(a.x);
#pragma unroll
    for (int j = 0; j < XS; j++) {
      const int c = (j * kW8Waves + wave) * 64 + lane;
      const bool in = j < nstep && c < nch;
      xa[j] = in ? xg[2 * c] : make_uint4(0, 0, 0, 0);
      xb[j] = in ? xg[2 * c + 1] : make_uint4(0, 0, 0, 0);
    }
  }

  T* yo = reinterpret_cast<T*>(a.y);
  const T* sc = reinterpret_cast<const T*>(a.scales);
  const T* sc3 = reinterpret_cast<const T*>(a.scales3);
  bool first = true;
  for (int r0 = row_first; r0 < N; r0 += gridDim.x * RB) {
    float acc[RB], acc3[RB];
#pragma unroll
    for (int r = 0; r < RB; r++) acc[r] = acc3[r] = 0.f;
#pragma unroll
    for (int s0 = 0; s0 < XS; s0 += CU) {
      if (s0 < nstep) {
        if (!first) issue(r0, s0);
        first = false;
#pragma unroll
        for (int u = 0; u < CU; u++) {
          const int j = s0 + u < XS ? s0 + u : XS - 1;  // beyond nstep the weights are zero-filled
#pragma unroll
          for (int r = 0; r < RB; r++) {
            acc[r] = dot_w8<T>(w[r][u], xa[j], xb[j], acc[r]);
            if (SWIGLU) acc3[r] = dot_w8<T>(w3[r][u], xa[j], xb[j], acc3[r]);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RB; r++) {
      const float s = gv_wave_sum(acc[r]);
      float s3 = 0.f;
      if (SWIGLU) s3 = gv_wave_sum(acc3[r]);
      if (lane == 0) {
        sm_part[wave][0][r] = s;
        if (SWIGLU) sm_part[wave][1][r] = s3;
      }
    }
    __syncthreads();
    if (wave == 0) {
      const int r = lane < RB ? lane : 0;
      const int row = r0 + r;
      const int rowc = row < N ? row : N - 1;
      // the reference's three rounding points: F.linear -> dtype, * scales -> dtype, + bias -> dtype
      float s = (sm_part[0][0][r] + sm_part[1][0][r]) + (sm_part[2][0][r] + sm_part[3][0][r]);
      s = ElemTraits<T>::rnd(cc_opaque_f32(s));
      s = ElemTraits<T>::rnd(cc_opaque_f32(__fmul_rn(s, ElemTraits<T>::load(sc, (size_t)rowc))));
      if (a.bias != nullptr) s = ElemTraits<T>::rnd(cc_opaque_f32(__fadd_rn(s, ElemTraits<T>::load(reinterpret_cast<const T*>(a.bias), (size_t)rowc))));
      if (SWIGLU) {
        float s3 = (sm_part[0][1][r] + sm_part[1][1][r]) + (sm_part[2][1][r] + sm_part[3][1][r]);
        s3 = ElemTraits<T>::rnd(cc_opaque_f32(s3));
        s3 = ElemTraits<T>::rnd(cc_opaque_f32(__fmul_rn(s3, ElemTraits<T>::load(sc3, (size_t)rowc))));
        const float sl = ElemTraits<T>::rnd(__fdiv_rn(s, 1.0f + expf(-s)));  // F.silu -> dtype
        s = __fmul_rn(sl, s3);
      }
      float out = s;
      if (a.freqs != nullptr) {  // RoPE on the (even, odd) row pairs of the q / k heads, on the rounded t
        const float other = gv_dpp<0xB1>(out);  // the pair partner lives in lane ^ 1 (r0 is even)
        if (row < a.rope_rows) {
          const int pr = (row % a.head_dim) >> 1;
          const float c = ElemTraits<T>::load(reinterpret_cast<const T*>(a.freqs), (size_t)pr * 2);
          const float sn = ElemTraits<T>::load(reinterpret_cast<const T*>(a.freqs), (size_t)pr * 2 + 1);
          out = (row & 1) ? __fadd_rn(__fmul_rn(out, c), __fmul_rn(other, sn)) : __fsub_rn(__fmul_rn(out, c), __fmul_rn(other, sn));
        }
      }
      if (lane < RB && row < N) ElemTraits<T>::store(yo, (size_t)row, cc_opaque_f32(out));
    }
    __syncthreads();  // sm_part is reused by the next row group
  }
}

struct W8Cfg {
  int rb, cu, cap;
};

static W8Cfg pick_w8_cfg(const GemvW8Args& a, int nstep) {
  static int env_rb = -1, env_cu = -1, env_cap = 2048;
  if (env_rb < 0) {  // tuning hook: CC_GEMV_W8_CFG="RB,CU[,max workgroups]"
    env_rb = env_cu = 0;
    if (const char* e = getenv("CC_GEMV_W8_CFG")) sscanf(e, "%d,%d,%d", &env_rb, &env_cu, &env_cap);
  }
  if (env_rb > 0 && env_cu > 0) return {env_rb, env_cu, env_cap};
  // the 16-bit kernel's choices at the same bytes in flight per lane (a 16-byte load holds twice the weights)
  if (nstep <= 1) {
    if (a.W3 != nullptr) return {4, 1, 2048};
    return a.N >= 32768 ? W8Cfg{4, 1, 1024} : W8Cfg{8, 1, 1024};
  }
  if (nstep <= 2) return a.W3 != nullptr ? W8Cfg{2, 2, 2048} : W8Cfg{4, 2, 1024};
  if (nstep <= 4) return a.W3 != nullptr ? W8Cfg{2, 4, 2048} : W8Cfg{4, 4, 512};
  return a.W3 != nullptr ? W8Cfg{2, 2, 2048} : W8Cfg{4, 2, 512};
}

// ---- the same product for NT input vectors from ONE pass over the int8 weights (cc_gemv_fused_w8_multi): cc_gemv.hip's
//      gemv_multi_kernel for this file's kernel.  Row t of y / h_out is BIT-IDENTICAL to gemv_w8_kernel on row t of x / delta / freqs:
//      the lane that owns a 16-byte weight chunk, the order of that lane's dot2 chain, gv_wave_sum, the four-wave meet
//      (p0 + p1) + (p2 + p3) and every rounding point of the prologue and the epilogue are gemv_w8_kernel's, kept per token.  A weight
//      register is loaded once and WIDENED once (DeqW8: the eight packed pairs DotW8<T>::word forms, exact either way) and then feeds
//      NT accumulator chains, so the conversion cost per token falls with NT.  None of that depends on RB, CU or the grid.
//      x, delta, h_out: [NT, K]; y: [NT, N]; freqs: [NT, head_dim / 2, 2].  A plain grid: no workgroup waits for another.
//
//      The RMSNorm prologue keeps ONE staging buffer (the single kernel's K * 2 bytes of dynamic LDS): every token's h = x + delta and
//      sum of squares are formed first, in the 16-bit kernel's chunk layout, with h parked in the registers that will hold the token's
//      input (2 * XS uint4, the same count); then the tokens pass through the buffer one after the other — normalise token t into it,
//      barrier, every lane picks up the 32-byte pieces it multiplies, barrier, the next token.
template <typename T>
struct DeqW8;  // one code word -> the two packed pairs DotW8<T>::word multiplies, and that multiply
template <>
struct DeqW8<bf16_t> {
  __device__ static __forceinline__ void word(uint32_t w, uint32_t& p0, uint32_t& p1) {
    p0 = DotW8<bf16_t>::pair(w, 0);
    p1 = DotW8<bf16_t>::pair(w, 2);
  }
  __device__ static __forceinline__ float dot(uint32_t p, uint32_t x, float acc) {
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, p), __builtin_bit_cast(bf16x2_t, x), acc, false);
  }
};
template <>
struct DeqW8<f16_t> {
  __device__ static __forceinline__ void word(uint32_t w, uint32_t& p0, uint32_t& p1) {
    const uint32_t u = w ^ 0x80808080u;  // q + 128 in every byte
    const f16x2_t bias = __builtin_bit_cast(f16x2_t, 0x64806480u);  // 1152 = 1024 + 128
    p0 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2_t, __builtin_amdgcn_perm(0x64646464u, u, 0x04010400u)) - bias);
    p1 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(f16x2_t, __builtin_amdgcn_perm(0x64646464u, u, 0x04030402u)) - bias);
  }
  __device__ static __forceinline__ float dot(uint32_t p, uint32_t x, float acc) {
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, p), __builtin_bit_cast(f16x2_t, x), acc, false);
  }
};
template <typename T>
__device__ __forceinline__ void deq_w8(uint4 w, uint32_t (&p)[8]) {
  DeqW8<T>::word(w.x, p[0], p[1]);
  DeqW8<T>::word(w.y, p[2], p[3]);
  DeqW8<T>::word(w.z, p[4], p[5]);
  DeqW8<T>::word(w.w, p[6], p[7]);
}
template <typename T>
__device__ __forceinline__ float dot_w8_deq(const uint32_t (&p)[8], uint4 xa, uint4 xb, float acc) {  // dot_w8's chain
  acc = DeqW8<T>::dot(p[0], xa.x, acc);
  acc = DeqW8<T>::dot(p[1], xa.y, acc);
  acc = DeqW8<T>::dot(p[2], xa.z, acc);
  acc = DeqW8<T>::dot(p[3], xa.w, acc);
  acc = DeqW8<T>::dot(p[4], xb.x, acc);
  acc = DeqW8<T>::dot(p[5], xb.y, acc);
  acc = DeqW8<T>::dot(p[6], xb.z, acc);
  acc = DeqW8<T>::dot(p[7], xb.w, acc);
  return acc;
}

template <typename T, bool SWIGLU, int RB, int CU, int XS, int NT>
__global__ __launch_bounds__(kW8Threads) void gemv_w8_multi_kernel(GemvW8Args a) {
  constexpr int VEC = 8;
  constexpr int WVEC = 16;
  static_assert(NT * RB <= 64 && RB % 2 == 0, "wave 0 finishes one (token, row) per lane; a RoPE pair stays in lanes l, l ^ 1");
  extern __shared__ uint4 sm_in[];  // ONE token's normalised input at a time, norm forms only (K / 8 chunks)
  __shared__ float sm_red[NT][kW8Waves];
  __shared__ float sm_part[NT][kW8Waves][2][RB];
  const int K = a.K, N = a.N;
  const int nch = K / WVEC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nseg = (nch + 63) / 64;
  const int nstep = (nseg + kW8Waves - 1) / kW8Waves;

  // ---- work decomposition and the weight tile: gemv_w8_kernel's (the first tile is requested before the inputs are touched)
  const uint4* Wv = reinterpret_cast<const uint4*>(a.W);
  const uint4* W3v = reinterpret_cast<const uint4*>(a.W3);
  uint4 w[RB][CU], w3[RB][CU];
  auto issue = gv_plain_tile<SWIGLU>(w, w3, Wv, W3v, N, nch, nstep, lane, wave);
  const int row_first = blockIdx.x * RB;
  if (row_first < N) issue(row_first, 0);

  // ---- the NT input vectors: xin[t][2 j], xin[t][2 j + 1] are gemv_w8_kernel's xa[j], xb[j] of token t
  uint4 xin[NT][2 * XS];
  if (a.norm_w != nullptr) {
    constexpr int XP = 2 * XS;
    const int nch8 = K / VEC;
    const int nstep8 = ((nch8 + 63) / 64 + kW8Waves - 1) / kW8Waves;
    const T* xg = reinterpret_cast<const T*>(a.x);
    const T* dg = reinterpret_cast<const T*>(a.delta);
    const T* wg = reinterpret_cast<const T*>(a.norm_w);
    float ss[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) ss[t] = 0.f;
#pragma unroll
    for (int j = 0; j < XP; j++) {
      const int c = (j * kW8Waves + wave) * 64 + lane;
      const bool in = j < nstep8 && c < nch8;
#pragma unroll
      for (int t = 0; t < NT; t++) {
        xin[t][j] = make_uint4(0, 0, 0, 0);
        if (in) {
          const size_t at = (size_t)t * K + (size_t)c * VEC;
          Vec16<T> xv, dv;
          float h[VEC];
          xv.load(xg + at);
          xv.unpack(h);
          if (dg != nullptr) {
            float d[VEC];
            dv.load(dg + at);
            dv.unpack(d);
#pragma unroll
            for (int e = 0; e < VEC; e++) h[e] = ElemTraits<T>::rnd(__fadd_rn(h[e], d[e]));  // model-dtype residual add
          }
#pragma unroll
          for (int e = 0; e < VEC; e++) ss[t] = fmaf(h[e], h[e], ss[t]);
          xin[t][j] = pack16<T>(h);  // (parked: the 8-element chunk c of token t's h)
          if (a.h_out != nullptr && blockIdx.x == 0) reinterpret_cast<uint4*>(a.h_out)[(size_t)t * nch8 + c] = xin[t][j];
        }
      }
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const float s = gv_wave_sum(ss[t]);
      if (lane == 0) sm_red[t][wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const float tot = (sm_red[t][0] + sm_red[t][1]) + (sm_red[t][2] + sm_red[t][3]);
      const float rs = rsqrtf(tot / (float)K + a.eps);
#pragma unroll
      for (int j = 0; j < XP; j++) {
        const int c = (j * kW8Waves + wave) * 64 + lane;
        if (j < nstep8 && c < nch8) {
          Vec16<T> hv, nv;
          float h[VEC], wf[VEC], o[VEC];
          hv.raw = xin[t][j];
          nv.load(wg + (size_t)c * VEC);
          hv.unpack(h);
          nv.unpack(wf);
#pragma unroll
          for (int e = 0; e < VEC; e++) o[e] = ElemTraits<T>::rnd(__fmul_rn(ElemTraits<T>::rnd(cc_opaque_f32(__fmul_rn(h[e], rs))), wf[e]));
          sm_in[c] = pack16<T>(o);
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < XS; j++) {
        const int c = (j * kW8Waves + wave) * 64 + lane;
        const bool in = j < nstep && c < nch;
        xin[t][2 * j] = in ? sm_in[2 * c] : make_uint4(0, 0, 0, 0);
        xin[t][2 * j + 1] = in ? sm_in[2 * c + 1] : make_uint4(0, 0, 0, 0);
      }
      if (t + 1 < NT) __syncthreads();  // the buffer is the next token's
    }
  } else {
    const uint4* xg = reinterpret_cast<const uint4*>(a.x);
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
      for (int j = 0; j < XS; j++) {
        const int c = (j * kW8Waves + wave) * 64 + lane;
        const bool in = j < nstep && c < nch;
        xin[t][2 * j] = in ? xg[((size_t)t * nch + c) * 2] : make_uint4(0, 0, 0, 0);
        xin[t][2 * j + 1] = in ? xg[((size_t)t * nch + c) * 2 + 1] : make_uint4(0, 0, 0, 0);
      }
    }
  }

  T* yo = reinterpret_cast<T*>(a.y);
  const T* sc = reinterpret_cast<const T*>(a.scales);
  const T* sc3 = reinterpret_cast<const T*>(a.scales3);
  bool first = true;
  for (int r0 = row_first; r0 < N; r0 += gridDim.x * RB) {
    float acc[NT][RB], acc3[NT][RB];
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
      for (int r = 0; r < RB; r++) acc[t][r] = acc3[t][r] = 0.f;
    }
#pragma unroll
    for (int s0 = 0; s0 < XS; s0 += CU) {
      if (s0 < nstep) {
        if (!first) issue(r0, s0);
        first = false;
#pragma unroll
        for (int u = 0; u < CU; u++) {
          const int j = s0 + u < XS ? s0 + u : XS - 1;  // beyond nstep the weights are zero-filled
#pragma unroll
          for (int r = 0; r < RB; r++) {
            uint32_t p[8];
            deq_w8<T>(w[r][u], p);  // widened once, multiplied NT times
#pragma unroll
            for (int t = 0; t < NT; t++) acc[t][r] = dot_w8_deq<T>(p, xin[t][2 * j], xin[t][2 * j + 1], acc[t][r]);
            if (SWIGLU) {
              deq_w8<T>(w3[r][u], p);
#pragma unroll
              for (int t = 0; t < NT; t++) acc3[t][r] = dot_w8_deq<T>(p, xin[t][2 * j], xin[t][2 * j + 1], acc3[t][r]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
      for (int r = 0; r < RB; r++) {
        const float s = gv_wave_sum(acc[t][r]);
        float s3 = 0.f;
        if (SWIGLU) s3 = gv_wave_sum(acc3[t][r]);
        if (lane == 0) {
          sm_part[t][wave][0][r] = s;
          if (SWIGLU) sm_part[t][wave][1][r] = s3;
        }
      }
    }
    __syncthreads();
    if (wave == 0) {  // lane t * RB + r finishes row r0 + r of token t
      const bool mine = lane < NT * RB;
      const int t = mine ? lane / RB : 0;
      const int r = mine ? lane % RB : 0;
      const int row = r0 + r;
      const int rowc = row < N ? row : N - 1;
      // gemv_w8_kernel's rounding points: F.linear -> dtype, * scales -> dtype, + bias -> dtype
      float s = (sm_part[t][0][0][r] + sm_part[t][1][0][r]) + (sm_part[t][2][0][r] + sm_part[t][3][0][r]);
      s = ElemTraits<T>::rnd(cc_opaque_f32(s));
      s = ElemTraits<T>::rnd(cc_opaque_f32(__fmul_rn(s, ElemTraits<T>::load(sc, (size_t)rowc))));
      if (a.bias != nullptr) s = ElemTraits<T>::rnd(cc_opaque_f32(__fadd_rn(s, ElemTraits<T>::load(reinterpret_cast<const T*>(a.bias), (size_t)rowc))));
      if (SWIGLU) {
        float s3 = (sm_part[t][0][1][r] + sm_part[t][1][1][r]) + (sm_part[t][2][1][r] + sm_part[t][3][1][r]);
        s3 = ElemTraits<T>::rnd(cc_opaque_f32(s3));
        s3 = ElemTraits<T>::rnd(cc_opaque_f32(__fmul_rn(s3, ElemTraits<T>::load(sc3, (size_t)rowc))));
        const float sl = ElemTraits<T>::rnd(__fdiv_rn(s, 1.0f + expf(-s)));  // F.silu -> dtype
        s = __fmul_rn(sl, s3);
      }
      float out = s;
      if (a.freqs != nullptr) {
        const float other = gv_dpp<0xB1>(out);  // the pair partner lives in lane ^ 1 (r0 and RB are even)
        if (row < a.rope_rows) {
          const T* fq = reinterpret_cast<const T*>(a.freqs) + (size_t)t * a.head_dim;  // token t's (cos, sin) rows
          const int pr = (row % a.head_dim) >> 1;
          const float c = ElemTraits<T>::load(fq, (size_t)pr * 2);
          const float sn = ElemTraits<T>::load(fq, (size_t)pr * 2 + 1);
          out = (row & 1) ? __fadd_rn(__fmul_rn(out, c), __fmul_rn(other, sn)) : __fsub_rn(__fmul_rn(out, c), __fmul_rn(other, sn));
        }
      }
      if (mine && row < N) ElemTraits<T>::store(yo, (size_t)t * N + row, cc_opaque_f32(out));
    }
    __syncthreads();  // sm_part is reused by the next row group
  }
}

// The geometry of a multi launch is pick_w8_cfg's choice for the shape too (results do not depend on it).  DESIGN.md §2.12 has the
// register figures of every instantiation: none of them needs fewer rows or column steps in flight.
template <typename T, bool SWIGLU, int RB, int CU, int XS, int NT>
static void launch_w8_cfg(const GemvW8Args& a, hipStream_t st, int cap) {
  int blocks = (a.N + RB - 1) / RB;
  if (blocks > cap) blocks = cap;
  const size_t lds = a.norm_w != nullptr ? (size_t)a.K * sizeof(T) : 0;  // one staging buffer, whatever NT
  if constexpr (NT == 1) {
    hipLaunchKernelGGL((gemv_w8_kernel<T, SWIGLU, RB, CU, XS>), dim3(blocks), dim3(kW8Threads), lds, st, a);
  } else {
    hipLaunchKernelGGL((gemv_w8_multi_kernel<T, SWIGLU, RB, CU, XS, NT>), dim3(blocks), dim3(kW8Threads), lds, st, a);
  }
}

template <typename T, int NT>
static int launch_gemv_w8(const GemvW8Args& a, hipStream_t st) {
  const int nseg = (a.K / 16 + 63) / 64, nstep = (nseg + kW8Waves - 1) / kW8Waves;
  const W8Cfg c = pick_w8_cfg(a, nstep);
  const int xs = nstep <= 1 ? 1 : nstep <= 2 ? 2 : nstep <= 4 ? 4 : 8;  // input chunk pairs kept per lane
  if (nstep > 8 || c.cu > xs || c.cap <= 0) return CC_ERR_UNSUPPORTED;
  const int key = (a.W3 ? 100000 : 0) + xs * 1000 + c.rb * 10 + c.cu;
  switch (key) {
    case 1041: launch_w8_cfg<T, false, 4, 1, 1, NT>(a, st, c.cap); break;
    case 1081: launch_w8_cfg<T, false, 8, 1, 1, NT>(a, st, c.cap); break;
    case 2042: launch_w8_cfg<T, false, 4, 2, 2, NT>(a, st, c.cap); break;
    case 4024: launch_w8_cfg<T, false, 2, 4, 4, NT>(a, st, c.cap); break;
    case 4042: launch_w8_cfg<T, false, 4, 2, 4, NT>(a, st, c.cap); break;
    case 4044: launch_w8_cfg<T, false, 4, 4, 4, NT>(a, st, c.cap); break;
    case 4082: launch_w8_cfg<T, false, 8, 2, 4, NT>(a, st, c.cap); break;
    case 8042: launch_w8_cfg<T, false, 4, 2, 8, NT>(a, st, c.cap); break;
    case 101021: launch_w8_cfg<T, true, 2, 1, 1, NT>(a, st, c.cap); break;
    case 101041: launch_w8_cfg<T, true, 4, 1, 1, NT>(a, st, c.cap); break;
    case 101081: launch_w8_cfg<T, true, 8, 1, 1, NT>(a, st, c.cap); break;
    case 102022: launch_w8_cfg<T, true, 2, 2, 2, NT>(a, st, c.cap); break;
    case 104024: launch_w8_cfg<T, true, 2, 4, 4, NT>(a, st, c.cap); break;
    case 108022: launch_w8_cfg<T, true, 2, 2, 8, NT>(a, st, c.cap); break;
    default: return CC_ERR_UNSUPPORTED;
  }
  CC_LAUNCH_CHECK();
  return CC_OK;
}

template <typename T>
static int launch_gemv_w8_t(const GemvW8Args& a, int nt, hipStream_t st) {
  switch (nt) {
    case 1: return launch_gemv_w8<T, 1>(a, st);  // one token: the single-vector kernel itself
    case 2: return launch_gemv_w8<T, 2>(a, st);
    case 3: return launch_gemv_w8<T, 3>(a, st);
    default: return launch_gemv_w8<T, 4>(a, st);
  }
}

}  // namespace

static int gemv_fused_w8_entry(const int8_t* W, const void* scales, const int8_t* W3, const void* scales3, const void* x, const void* delta,
                               const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs, int32_t rope_rows,
                               int32_t head_dim, void* y, int32_t N, int32_t K, int32_t T, int32_t dtype, cc_stream_t stream) {
  if (!scales || (W3 != nullptr) != (scales3 != nullptr)) return CC_ERR_BAD_ARG;
  if (const int rc = gv_check_args(W, W3, x, delta, norm_w, h_out, bias, freqs, rope_rows, head_dim, y, N, K, T, dtype)) return rc;
  if (dtype == CC_DT_F32) return CC_ERR_UNSUPPORTED;  // 16-bit activations only
  if (K % 16) return CC_ERR_UNSUPPORTED;
  GemvW8Args a{W, W3, scales, scales3, x, delta, norm_w, bias, freqs, h_out, y, eps, N, K, freqs ? rope_rows : 0, freqs ? head_dim : 2};
  hipStream_t st = (hipStream_t)stream;
  return dtype == CC_DT_BF16 ? launch_gemv_w8_t<bf16_t>(a, T, st) : launch_gemv_w8_t<f16_t>(a, T, st);
}

extern "C" int cc_gemv_fused_w8(const int8_t* W, const void* scales, const int8_t* W3, const void* scales3, const void* x,
                                const void* delta, const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs,
                                int32_t rope_rows, int32_t head_dim, void* y, int32_t N, int32_t K, int32_t dtype, cc_stream_t stream) {
  CC_ENTRY();
  return gemv_fused_w8_entry(W, scales, W3, scales3, x, delta, norm_w, eps, h_out, bias, freqs, rope_rows, head_dim, y, N, K, 1, dtype, stream);
}

extern "C" int cc_gemv_fused_w8_multi(const int8_t* W, const void* scales, const int8_t* W3, const void* scales3, const void* x,
                                      const void* delta, const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs,
                                      int32_t rope_rows, int32_t head_dim, void* y, int32_t N, int32_t K, int32_t T, int32_t dtype,
                                      cc_stream_t stream) {
  CC_ENTRY();
  return gemv_fused_w8_entry(W, scales, W3, scales3, x, delta, norm_w, eps, h_out, bias, freqs, rope_rows, head_dim, y, N, K, T, dtype, stream);
}
