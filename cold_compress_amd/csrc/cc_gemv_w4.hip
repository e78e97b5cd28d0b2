// cc_gemv_w4.hip — the int4 group-wise weight-only counterpart of cc_gemv.hip / cc_gemv_w8.hip: the same five decode-layer forms
// (plain, RMSNorm(x + delta) prologue with h_out, SwiGLU pair, RoPE epilogue, bias) over W stored as uint8 [N, K / 2] (two 4-bit
// codes per byte, column 2j in the low nibble) with one bf16 (scale, zero) pair per row and group of G columns, held per row as
// [N, K / G] 32-bit words (harness/quantize.py WeightOnlyInt4Linear; the reference's formula is W = (q - 8) * scale + zero).
//
// Layout: one non-temporal 16-byte load per lane carries 32 codes, so a wave covers a 1 KiB segment of a row (2048 weights) per load
// instruction.  A decode row is short at int4 (K = 4096: 2 KiB, two segments), so the four waves of a workgroup split into WS waves
// per row (WS = 1, 2 or 4, from the segment count) and 4 / WS row groups; RB rows and CU segments per wave are in flight together,
// and the FIRST tile's weights are requested before the input vector is touched.  A 32-column chunk never straddles a group
// (G >= 32), so each lane fetches one (scale, zero) word per chunk and row beside the codes.
//
// Arithmetic, group-factored (per chunk of 32 columns, one group):  sum_k x_k ((q_k - 8) s + z) = s (sum_k x_k (128 + q_k) - 136 Sx) + z Sx
// with Sx = sum_k x_k.  The codes become bf16 128 + q EXACTLY (v_perm puts each nibble byte under a 0x43 exponent byte) and go
// through the 16-bit kernel's packed v_dot2_f32_bf16, starting from -136 Sx; the lane pre-pairs its inputs to the perm's column
// order (even columns of a word, then odd) once, and Sx depends on x alone, so it is computed once per lane.  Per chunk and row:
// 3 ops per code word + 4 perms + 4 dot2 per 8 codes, then 2 fma and 2 bit ops: about 3 VALU operations per weight byte.  The
// cancellation costs about 7 of fp32's 24 bits, far below a bf16 ulp.
//
// The RMSNorm prologue runs in the 16-bit kernel's layout (8 elements per lane and chunk, the same chunk order, the same fp32
// chains and the same LDS reduction): h_out and the normalised input are bit-identical to cc_gemv_fused's.  The normalised vector
// is passed to the lanes that multiply it through LDS (K * 2 bytes, norm forms only).
//
// TWO COPIES: gemv_w4_multi_kernel further down (the same product for up to four input vectors) repeats gemv_w4_kernel's prologue,
// row loop and epilogue, token by token, and promises the same bits; the code / (scale, zero) tile, and with it the chunk ownership,
// is ONE function for both (gv_scaled_tile, cc_gemv_core.h, shared with the MXFP4 kernel).  A change to a chain's order, a reduction
// or a rounding point here has to be made there too (tests/test_gpu_gemv_w4_multi.py compares the two bit for bit).  The copies stay
// because moving those steps into shared functions changes the single-vector kernels' machine code.  Launcher,
// W4_CASE table and argument checks exist once, for every token count (NT = 1: the single-vector kernel).
#include <cstdio>
#include <cstdlib>

#include "cc_common.h"
#include "cc_gemv_core.h"

namespace {

struct GemvW4Args {
  const uint8_t* W;
  const uint8_t* W3;      // second matrix of the SwiGLU pair, or null
  const uint32_t* qp;     // [N, K / G] (scale, zero) bf16 pairs, the scale in the low half
  const uint32_t* qp3;    // the same for W3
  const void* x;          // [K] bf16
  const void* delta;      // [K] pending residual, or null
  const void* norm_w;     // [K] RMSNorm weight, or null (no norm prologue)
  const void* bias;       // [N] or null
  const void* freqs;      // [head_dim/2, 2] (cos, sin) of this position, or null
  void* h_out;            // [K] x + delta, or null
  void* y;                // [N]
  float eps;
  int N, K, gshift, rope_rows, head_dim;  // gshift = log2(G / 32): the group of 32-column chunk c is c >> gshift
};

constexpr int kW4Threads = 256;
constexpr int kW4Waves = kW4Threads / 64;

__device__ __forceinline__ float dot2_bf16(uint32_t a, uint32_t b, float acc) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a), __builtin_bit_cast(bf16x2_t, b), acc, false);
}

// acc += sum over the 8 codes of w (columns 8i .. 8i + 7 of a chunk) of (128 + q) * x; xr holds that word's inputs as the bf16
// pairs (x0, x2), (x4, x6), (x1, x3), (x5, x7)
__device__ __forceinline__ float dot_w4_word(uint32_t w, uint4 xr, float acc) {
  const uint32_t lo = w & 0x0F0F0F0Fu;         // codes of columns 0, 2, 4, 6
  const uint32_t hi = (w >> 4) & 0x0F0F0F0Fu;  // codes of columns 1, 3, 5, 7
  constexpr uint32_t kExp = 0x43434343u;       // byte q under 0x43: the bf16 128 + q
  acc = dot2_bf16(__builtin_amdgcn_perm(kExp, lo, 0x04010400u), xr.x, acc);
  acc = dot2_bf16(__builtin_amdgcn_perm(kExp, lo, 0x04030402u), xr.y, acc);
  acc = dot2_bf16(__builtin_amdgcn_perm(kExp, hi, 0x04010400u), xr.z, acc);
  acc = dot2_bf16(__builtin_amdgcn_perm(kExp, hi, 0x04030402u), xr.w, acc);
  return acc;
}

// one chunk (32 codes) of a row: sum x (q - 8) (from -136 Sx), then the group's scale and zero
__device__ __forceinline__ float chunk_w4(uint4 w, uint32_t q, const uint4 (&xr)[4], float sx, float m136, float acc) {
  float d = dot_w4_word(w.x, xr[0], m136);
  d = dot_w4_word(w.y, xr[1], d);
  d = dot_w4_word(w.z, xr[2], d);
  d = dot_w4_word(w.w, xr[3], d);
  acc = fmaf(__uint_as_float(q << 16), d, acc);              // scale
  return fmaf(__uint_as_float(q & 0xffff0000u), sx, acc);    // zero
}

template <bool SWIGLU, int RB, int CU, int XS, int WS>
__global__ __launch_bounds__(kW4Threads) void gemv_w4_kernel(GemvW4Args a) {
  typedef bf16_t T;
  constexpr int VEC = 8;             // bf16 elements per 16-byte chunk of the input
  constexpr int RG = kW4Waves / WS;  // row groups of a workgroup
  constexpr int RW = RB * RG;        // rows per workgroup round (even: RoPE's pair partner is lane ^ 1)
  static_assert(RW <= 64 && RW % 2 == 0, "rows per round");
  extern __shared__ uint4 sm_in[];   // the normalised input, norm forms only (K / 8 chunks)
  __shared__ float sm_red[kW4Waves];
  __shared__ float sm_part[kW4Waves][2][RB];
  const int K = a.K, N = a.N;
  const int nch = K / 32;            // 16-byte code chunks per row
  const int ngr = nch >> a.gshift;   // groups per row
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ws = wave % WS, rg = wave / WS;
  const int nseg = (nch + 63) / 64;
  const int nstep = (nseg + WS - 1) / WS;  // segments per wave (<= XS, checked by the launcher)
  const uint4* Wv = reinterpret_cast<const uint4*>(a.W);
  const uint4* W3v = reinterpret_cast<const uint4*>(a.W3);
  uint4 w[RB][CU], w3[RB][CU];
  uint32_t q[RB][CU], q3[RB][CU];
  auto issue = gv_scaled_tile<SWIGLU, WS, true, 0u>(w, w3, q, q3, Wv, W3v, a.qp, a.qp3, N, nch, nstep, lane, ws, ngr, a.gshift);
  const int row_first = blockIdx.x * RW;  // < N (the launcher sizes the grid)
  issue(row_first + rg * RB, 0);

  // ---- the input vector: the lane keeps elements [32 c, 32 c + 32) of every chunk c = (j * WS + ws) * 64 + lane it multiplies
  uint4 xv[XS][4];
  if (a.norm_w != nullptr) {
    // cc_gemv.hip's prologue, operation for operation: 8-element chunks c8 = (j * 4 + wave) * 64 + lane, the same sum-of-squares
    // chain per lane, the same wave and workgroup reductions
    const int nch8 = K / VEC;
    const int nstep8 = ((nch8 + 63) / 64 + kW4Waves - 1) / kW4Waves;
    const T* xg = reinterpret_cast<const T*>(a.x);
    const T* dg = reinterpret_cast<const T*>(a.delta);
    const T* wg = reinterpret_cast<const T*>(a.norm_w);
    float ss = 0.f;
    for (int j = 0; j < nstep8; j++) {
      const int c = (j * kW4Waves + wave) * 64 + lane;
      if (c < nch8) {
        Vec16<T> xl, dv;
        float h[VEC];
        xl.load(xg + (size_t)c * VEC);
        xl.unpack(h);
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
    for (int j = 0; j < nstep8; j++) {
      const int c = (j * kW4Waves + wave) * 64 + lane;
      if (c < nch8) {  // (each lane rewrites only the chunks it wrote)
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
      const int c = (j * WS + ws) * 64 + lane;
      const bool in = j < nstep && c < nch;
#pragma unroll
      for (int i = 0; i < 4; i++) xv[j][i] = in ? sm_in[4 * c + i] : make_uint4(0, 0, 0, 0);
    }
  } else {
    const uint4* xg = reinterpret_cast<const uint4*>(a.x);
#pragma unroll
    for (int j = 0; j < XS; j++) {
      const int c = (j * WS + ws) * 64 + lane;
      const bool in = j < nstep && c < nch;
#pragma unroll
      for (int i = 0; i < 4; i++) xv[j][i] = in ? xg[4 * c + i] : make_uint4(0, 0, 0, 0);
    }
  }
  // pair the inputs to the perm's column order and take the per-chunk sums (once per lane)
  uint4 xr[XS][4];
  float sx[XS], m136[XS];
#pragma unroll
  for (int j = 0; j < XS; j++) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const uint4 v = xv[j][i];
      xr[j][i] = make_uint4(__builtin_amdgcn_perm(v.y, v.x, 0x05040100u), __builtin_amdgcn_perm(v.w, v.z, 0x05040100u),
                            __builtin_amdgcn_perm(v.y, v.x, 0x07060302u), __builtin_amdgcn_perm(v.w, v.z, 0x07060302u));
      s = dot2_bf16(v.x, 0x3F803F80u, s);  // (1, 1)
      s = dot2_bf16(v.y, 0x3F803F80u, s);
      s = dot2_bf16(v.z, 0x3F803F80u, s);
      s = dot2_bf16(v.w, 0x3F803F80u, s);
    }
    sx[j] = s;
    m136[j] = -136.f * s;
  }

  T* yo = reinterpret_cast<T*>(a.y);
  bool first = true;
  for (int r0 = row_first; r0 < N; r0 += gridDim.x * RW) {
    const int rw0 = r0 + rg * RB;
    float acc[RB], acc3[RB];
#pragma unroll
    for (int r = 0; r < RB; r++) acc[r] = acc3[r] = 0.f;
#pragma unroll
    for (int s0 = 0; s0 < XS; s0 += CU) {
      if (s0 < nstep) {
        if (!first) issue(rw0, s0);
        first = false;
#pragma unroll
        for (int u = 0; u < CU; u++) {
          const int j = s0 + u < XS ? s0 + u : XS - 1;  // beyond nstep the codes and (scale, zero) are zero-filled
#pragma unroll
          for (int r = 0; r < RB; r++) {
            acc[r] = chunk_w4(w[r][u], q[r][u], xr[j], sx[j], m136[j], acc[r]);
            if (SWIGLU) acc3[r] = chunk_w4(w3[r][u], q3[r][u], xr[j], sx[j], m136[j], acc3[r]);
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
      const int l = lane < RW ? lane : 0;
      const int g = l / RB, r = l % RB;
      const int row = r0 + l;
      const int rowc = row < N ? row : N - 1;
      auto part = [&](int m) {  // the WS waves of row group g, in a fixed order
        if (WS == 1) return sm_part[g][m][r];
        if (WS == 2) return sm_part[2 * g][m][r] + sm_part[2 * g + 1][m][r];
        return (sm_part[0][m][r] + sm_part[1][m][r]) + (sm_part[2][m][r] + sm_part[3][m][r]);
      };
      // t = bf16(p); with bias t = bf16(t + bias)
      float s = ElemTraits<T>::rnd(cc_opaque_f32(part(0)));
      if (a.bias != nullptr) s = ElemTraits<T>::rnd(cc_opaque_f32(__fadd_rn(s, ElemTraits<T>::load(reinterpret_cast<const T*>(a.bias), (size_t)rowc))));
      if (SWIGLU) {
        const float s3 = ElemTraits<T>::rnd(cc_opaque_f32(part(1)));
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
      if (lane < RW && row < N) ElemTraits<T>::store(yo, (size_t)row, cc_opaque_f32(out));
    }
    __syncthreads();  // sm_part is reused by the next row group
  }
}

struct W4Cfg {
  int rb, cu, cap;
};

// rows x segments in flight per wave, by segments per wave (nstep) and form; tools/bench_gemv_w4.py measured them
static W4Cfg pick_w4_cfg(const GemvW4Args& a, int nstep) {
  static int env_rb = -1, env_cu = -1, env_cap = 2048;
  if (env_rb < 0) {  // tuning hook: CC_GEMV_W4_CFG="RB,CU[,max workgroups]"
    env_rb = env_cu = 0;
    if (const char* e = getenv("CC_GEMV_W4_CFG")) sscanf(e, "%d,%d,%d", &env_rb, &env_cu, &env_cap);
  }
  if (env_rb > 0 && env_cu > 0) return {env_rb, env_cu, env_cap};
  // same-box sweep (profiles/w4_gemv_sweep.jsonl, G = 32): the pair 4 x 1 at 2048 / 1024 / 512 workgroups 22.7 / 20.0 / 19.2 us
  // (2 x 1: 21.7, 8 x 1: 21.0-23.6); w2 4 x 2 x 512 10.9 us (8 x 2: 11.7-12.4, 8 x 1: 11.3); one-segment plain rows 4 x 1 x 1024
  // (LM head 60.6 us against 62.4-65.5, wqkv 8.4, wo 5.0).  Fewer, longer-lived workgroups amortise the per-workgroup prologue.
  // Rows of more than two segments per wave (K > 16384 at WS = 4, e.g. the 70B w2) take w2's choice; the sweep did not cover them.
  if (nstep <= 1) return a.W3 != nullptr ? W4Cfg{4, 1, 512} : W4Cfg{4, 1, 1024};
  return a.W3 != nullptr ? W4Cfg{2, 2, 512} : W4Cfg{4, 2, 512};
}

// ---- the same product for NT input vectors from ONE pass over the int4 weights (cc_gemv_fused_w4_multi): cc_gemv_mx4.hip's
//      gemv_mx4_multi_kernel for this file's kernel.  Row t of y / h_out is BIT-IDENTICAL to gemv_w4_kernel on row t of x / delta /
//      freqs: the lane that owns a 16-byte code chunk, dot_w4_word's order of the four dot2 per word and the words' order within a
//      chunk, the chain start -136 Sx, the two fmaf per chunk (scale, then zero times Sx), the order of a lane's chunks, gv_wave_sum,
//      the meet of a row's WS waves (WS is launch_gemv_w4's function of K) and every rounding point of the prologue and the epilogue
//      are gemv_w4_kernel's, kept per token.  A code register and its (scale, zero) word are loaded once and DECODED once (the two
//      nibble masks and four v_perm of a word, exact) and then feed NT accumulator chains, so the decode cost per token falls with
//      NT; the sixteen dot2 and two fma per chunk and token do not.  None of that depends on RB, CU or the grid.  x, delta, h_out:
//      [NT, K]; y: [NT, N]; freqs: [NT, head_dim / 2, 2].  A plain grid: no workgroup waits for another.
//
//      The RMSNorm prologue keeps ONE staging buffer (the single kernel's K * 2 bytes of dynamic LDS): every token's h = x + delta and
//      sum of squares are formed first, in the 16-bit kernel's chunk layout, with h parked in the registers that will hold the token's
//      re-paired input (4 * XS uint4: a lane never owns more 8-element chunks than that); then the tokens pass through the buffer one
//      after the other — normalise token t into it, barrier, every lane picks up the 64-byte pieces it multiplies, barrier, the next
//      token.  Re-pairing and Sx follow the pick-up, as in gemv_w4_kernel.
__device__ __forceinline__ void deq_w4_word(uint32_t w, uint32_t* p) {  // dot_w4_word's four operands, in its order
  const uint32_t lo = w & 0x0F0F0F0Fu;
  const uint32_t hi = (w >> 4) & 0x0F0F0F0Fu;
  constexpr uint32_t kExp = 0x43434343u;
  p[0] = __builtin_amdgcn_perm(kExp, lo, 0x04010400u);
  p[1] = __builtin_amdgcn_perm(kExp, lo, 0x04030402u);
  p[2] = __builtin_amdgcn_perm(kExp, hi, 0x04010400u);
  p[3] = __builtin_amdgcn_perm(kExp, hi, 0x04030402u);
}
// one chunk's 32 codes as the 16 bf16 pairs 128 + q, in chunk_w4's order (decoded once for the NT tokens)
__device__ __forceinline__ void deq_w4(uint4 w, uint32_t (&p)[16]) {
  deq_w4_word(w.x, p);
  deq_w4_word(w.y, p + 4);
  deq_w4_word(w.z, p + 8);
  deq_w4_word(w.w, p + 12);
}
// chunk_w4 over decoded pairs: the chain from -136 Sx, then the group's scale and zero
__device__ __forceinline__ float chunk_w4_deq(const uint32_t (&p)[16], uint32_t q, const uint4* xr, float sx, float m136, float acc) {
  float d = m136;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    d = dot2_bf16(p[4 * i], xr[i].x, d);
    d = dot2_bf16(p[4 * i + 1], xr[i].y, d);
    d = dot2_bf16(p[4 * i + 2], xr[i].z, d);
    d = dot2_bf16(p[4 * i + 3], xr[i].w, d);
  }
  acc = fmaf(__uint_as_float(q << 16), d, acc);              // scale
  return fmaf(__uint_as_float(q & 0xffff0000u), sx, acc);    // zero
}

template <bool SWIGLU, int RB, int CU, int XS, int WS, int NT>
__global__ __launch_bounds__(kW4Threads) void gemv_w4_multi_kernel(GemvW4Args a) {
  typedef bf16_t T;
  constexpr int VEC = 8;
  constexpr int RG = kW4Waves / WS;
  constexpr int RW = RB * RG;
  static_assert(NT * RW <= 64 && RW % 2 == 0, "wave 0 finishes one (token, row) per lane; a RoPE pair stays in lanes l, l ^ 1");
  extern __shared__ uint4 sm_in[];  // ONE token's normalised input at a time, norm forms only (K / 8 chunks)
  __shared__ float sm_red[NT][kW4Waves];
  __shared__ float sm_part[NT][kW4Waves][2][RB];
  const int K = a.K, N = a.N;
  const int nch = K / 32;
  const int ngr = nch >> a.gshift;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ws = wave % WS, rg = wave / WS;
  const int nseg = (nch + 63) / 64;
  const int nstep = (nseg + WS - 1) / WS;

  // ---- work decomposition and the code / (scale, zero) tile: gemv_w4_kernel's (requested before the inputs are touched)
  const uint4* Wv = reinterpret_cast<const uint4*>(a.W);
  const uint4* W3v = reinterpret_cast<const uint4*>(a.W3);
  uint4 w[RB][CU], w3[RB][CU];
  uint32_t q[RB][CU], q3[RB][CU];
  auto issue = gv_scaled_tile<SWIGLU, WS, true, 0u>(w, w3, q, q3, Wv, W3v, a.qp, a.qp3, N, nch, nstep, lane, ws, ngr, a.gshift);
  const int row_first = blockIdx.x * RW;  // < N (the launcher sizes the grid)
  issue(row_first + rg * RB, 0);

  // ---- the NT input vectors: xr[t][4 j + i] ends as gemv_w4_kernel's xr[j][i] of token t (before that its xv[j][i], and in the
  //      norm prologue the parked h)
  uint4 xr[NT][4 * XS];
  if (a.norm_w != nullptr) {
    constexpr int XP = 4 * XS;
    const int nch8 = K / VEC;
    const int nstep8 = ((nch8 + 63) / 64 + kW4Waves - 1) / kW4Waves;  // <= nseg <= WS * nstep <= XP
    const T* xg = reinterpret_cast<const T*>(a.x);
    const T* dg = reinterpret_cast<const T*>(a.delta);
    const T* wg = reinterpret_cast<const T*>(a.norm_w);
    float ss[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) ss[t] = 0.f;
#pragma unroll
    for (int j = 0; j < XP; j++) {
      const int c = (j * kW4Waves + wave) * 64 + lane;
      const bool in = j < nstep8 && c < nch8;
#pragma unroll
      for (int t = 0; t < NT; t++) {
        xr[t][j] = make_uint4(0, 0, 0, 0);
        if (in) {
          const size_t at = (size_t)t * K + (size_t)c * VEC;
          Vec16<T> xl, dv;
          float h[VEC];
          xl.load(xg + at);
          xl.unpack(h);
          if (dg != nullptr) {
            float d[VEC];
            dv.load(dg + at);
            dv.unpack(d);
#pragma unroll
            for (int e = 0; e < VEC; e++) h[e] = ElemTraits<T>::rnd(__fadd_rn(h[e], d[e]));  // model-dtype residual add
          }
#pragma unroll
          for (int e = 0; e < VEC; e++) ss[t] = fmaf(h[e], h[e], ss[t]);
          xr[t][j] = pack16<T>(h);  // (parked: the 8-element chunk c of token t's h)
          if (a.h_out != nullptr && blockIdx.x == 0) reinterpret_cast<uint4*>(a.h_out)[(size_t)t * nch8 + c] = xr[t][j];
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
        const int c = (j * kW4Waves + wave) * 64 + lane;
        if (j < nstep8 && c < nch8) {
          Vec16<T> hv, nv;
          float h[VEC], wf[VEC], o[VEC];
          hv.raw = xr[t][j];
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
        const int c = (j * WS + ws) * 64 + lane;
        const bool in = j < nstep && c < nch;
#pragma unroll
        for (int i = 0; i < 4; i++) xr[t][4 * j + i] = in ? sm_in[4 * c + i] : make_uint4(0, 0, 0, 0);
      }
      if (t + 1 < NT) __syncthreads();  // the buffer is the next token's
    }
  } else {
    const uint4* xg = reinterpret_cast<const uint4*>(a.x);
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
      for (int j = 0; j < XS; j++) {
        const int c = (j * WS + ws) * 64 + lane;
        const bool in = j < nstep && c < nch;
#pragma unroll
        for (int i = 0; i < 4; i++) xr[t][4 * j + i] = in ? xg[((size_t)t * nch + c) * 4 + i] : make_uint4(0, 0, 0, 0);
      }
    }
  }
  // pair every token's inputs to the perm's column order, in place, and take the per-chunk sums (gemv_w4_kernel's chain)
  float sx[NT][XS], m136[NT][XS];
#pragma unroll
  for (int t = 0; t < NT; t++) {
#pragma unroll
    for (int j = 0; j < XS; j++) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const uint4 v = xr[t][4 * j + i];
        xr[t][4 * j + i] = make_uint4(__builtin_amdgcn_perm(v.y, v.x, 0x05040100u), __builtin_amdgcn_perm(v.w, v.z, 0x05040100u),
                                      __builtin_amdgcn_perm(v.y, v.x, 0x07060302u), __builtin_amdgcn_perm(v.w, v.z, 0x07060302u));
        s = dot2_bf16(v.x, 0x3F803F80u, s);  // (1, 1)
        s = dot2_bf16(v.y, 0x3F803F80u, s);
        s = dot2_bf16(v.z, 0x3F803F80u, s);
        s = dot2_bf16(v.w, 0x3F803F80u, s);
      }
      sx[t][j] = s;
      m136[t][j] = -136.f * s;
    }
  }

  T* yo = reinterpret_cast<T*>(a.y);
  bool first = true;
  for (int r0 = row_first; r0 < N; r0 += gridDim.x * RW) {
    const int rw0 = r0 + rg * RB;
    float acc[NT][RB], acc3[NT][RB];
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
      for (int r = 0; r < RB; r++) acc[t][r] = acc3[t][r] = 0.f;
    }
#pragma unroll
    for (int s0 = 0; s0 < XS; s0 += CU) {
      if (s0 < nstep) {
        if (!first) issue(rw0, s0);
        first = false;
#pragma unroll
        for (int u = 0; u < CU; u++) {
          const int j = s0 + u < XS ? s0 + u : XS - 1;  // beyond nstep the codes and (scale, zero) are zero-filled
#pragma unroll
          for (int r = 0; r < RB; r++) {
            uint32_t p[16];
            deq_w4(w[r][u], p);  // decoded once, multiplied NT times
#pragma unroll
            for (int t = 0; t < NT; t++) acc[t][r] = chunk_w4_deq(p, q[r][u], &xr[t][4 * j], sx[t][j], m136[t][j], acc[t][r]);
            if (SWIGLU) {
              deq_w4(w3[r][u], p);
#pragma unroll
              for (int t = 0; t < NT; t++) acc3[t][r] = chunk_w4_deq(p, q3[r][u], &xr[t][4 * j], sx[t][j], m136[t][j], acc3[t][r]);
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
    if (wave == 0) {  // lane t * RW + l finishes row r0 + l of token t
      const bool mine = lane < NT * RW;
      const int t = mine ? lane / RW : 0;
      const int l = mine ? lane % RW : 0;
      const int g = l / RB, r = l % RB;
      const int row = r0 + l;
      const int rowc = row < N ? row : N - 1;
      auto part = [&](int m) {  // the WS waves of row group g, in gemv_w4_kernel's order
        if (WS == 1) return sm_part[t][g][m][r];
        if (WS == 2) return sm_part[t][2 * g][m][r] + sm_part[t][2 * g + 1][m][r];
        return (sm_part[t][0][m][r] + sm_part[t][1][m][r]) + (sm_part[t][2][m][r] + sm_part[t][3][m][r]);
      };
      float s = ElemTraits<T>::rnd(cc_opaque_f32(part(0)));
      if (a.bias != nullptr) s = ElemTraits<T>::rnd(cc_opaque_f32(__fadd_rn(s, ElemTraits<T>::load(reinterpret_cast<const T*>(a.bias), (size_t)rowc))));
      if (SWIGLU) {
        const float s3 = ElemTraits<T>::rnd(cc_opaque_f32(part(1)));
        const float sl = ElemTraits<T>::rnd(__fdiv_rn(s, 1.0f + expf(-s)));  // F.silu -> dtype
        s = __fmul_rn(sl, s3);
      }
      float out = s;
      if (a.freqs != nullptr) {
        const float other = gv_dpp<0xB1>(out);  // the pair partner lives in lane ^ 1 (r0 and RW are even)
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

// NT = 1: the single-vector kernel at the geometry asked for.  NT > 1: only the DEFAULT geometry of a shape class (pick_w4_cfg
// without the tuning hook: 4 x 1 for one segment per wave, else 2 x 2 for the pair and 4 x 2) is built, ten instantiations per NT
// (DESIGN.md §2.27 has their register figures; 8 rows per wave at WS = 1 would need more than wave 0's 64 finishing lanes), and every
// geometry of the class runs it: the same bits — results do not depend on RB or CU — with the hook's cap on the grid.  WS stays
// launch_gemv_w4's function of K, which the order of a row's sum does depend on.
template <bool SWIGLU, int RB, int CU, int XS, int WS, int NT>
static void launch_w4_geo(const GemvW4Args& a, hipStream_t st, int cap) {
  constexpr int RW = RB * (kW4Waves / WS);
  int blocks = (a.N + RW - 1) / RW;
  if (blocks > cap) blocks = cap;
  const size_t lds = a.norm_w != nullptr ? (size_t)a.K * sizeof(bf16_t) : 0;  // one staging buffer, whatever NT
  if constexpr (NT == 1) {
    hipLaunchKernelGGL((gemv_w4_kernel<SWIGLU, RB, CU, XS, WS>), dim3(blocks), dim3(kW4Threads), lds, st, a);
  } else {
    hipLaunchKernelGGL((gemv_w4_multi_kernel<SWIGLU, RB, CU, XS, WS, NT>), dim3(blocks), dim3(kW4Threads), lds, st, a);
  }
}
template <bool SWIGLU, int RB, int CU, int XS, int WS, int NT>
static void launch_w4_cfg(const GemvW4Args& a, hipStream_t st, int cap) {
  if constexpr (NT == 1) {
    launch_w4_geo<SWIGLU, RB, CU, XS, WS, 1>(a, st, cap);
  } else {
    launch_w4_geo<SWIGLU, XS == 1 ? 4 : SWIGLU ? 2 : 4, XS == 1 ? 1 : 2, XS, WS, NT>(a, st, cap);
  }
}

// (the same CC_ERR_UNSUPPORTED cases for every NT: a CC_GEMV_W4_CFG must name a geometry of this table)
template <int NT>
static int launch_gemv_w4(const GemvW4Args& a, hipStream_t st) {
  const int nseg = (a.K / 32 + 63) / 64;
  const int ws = nseg >= 3 ? 4 : nseg;  // waves per row: a short row leaves no wave idle
  const int nstep = (nseg + ws - 1) / ws;
  const W4Cfg c = pick_w4_cfg(a, nstep);
  const int xs = nstep <= 1 ? 1 : nstep <= 2 ? 2 : 4;  // input chunks kept per lane
  if (nstep > 4 || c.cu > xs || c.cap <= 0) return CC_ERR_UNSUPPORTED;
  const int key = (a.W3 ? 100000 : 0) + ws * 10000 + xs * 1000 + c.rb * 10 + c.cu;
#define W4_CASE(SW, WS_, XS_, RB_, CU_) \
  case (SW ? 100000 : 0) + WS_ * 10000 + XS_ * 1000 + RB_ * 10 + CU_: launch_w4_cfg<SW, RB_, CU_, XS_, WS_, NT>(a, st, c.cap); break;
  switch (key) {
    W4_CASE(false, 1, 1, 2, 1) W4_CASE(false, 1, 1, 4, 1) W4_CASE(false, 1, 1, 8, 1)
    W4_CASE(false, 2, 1, 2, 1) W4_CASE(false, 2, 1, 4, 1) W4_CASE(false, 2, 1, 8, 1)
    W4_CASE(false, 4, 1, 2, 1) W4_CASE(false, 4, 1, 4, 1) W4_CASE(false, 4, 1, 8, 1)
    W4_CASE(false, 4, 2, 4, 1) W4_CASE(false, 4, 2, 8, 1) W4_CASE(false, 4, 2, 2, 2) W4_CASE(false, 4, 2, 4, 2) W4_CASE(false, 4, 2, 8, 2)
    W4_CASE(false, 4, 4, 2, 4) W4_CASE(false, 4, 4, 4, 2) W4_CASE(false, 4, 4, 8, 2) W4_CASE(false, 4, 4, 4, 4)
    W4_CASE(true, 1, 1, 2, 1) W4_CASE(true, 1, 1, 4, 1) W4_CASE(true, 1, 1, 8, 1)
    W4_CASE(true, 2, 1, 2, 1) W4_CASE(true, 2, 1, 4, 1) W4_CASE(true, 2, 1, 8, 1)
    W4_CASE(true, 4, 1, 2, 1) W4_CASE(true, 4, 1, 4, 1) W4_CASE(true, 4, 1, 8, 1)
    W4_CASE(true, 4, 2, 2, 1) W4_CASE(true, 4, 2, 4, 1) W4_CASE(true, 4, 2, 2, 2) W4_CASE(true, 4, 2, 4, 2)
    W4_CASE(true, 4, 4, 2, 2) W4_CASE(true, 4, 4, 4, 2) W4_CASE(true, 4, 4, 2, 4)
    default: return CC_ERR_UNSUPPORTED;
  }
#undef W4_CASE
  CC_LAUNCH_CHECK();
  return CC_OK;
}

static int launch_gemv_w4_t(const GemvW4Args& a, int nt, hipStream_t st) {
  switch (nt) {
    case 1: return launch_gemv_w4<1>(a, st);  // one token: the single-vector kernel itself
    case 2: return launch_gemv_w4<2>(a, st);
    case 3: return launch_gemv_w4<3>(a, st);
    default: return launch_gemv_w4<4>(a, st);
  }
}

}  // namespace

static inline bool w4_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the checks of both entry points, in one order; ALIGN: the multi entry point's pointer alignment conditions
template <bool ALIGN>
static int gemv_fused_w4_entry(const uint8_t* W, const void* qparams, const uint8_t* W3, const void* qparams3, const void* x,
                               const void* delta, const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs,
                               int32_t rope_rows, int32_t head_dim, void* y, int32_t N, int32_t K, int32_t groupsize, int32_t T,
                               int32_t dtype, cc_stream_t stream) {
  if (!qparams || (W3 != nullptr) != (qparams3 != nullptr)) return CC_ERR_BAD_ARG;
  const int gshift = groupsize == 32 ? 0 : groupsize == 64 ? 1 : groupsize == 128 ? 2 : groupsize == 256 ? 3 : -1;
  if (gshift < 0) return CC_ERR_BAD_ARG;
  // 16-byte vector accesses to the codes, the input vectors and the prologue's operands, 32-bit (scale, zero) words (null: aligned).
  // (row t of x / delta / h_out starts K * 2 bytes behind row t - 1: K % 32 == 0 keeps every row as aligned as the first)
  if (ALIGN && (!w4_aligned(W, 16) || !w4_aligned(W3, 16) || !w4_aligned(x, 16) || !w4_aligned(delta, 16) || !w4_aligned(norm_w, 16) ||
                !w4_aligned(h_out, 16) || !w4_aligned(qparams, 4) || !w4_aligned(qparams3, 4)))
    return CC_ERR_BAD_ARG;
  if (const int rc = gv_check_args(W, W3, x, delta, norm_w, h_out, bias, freqs, rope_rows, head_dim, y, N, K, T, dtype)) return rc;
  if (dtype != CC_DT_BF16) return CC_ERR_UNSUPPORTED;  // bf16 models only (the reference's int4 kernel is bf16-only)
  if (K % groupsize) return CC_ERR_UNSUPPORTED;
  GemvW4Args a{W, W3, reinterpret_cast<const uint32_t*>(qparams), reinterpret_cast<const uint32_t*>(qparams3), x, delta, norm_w, bias,
               freqs, h_out, y, eps, N, K, gshift, freqs ? rope_rows : 0, freqs ? head_dim : 2};
  return launch_gemv_w4_t(a, T, (hipStream_t)stream);
}

extern "C" int cc_gemv_fused_w4(const uint8_t* W, const void* qparams, const uint8_t* W3, const void* qparams3, const void* x,
                                const void* delta, const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs,
                                int32_t rope_rows, int32_t head_dim, void* y, int32_t N, int32_t K, int32_t groupsize, int32_t dtype,
                                cc_stream_t stream) {
  CC_ENTRY();
  return gemv_fused_w4_entry<false>(W, qparams, W3, qparams3, x, delta, norm_w, eps, h_out, bias, freqs, rope_rows, head_dim, y, N, K,
                                    groupsize, 1, dtype, stream);
}

extern "C" int cc_gemv_fused_w4_multi(const uint8_t* W, const void* qparams, const uint8_t* W3, const void* qparams3, const void* x,
                                      const void* delta, const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs,
                                      int32_t rope_rows, int32_t head_dim, void* y, int32_t N, int32_t K, int32_t groupsize, int32_t T,
                                      int32_t dtype, cc_stream_t stream) {
  CC_ENTRY();
  return gemv_fused_w4_entry<true>(W, qparams, W3, qparams3, x, delta, norm_w, eps, h_out, bias, freqs, rope_rows, head_dim, y, N, K,
                                   groupsize, T, dtype, stream);
}
