// cc_gemv_core.h — the arithmetic of the streamed matrix-vector products (cc_gemv.hip), shared with the single-launch layer step
// that folds the layer's QKV projection in (cc_attn_decode_qkv.hip): the SAME products, chains and reduction orders, so that the
// fused launch and the stand-alone GEMV give bit-identical q / k / v.  Also here, once for the five cc_gemv*.hip: the weight tiles of
// the two layouts (gv_plain_tile, gv_scaled_tile), the dense body (gemv_body), its prologue and epilogue as functions (gv_prologue,
// gv_epilogue), the pipelined body for long rows that calls the same two (gemv_long_body) and the entry points' shared argument
// check (gv_check_args).  DESIGN.md §2.19 lists which step lives where, and which are still one text per kernel.
#pragma once
#include "cc_common.h"

namespace {

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));

template <typename T>
struct Dot16;  // acc += <16 bytes of W, 16 bytes of x>
template <>
struct Dot16<bf16_t> {
  __device__ static __forceinline__ float run(uint4 w, uint4 x, float acc) {
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, w.x), __builtin_bit_cast(bf16x2_t, x.x), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, w.y), __builtin_bit_cast(bf16x2_t, x.y), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, w.z), __builtin_bit_cast(bf16x2_t, x.z), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, w.w), __builtin_bit_cast(bf16x2_t, x.w), acc, false);
    return acc;
  }
};
template <>
struct Dot16<f16_t> {
  __device__ static __forceinline__ float run(uint4 w, uint4 x, float acc) {
    acc = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, w.x), __builtin_bit_cast(f16x2_t, x.x), acc, false);
    acc = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, w.y), __builtin_bit_cast(f16x2_t, x.y), acc, false);
    acc = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, w.z), __builtin_bit_cast(f16x2_t, x.z), acc, false);
    acc = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, w.w), __builtin_bit_cast(f16x2_t, x.w), acc, false);
    return acc;
  }
};
template <>
struct Dot16<float> {
  __device__ static __forceinline__ float run(uint4 w, uint4 x, float acc) {
    acc = fmaf(__uint_as_float(w.x), __uint_as_float(x.x), acc);
    acc = fmaf(__uint_as_float(w.y), __uint_as_float(x.y), acc);
    acc = fmaf(__uint_as_float(w.z), __uint_as_float(x.z), acc);
    acc = fmaf(__uint_as_float(w.w), __uint_as_float(x.w), acc);
    return acc;
  }
};

template <int CTRL>
__device__ __forceinline__ float gv_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// whole-wave sum with a wave-uniform result (4 DPP steps per 16-lane row, 4 v_readlane); fixed order
__device__ __forceinline__ float gv_wave_sum(float v) {
  v += gv_dpp<0xB1>(v);
  v += gv_dpp<0x4E>(v);
  v += gv_dpp<0x141>(v);
  v += gv_dpp<0x140>(v);
  const int u = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(u, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(u, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(u, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(u, 48));
  return (r0 + r1) + (r2 + r3);
}

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 nt_load(const uint4* p) {  // streamed once per token: do not keep it in L2 / MALL
  const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
  return make_uint4(v.x, v.y, v.z, v.w);
}

template <typename T>
__device__ __forceinline__ uint4 pack16(const float* f) {
  if constexpr (sizeof(T) == 4) {
    return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
  } else {
    T e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) ElemTraits<T>::store(&e[i], 0, f[i]);
    return make_uint4((uint32_t)e[0].x | ((uint32_t)e[1].x << 16), (uint32_t)e[2].x | ((uint32_t)e[3].x << 16),
                      (uint32_t)e[4].x | ((uint32_t)e[5].x << 16), (uint32_t)e[6].x | ((uint32_t)e[7].x << 16));
  }
}

constexpr int kGvCoreThreads = 256;  // the workgroup gemv_body is written for: four waves split a row's segments
constexpr int kGvCoreWaves = kGvCoreThreads / 64;

// ---- the weight tile of a wave, once for every kernel of a layout (single and multi forms of a format share it, and with it the
//      chunk ownership): the returned issue(r0, s0) requests RB rows from r0 x CU column steps from s0 into w / w3, zero-filled
//      outside the matrix.  It refers to the kernel's own variables, so they must outlive it.
//      Non-temporal: 15 GB of weights pass once per token, nothing is gained by keeping them in L2 / the 256 MB Infinity Cache
//      (measured: w1+w3 43.1 -> 40.1 us, w2 24.8 -> 22.5 us).
//      The PLAIN layout (dense, int8): the four waves of a workgroup split every row's 1 KiB segments.
template <bool SWIGLU, int RB, int CU>
__device__ __forceinline__ auto gv_plain_tile(uint4 (&w)[RB][CU], uint4 (&w3)[RB][CU], const uint4* const& Wv, const uint4* const& W3v,
                                              const int& N, const int& nch, const int& nstep, const int& lane, const int& wave) {
  return [&](int r0, int s0) {
#pragma unroll
    for (int u = 0; u < CU; u++) {
      const int c = ((s0 + u) * kGvCoreWaves + wave) * 64 + lane;
      const bool cin = (s0 + u < nstep) && c < nch;
#pragma unroll
      for (int r = 0; r < RB; r++) {
        const bool in = cin && (r0 + r < N);
        const size_t off = (size_t)(r0 + r) * nch + c;
        w[r][u] = in ? nt_load(Wv + off) : make_uint4(0, 0, 0, 0);
        if (SWIGLU) w3[r][u] = in ? nt_load(W3v + off) : make_uint4(0, 0, 0, 0);
      }
    }
  };
}
//      The SCALED layout (int4, MXFP4): WS waves per row (wave ws of them takes segments ws, ws + WS, ...), r0 is this wave's first
//      row, and a 32-bit scale word travels beside every chunk, read from the format's table sc (sc3 for W3): GROUPED, the word of
//      the chunk's group, sc[row * ngr + (c >> gshift)]; otherwise the chunk's own, sc[row * nch + c] (ngr and gshift are not read).
//      FILL stands beside zero-filled codes.
template <bool SWIGLU, int WS, bool GROUPED, uint32_t FILL, int RB, int CU, typename P>
__device__ __forceinline__ auto gv_scaled_tile(uint4 (&w)[RB][CU], uint4 (&w3)[RB][CU], uint32_t (&q)[RB][CU], uint32_t (&q3)[RB][CU],
                                               const uint4* const& Wv, const uint4* const& W3v, const P* const& sc, const P* const& sc3,
                                               const int& N, const int& nch, const int& nstep, const int& lane, const int& ws,
                                               const int& ngr, const int& gshift) {
  return [&](int r0, int s0) {
#pragma unroll
    for (int u = 0; u < CU; u++) {
      const int c = ((s0 + u) * WS + ws) * 64 + lane;
      const bool cin = (s0 + u < nstep) && c < nch;
#pragma unroll
      for (int r = 0; r < RB; r++) {
        const bool in = cin && (r0 + r < N);
        const size_t off = (size_t)(r0 + r) * nch + c;
        const size_t qoff = GROUPED ? (size_t)(r0 + r) * ngr + (c >> gshift) : off;
        w[r][u] = in ? nt_load(Wv + off) : make_uint4(0, 0, 0, 0);
        q[r][u] = in ? (uint32_t)__builtin_nontemporal_load(sc + qoff) : FILL;
        if (SWIGLU) {
          w3[r][u] = in ? nt_load(W3v + off) : make_uint4(0, 0, 0, 0);
          q3[r][u] = in ? (uint32_t)__builtin_nontemporal_load(sc3 + qoff) : FILL;
        }
      }
    }
  };
}

// ---- the single-vector GEMV (cc_gemv.hip's gemv_kernel) as a body over three callables of the kernel that owns the weight
//      registers: issue(r0, s0) requests a wave's RB x CU weight chunks, get(r, u) / get3(r, u) hand one of them out as 16 bytes of
//      T.  gemv_kernel reads them from the dense tensor; cc_gemv_w12.hip rebuilds the same 16 bytes from the 12-bit packed copy.
//      Prologue, Dot16 chains, reductions and epilogue exist once, here.
struct GemvArgs {
  const void* W;
  const void* W3;      // second matrix of the SwiGLU pair, or null
  const void* x;       // [K]
  const void* delta;   // [K] pending residual, or null
  const void* norm_w;  // [K] RMSNorm weight, or null (no norm prologue)
  const void* bias;    // [N] or null
  const void* freqs;   // [head_dim/2, 2] (cos, sin) of this position, or null
  void* h_out;         // [K] x + delta, or null
  void* y;             // [N]
  float eps;
  int N, K, rope_rows, head_dim;
};

// ---- the prologue of every single-vector body: the input vector.  Every lane keeps exactly the 16-byte chunks it will multiply
//      (no LDS staging).  With a norm prologue, x / delta / norm weight of those chunks are requested together (one memory round
//      trip), the four waves exchange their partial sums of squares through LDS (one barrier), and the normalised chunks replace h
//      in the same registers.  sm_red: kGvCoreWaves floats of the caller's LDS.
template <typename T, int XS>
__device__ __forceinline__ void gv_prologue(const GemvArgs& a, float* sm_red, uint4 (&xr)[XS], int nch, int nstep, int lane, int wave) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int K = a.K;
  const T* xg = reinterpret_cast<const T*>(a.x);
  if (a.norm_w != nullptr) {
    const T* dg = reinterpret_cast<const T*>(a.delta);
    const T* wg = reinterpret_cast<const T*>(a.norm_w);
    Vec16<T> xv[XS], dv[XS], nv[XS];
#pragma unroll
    for (int j = 0; j < XS; j++) {
      const int c = (j * kGvCoreWaves + wave) * 64 + lane;
      if (j < nstep && c < nch) {
        xv[j].load(xg + (size_t)c * VEC);
        if (dg != nullptr) dv[j].load(dg + (size_t)c * VEC);
        nv[j].load(wg + (size_t)c * VEC);
      }
    }
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < XS; j++) {
      const int c = (j * kGvCoreWaves + wave) * 64 + lane;
      xr[j] = make_uint4(0, 0, 0, 0);
      if (j < nstep && c < nch) {
        float h[VEC];
        xv[j].unpack(h);
        if (dg != nullptr) {
          float d[VEC];
          dv[j].unpack(d);
#pragma unroll
          for (int e = 0; e < VEC; e++) h[e] = ElemTraits<T>::rnd(__fadd_rn(h[e], d[e]));  // model-dtype residual add
        }
#pragma unroll
        for (int e = 0; e < VEC; e++) ss = fmaf(h[e], h[e], ss);
        xr[j] = pack16<T>(h);  // h is already rounded to T: packing is exact
        if (a.h_out != nullptr && blockIdx.x == 0) reinterpret_cast<uint4*>(a.h_out)[c] = xr[j];
      }
    }
    ss = gv_wave_sum(ss);
    if (lane == 0) sm_red[wave] = ss;
    __syncthreads();
    const float tot = (sm_red[0] + sm_red[1]) + (sm_red[2] + sm_red[3]);
    const float rs = rsqrtf(tot / (float)K + a.eps);  // ref: model.py:452-457 (fp32 inside)
#pragma unroll
    for (int j = 0; j < XS; j++) {
      const int c = (j * kGvCoreWaves + wave) * 64 + lane;
      if (j < nstep && c < nch) {
        Vec16<T> hv;
        float h[VEC], wf[VEC], o[VEC];
        hv.raw = xr[j];
        hv.unpack(h);
        nv[j].unpack(wf);
#pragma unroll
        for (int e = 0; e < VEC; e++) o[e] = ElemTraits<T>::rnd(__fmul_rn(ElemTraits<T>::rnd(cc_opaque_f32(__fmul_rn(h[e], rs))), wf[e]));  // (opaque: see the epilogue)
        xr[j] = pack16<T>(o);
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < XS; j++) {
      const int c = (j * kGvCoreWaves + wave) * 64 + lane;
      xr[j] = (j < nstep && c < nch) ? reinterpret_cast<const uint4*>(xg)[c] : make_uint4(0, 0, 0, 0);
    }
  }
}

// ---- the end of a row group in every single-vector body: the four K-quarters of every row meet in LDS (fixed order:
//      deterministic), then lane r of wave 0 finishes row r0 + r (bias, rounding to the model dtype, SwiGLU, RoPE, store).
//      sm_part: the caller's LDS, reused by the next row group (the second barrier).
template <typename T, bool SWIGLU, int RB>
__device__ __forceinline__ void gv_epilogue(const GemvArgs& a, float (*sm_part)[2][RB], const float (&acc)[RB], const float (&acc3)[RB],
                                            int r0, int lane, int wave) {
  const int N = a.N;
  T* yo = reinterpret_cast<T*>(a.y);
  {
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
      float out = 0.f;  // lane r finishes row r0 + r
      const int r = lane < RB ? lane : 0;
      float s = (sm_part[0][0][r] + sm_part[1][0][r]) + (sm_part[2][0][r] + sm_part[3][0][r]);
      const int row = r0 + r;
      if (a.bias != nullptr && row < N) s += ElemTraits<T>::load(reinterpret_cast<const T*>(a.bias), (size_t)row);
      // (cc_opaque_f32: the fp32 value first, THEN its rounding — otherwise the f16 instantiations may fuse the bias add / the
      //  rotation with the conversion into one v_fma_mix rounding, differently in different kernels: the QKV form of the layer step,
      //  cc_attn_decode_qkv.hip, runs these operations too and must give the same bits)
      s = ElemTraits<T>::rnd(cc_opaque_f32(s));  // the Linear's output in the model dtype
      if (SWIGLU) {
        const float s3 = ElemTraits<T>::rnd((sm_part[0][1][r] + sm_part[1][1][r]) + (sm_part[2][1][r] + sm_part[3][1][r]));
        const float sl = ElemTraits<T>::rnd(__fdiv_rn(s, 1.0f + expf(-s)));  // F.silu -> dtype (model.py:443)
        s = __fmul_rn(sl, s3);
      }
      out = s;
      if (a.freqs != nullptr) {  // RoPE on the (even, odd) row pairs of the q / k heads (model.py:507-519)
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

template <typename T, bool SWIGLU, int RB, int CU, int XS, typename ISSUE, typename GET, typename GET3>
__device__ __forceinline__ void gemv_body(const GemvArgs& a, ISSUE&& issue, GET&& get, GET3&& get3) {
  constexpr int VEC = 16 / (int)sizeof(T);
  __shared__ float sm_red[kGvCoreWaves];
  __shared__ float sm_part[kGvCoreWaves][2][RB];
  const int N = a.N;
  const int nch = a.K / VEC;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  // ---- Work decomposition: a WORKGROUP owns RB consecutive rows at a time; its four waves split K (wave w takes
  //      the 1 KiB segments w, w+4, w+8, ... of every row), CU segments per row in flight per wave, and the four
  //      partial sums meet in LDS.  For the decode shapes this puts a whole matrix in flight in one phase
  //      (wo: 2 rows x 2 segments per wave; w2: 4 rows x 4 of 7 segments) instead of looping inside a wave.
  //      The FIRST tile's weight loads are issued before the input vector is touched: W does not depend on x.
  const int nseg = (nch + 63) / 64;                      // 1 KiB segments per row
  const int nstep = (nseg + kGvCoreWaves - 1) / kGvCoreWaves;    // segments per wave (<= XS, checked by the launcher)
  const int row_first = blockIdx.x * RB;
  if (row_first < N) issue(row_first, 0);

  uint4 xr[XS];
  gv_prologue<T, XS>(a, sm_red, xr, nch, nstep, lane, wave);

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
          const uint4 xv = xr[s0 + u < XS ? s0 + u : XS - 1];  // beyond nstep the weights are zero-filled
#pragma unroll
          for (int r = 0; r < RB; r++) {
            acc[r] = Dot16<T>::run(get(r, u), xv, acc[r]);
            if (SWIGLU) acc3[r] = Dot16<T>::run(get3(r, u), xv, acc3[r]);
          }
        }
      }
    }
    gv_epilogue<T, SWIGLU, RB>(a, sm_part, acc, acc3, r0, lane, wave);
  }
}

// ---- the same GEMV for LONG rows (NSTEP = 3 .. 8 column steps per wave, a template argument), plain form, with its own requests in
//      flight while it works: small RB x CU tiles in TWO register sets, and the tile after the current one — the next column steps
//      of this row group, or the first tile of the workgroup's next row group — is requested before the current one is consumed, so
//      a wave's requests also cross the wave sums, the LDS meet and the barriers of gv_epilogue.  Column steps beyond NSTEP are not
//      requested and not read (known at compile time: the waits count down load by load); a next row group that does not exist
//      is not requested either.  The arithmetic of a row is gemv_body's: chunk ownership, a lane's Dot16 chain over ascending column
//      steps, gv_wave_sum, the four-wave meet, prologue and epilogue (the same two functions).  Where gemv_body's long-row geometry
//      (4 column steps in flight) ends a row on zero-filled chunks, NSTEP % 4 != 0, the chain here ends on one Dot16 of zeros too.
//      Callables: issue(set, r0, s0) requests a tile into register set `set`, get(set, r, u, r0, s0) hands one of its chunks out;
//      `set` is a GvSet<0 or 1> (the sets are registers, so the choice is a type).  Tile t of a row group lives in set
//      (PAR + t) & 1, and the next row group starts where this one ended: PAR ^ (tiles & 1).
template <int V>
struct GvSet {
  static constexpr int value = V;
};

template <typename T, int RB, int CU, int NSTEP, int PAR, typename ISSUE, typename GET>
__device__ __forceinline__ void gv_long_group(const uint4 (&xr)[NSTEP], float (&acc)[RB], int r0, int r_next, int N, ISSUE&& issue, GET&& get) {
  constexpr int NT = (NSTEP + CU - 1) / CU;
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int s0 = t * CU;
    const bool even = ((PAR + t) & 1) == 0;  // (constants once unrolled: the choices of a set fold)
    if (t + 1 < NT) {
      if (even) issue(GvSet<1>(), r0, s0 + CU);
      else issue(GvSet<0>(), r0, s0 + CU);
    } else if (r_next < N) {
      if (even) issue(GvSet<1>(), r_next, 0);
      else issue(GvSet<0>(), r_next, 0);
    }
#pragma unroll
    for (int u = 0; u < CU; u++) {
      if (s0 + u < NSTEP) {
#pragma unroll
        for (int r = 0; r < RB; r++)
          acc[r] = Dot16<T>::run(even ? get(GvSet<0>(), r, u, r0, s0) : get(GvSet<1>(), r, u, r0, s0), xr[s0 + u < NSTEP ? s0 + u : 0], acc[r]);
      }
    }
  }
  if (NSTEP % 4 != 0) {
#pragma unroll
    for (int r = 0; r < RB; r++) acc[r] = Dot16<T>::run(make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), acc[r]);
  }
}

template <typename T, int RB, int CU, int NSTEP, typename ISSUE, typename GET>
__device__ __forceinline__ void gemv_long_body(const GemvArgs& a, ISSUE&& issue, GET&& get) {
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int NT = (NSTEP + CU - 1) / CU;
  __shared__ float sm_red[kGvCoreWaves];
  __shared__ float sm_part[kGvCoreWaves][2][RB];
  const int N = a.N;
  const int nch = a.K / VEC;  // ((nch + 63) / 64 + 3) / 4 == NSTEP, checked by the launcher
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row_first = blockIdx.x * RB, stride = gridDim.x * RB;
  if (row_first < N) issue(GvSet<0>(), row_first, 0);  // before the input vector is touched: W does not depend on x

  uint4 xr[NSTEP];
  gv_prologue<T, NSTEP>(a, sm_red, xr, nch, NSTEP, lane, wave);

  int par = 0;
  for (int r0 = row_first; r0 < N; r0 += stride) {
    float acc[RB], acc3[RB];
#pragma unroll
    for (int r = 0; r < RB; r++) acc[r] = acc3[r] = 0.f;
    if (NT % 2 == 0 || par == 0) gv_long_group<T, RB, CU, NSTEP, 0>(xr, acc, r0, r0 + stride, N, issue, get);
    else gv_long_group<T, RB, CU, NSTEP, 1>(xr, acc, r0, r0 + stride, N, issue, get);
    par ^= NT & 1;
    gv_epilogue<T, false, RB>(a, sm_part, acc, acc3, r0, lane, wave);
  }
}

// the geometry of a single-vector launch: rows per workgroup, column steps in flight per wave, the most workgroups
struct GvCfg {
  int rb, cu, cap;
};

// ---- the argument conditions all cc_gemv_fused* entry points share (T = 1 for a single-vector entry point).  An entry point checks
//      its own pointers and pairings before this, and what its format supports (dtype, K's multiple, alignment) after it: every
//      CC_ERR_BAD_ARG condition comes before every CC_ERR_UNSUPPORTED one.
static inline int gv_check_args(const void* W, const void* W3, const void* x, const void* delta, const void* norm_w, const void* h_out,
                                const void* bias, const void* freqs, int rope_rows, int head_dim, const void* y, int N, int K, int T,
                                int dtype) {
  if (!W || !x || !y || N <= 0 || K <= 0 || !cc_dt_ok(dtype)) return CC_ERR_BAD_ARG;
  if (T < 1 || T > CC_GEMV_MULTI_MAX_T) return CC_ERR_BAD_ARG;
  if ((delta || h_out) && !norm_w) return CC_ERR_BAD_ARG;
  if (freqs && (W3 || rope_rows < 0 || rope_rows > N || head_dim <= 0 || (head_dim & 1) || (rope_rows % head_dim))) return CC_ERR_BAD_ARG;
  if (W3 && bias) return CC_ERR_BAD_ARG;
  if ((size_t)K * cc_dt_size(dtype) > 64 * 1024) return CC_ERR_UNSUPPORTED;  // 16 input chunks per lane at most
  return CC_OK;
}

}  // namespace
