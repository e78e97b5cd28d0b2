// cc_gemv.hip — the five dense matrix-vector products of a decode layer, with the caller glue fused in:
//   wqkv : RMSNorm(x + delta) prologue (the pending residual add included) + RoPE epilogue on the q / k rows
//   wo   : plain
//   w1/w3: RMSNorm prologue + SwiGLU epilogue  silu(w1·n) * (w3·n)  (one pass over both matrices)
//   w2   : plain
// ref (caller side): model.py:317-327 (pre-norm block), :375-387 (split + apply_rotary_emb), :442-443 (FFN),
// :452-457 (RMSNorm), :507-519 (RoPE).  Eleven launches per layer become six; every rounding point of the eager
// bf16 chain is kept (each tensor op rounds to the model dtype).
//
// HBM-bound streaming of W (batch 1: 2 flops per 2-byte weight).  One WAVE owns a row at a time: its 64 lanes
// stride over K with 16-byte loads (one fully coalesced 1 KiB segment per load instruction), RB rows and CU
// column steps are in flight together (RB*CU 16-byte loads per lane), products go through v_dot2c_f32_bf16 /
// v_dot2_f32_f16 (fp32 accumulate), the row total through 4 DPP steps + 4 v_readlane.  The input vector is
// normalised ONCE per workgroup into LDS as packed 16-bit (every workgroup recomputes the 8 KiB norm rather than
// paying a launch for it) and kept in the registers of the lanes that multiply it.  No atomics, fixed orders.
#include <cstdio>
#include <cstdlib>

#include "cc_common.h"
#include "cc_gemv_core.h"

namespace {

constexpr int kGvThreads = 256;
constexpr int kGvWaves = kGvThreads / 64;
static_assert(kGvThreads == kGvCoreThreads, "gemv_body's workgroup");

template <typename T, bool SWIGLU, int RB, int CU, int XS>
__global__ __launch_bounds__(kGvThreads) void gemv_kernel(GemvArgs a) {
  // (the body, shared with the 12-bit packed form: cc_gemv_core.h)
  constexpr int VEC = 16 / (int)sizeof(T);
  const int N = a.N, nch = a.K / VEC;
  const int nstep = ((nch + 63) / 64 + kGvWaves - 1) / kGvWaves;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint4* Wv = reinterpret_cast<const uint4*>(a.W);
  const uint4* W3v = reinterpret_cast<const uint4*>(a.W3);
  uint4 w[RB][CU], w3[RB][CU];
  auto issue = gv_plain_tile<SWIGLU>(w, w3, Wv, W3v, N, nch, nstep, lane, wave);
  auto get = [&](int r, int u) { return w[r][u]; };
  auto get3 = [&](int r, int u) { return w3[r][u]; };
  gemv_body<T, SWIGLU, RB, CU, XS>(a, issue, get, get3);
}

// tuning hook: CC_GEMV_CFG="RB,CU[,max workgroups]" (read once per process) -> true and the geometry it names
static bool env_cfg(GvCfg* c) {
  static int env_rb = -1, env_cu = -1, env_cap = 2048;
  if (env_rb < 0) {
    env_rb = env_cu = 0;
    if (const char* e = getenv("CC_GEMV_CFG")) sscanf(e, "%d,%d,%d", &env_rb, &env_cu, &env_cap);
  }
  if (env_rb <= 0 || env_cu <= 0) return false;
  *c = {env_rb, env_cu, env_cap};
  return true;
}

static GvCfg pick_cfg(const GemvArgs& a, int vec) {
  GvCfg env;
  if (env_cfg(&env)) return env;
  const int nseg = (a.K / vec + 63) / 64, nstep = (nseg + kGvWaves - 1) / kGvWaves;
  // measured on MI355X (tools/bench_gemv.py): 2 rows x 2 segments per wave for the SwiGLU pair at K = 4096 (w1 + w3 39.5 us =
  // 5.95 TB/s), 4 x 4 for K = 14336 (w2 20.9 us)
  GvCfg c;
  c.cap = 2048;
  if (nstep <= 2 && a.W3 == nullptr) {
    // r5 (same-box sweeps, tools/bench_gemv.py with CC_GEMV_CFG, two repetitions each): 4 rows per workgroup and 1024 workgroups — 8
    // loads in flight per lane, four workgroups per CU — instead of 2 rows and 2048: wqkv with its norm prologue and RoPE epilogue
    // 12.25 -> 11.0 us, wo 8.14 -> 7.86 (2048 / 1536 / 1280 / 896 / 768 / 640 / 512 workgroups: 12.4 / 12.4 / 12.1 / 11.5 / 11.6 /
    // 12.0 / 12.7; 8 rows: 11.8-11.9); the LM head (128256 rows: 125 rounds per workgroup) prefers 2 rows x 1024: 163.4 -> 157.7.
    // The arithmetic of a row does not depend on either number: bit-identical results.  (Also tried, r5: the SwiGLU pair as one wave
    // per row pair — 256 workgroups x 8 waves, no LDS, no barrier, the geometry at which a stream-only launch moves the pair's 235 MB
    // in 37.1 us: 41.1-41.4 us against this kernel's 40.0; removed.)
    if (a.N >= 32768) {
      c.rb = 2; c.cu = 2;
    } else {
      c.rb = 4; c.cu = 2;
    }
    c.cap = 1024;
  } else if (nstep <= 2) {
    c.rb = 2; c.cu = 2;
  } else if (a.W3 != nullptr) {
    c.rb = 2; c.cu = (nstep <= 4 || nstep > 8) ? 4 : 8;
  } else {
    c.rb = 4; c.cu = 4;
    c.cap = 512;  // long rows: two workgroups per CU looping over row groups (w2: 21.1 vs 21.8 us at 1024+)
  }
  return c;
}

// ---- the same product for NT input vectors from ONE pass over the weights (cc_gemv_fused_multi): blocks of decode steps whose
//      input tokens are known (teacher forcing, the tail of a long prompt) need not stream W once per token.  Row t of y / h_out is
//      BIT-IDENTICAL to gemv_kernel on row t of x / delta / freqs: the lane that owns a 16-byte chunk, the order of a lane's Dot16
//      chain, gv_wave_sum, the four-wave meet (p0 + p1) + (p2 + p3) and every rounding point of the prologue and the epilogue are
//      gemv_kernel's, kept per token — a weight register loaded once feeds NT accumulator chains instead of one.  None of that
//      depends on RB, CU or the grid, so the launcher is free to choose them by the register budget (NT * XS input chunks per lane).
//      x, delta, h_out: [NT, K]; y: [NT, N]; freqs: [NT, head_dim / 2, 2].  A plain grid: no workgroup waits for another.
template <typename T, bool SWIGLU, int RB, int CU, int XS, int NT>
__global__ __launch_bounds__(kGvThreads) void gemv_multi_kernel(GemvArgs a) {
  constexpr int VEC = 16 / (int)sizeof(T);
  static_assert(NT * RB <= 64, "wave 0 finishes one (token, row) per lane");
  __shared__ float sm_red[NT][kGvWaves];
  __shared__ float sm_part[NT][kGvWaves][2][RB];
  const int K = a.K, N = a.N;
  const int nch = K / VEC;
  const T* xg = reinterpret_cast<const T*>(a.x);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  // ---- work decomposition and the weight tile: gemv_kernel's (the first tile is requested before the inputs are touched)
  const int nseg = (nch + 63) / 64;
  const int nstep = (nseg + kGvWaves - 1) / kGvWaves;
  const uint4* Wv = reinterpret_cast<const uint4*>(a.W);
  const uint4* W3v = reinterpret_cast<const uint4*>(a.W3);
  uint4 w[RB][CU], w3[RB][CU];
  auto issue = gv_plain_tile<SWIGLU>(w, w3, Wv, W3v, N, nch, nstep, lane, wave);
  const int row_first = blockIdx.x * RB;
  if (row_first < N) issue(row_first, 0);

  // ---- the NT input vectors: every lane keeps the chunks it will multiply, of every token (NT * XS uint4).  The norm prologue
  //      runs per token (NT sums of squares, ONE barrier); chunk by chunk, so that only one chunk's x / delta of every token is
  //      live beside the kept registers.  A token's sum of squares still runs over its chunks in gemv_kernel's order.
  uint4 xr[NT][XS];
  if (a.norm_w != nullptr) {
    const T* dg = reinterpret_cast<const T*>(a.delta);
    const T* wg = reinterpret_cast<const T*>(a.norm_w);
    // (fp32 at 16 chunks and 3 or 4 tokens: the norm weight's chunks are read again behind the barrier instead of being kept — the
    //  64 registers they would take are what that instantiation lacks)
    constexpr bool KEEP_NV = !(sizeof(T) == 4 && XS == 16 && NT >= 3);
    Vec16<T> nv[KEEP_NV ? XS : 1];
    float ss[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) ss[t] = 0.f;
#pragma unroll
    for (int j = 0; j < XS; j++) {
      const int c = (j * kGvWaves + wave) * 64 + lane;
      const bool in = j < nstep && c < nch;
      if (KEEP_NV && in) nv[KEEP_NV ? j : 0].load(wg + (size_t)c * VEC);
#pragma unroll
      for (int t = 0; t < NT; t++) {
        xr[t][j] = make_uint4(0, 0, 0, 0);
        if (in) {
          const size_t at = (size_t)t * K + (size_t)c * VEC;
          Vec16<T> xv, dv;
          xv.load(xg + at);
          if (dg != nullptr) dv.load(dg + at);
          float h[VEC];
          xv.unpack(h);
          if (dg != nullptr) {
            float d[VEC];
            dv.unpack(d);
#pragma unroll
            for (int e = 0; e < VEC; e++) h[e] = ElemTraits<T>::rnd(__fadd_rn(h[e], d[e]));  // model-dtype residual add
          }
#pragma unroll
          for (int e = 0; e < VEC; e++) ss[t] = fmaf(h[e], h[e], ss[t]);
          xr[t][j] = pack16<T>(h);
          if (a.h_out != nullptr && blockIdx.x == 0) reinterpret_cast<uint4*>(a.h_out)[(size_t)t * nch + c] = xr[t][j];
        }
      }
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const float s = gv_wave_sum(ss[t]);
      if (lane == 0) sm_red[t][wave] = s;
    }
    __syncthreads();
    float rs[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const float tot = (sm_red[t][0] + sm_red[t][1]) + (sm_red[t][2] + sm_red[t][3]);
      rs[t] = rsqrtf(tot / (float)K + a.eps);
    }
#pragma unroll
    for (int j = 0; j < XS; j++) {
      const int c = (j * kGvWaves + wave) * 64 + lane;
      if (j < nstep && c < nch) {
        float wf[VEC];
        if (KEEP_NV) {
          nv[KEEP_NV ? j : 0].unpack(wf);
        } else {
          Vec16<T> n;
          n.load(wg + (size_t)c * VEC);
          n.unpack(wf);
        }
#pragma unroll
        for (int t = 0; t < NT; t++) {
          Vec16<T> hv;
          float h[VEC], o[VEC];
          hv.raw = xr[t][j];
          hv.unpack(h);
#pragma unroll
          for (int e = 0; e < VEC; e++) o[e] = ElemTraits<T>::rnd(__fmul_rn(ElemTraits<T>::rnd(cc_opaque_f32(__fmul_rn(h[e], rs[t]))), wf[e]));
          xr[t][j] = pack16<T>(o);
        }
      }
    }
  } else {
#pragma unroll
    for (int t = 0; t < NT; t++) {
#pragma unroll
      for (int j = 0; j < XS; j++) {
        const int c = (j * kGvWaves + wave) * 64 + lane;
        xr[t][j] = (j < nstep && c < nch) ? reinterpret_cast<const uint4*>(xg)[(size_t)t * nch + c] : make_uint4(0, 0, 0, 0);
      }
    }
  }

  T* yo = reinterpret_cast<T*>(a.y);
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
#pragma unroll
          for (int t = 0; t < NT; t++) {
            const uint4 xv = xr[t][s0 + u < XS ? s0 + u : XS - 1];  // beyond nstep the weights are zero-filled
#pragma unroll
            for (int r = 0; r < RB; r++) {
              acc[t][r] = Dot16<T>::run(w[r][u], xv, acc[t][r]);
              if (SWIGLU) acc3[t][r] = Dot16<T>::run(w3[r][u], xv, acc3[t][r]);
            }
          }
        }
      }
    }
    // ---- the four K-quarters of every (token, row) meet in LDS (fixed order: deterministic)
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
    if (wave == 0) {
      float out = 0.f;  // lane t * RB + r finishes row r0 + r of token t (RB is even: a RoPE pair stays in lanes l, l ^ 1)
      const bool mine = lane < NT * RB;
      const int t = mine ? lane / RB : 0;
      const int r = mine ? lane % RB : 0;
      float s = (sm_part[t][0][0][r] + sm_part[t][1][0][r]) + (sm_part[t][2][0][r] + sm_part[t][3][0][r]);
      const int row = r0 + r;
      if (a.bias != nullptr && row < N) s += ElemTraits<T>::load(reinterpret_cast<const T*>(a.bias), (size_t)row);
      s = ElemTraits<T>::rnd(cc_opaque_f32(s));  // (opaque, here and below: gemv_kernel's rounding points)
      if (SWIGLU) {
        const float s3 = ElemTraits<T>::rnd((sm_part[t][0][1][r] + sm_part[t][1][1][r]) + (sm_part[t][2][1][r] + sm_part[t][3][1][r]));
        const float sl = ElemTraits<T>::rnd(__fdiv_rn(s, 1.0f + expf(-s)));
        s = __fmul_rn(sl, s3);
      }
      out = s;
      if (a.freqs != nullptr) {
        const float other = gv_dpp<0xB1>(out);
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

// The geometry of a multi launch: pick_cfg's choice for the shape, with fewer rows / column steps in flight where NT * XS input
// chunks per lane leave no room for it (results do not depend on either number).  Only fp32 needs it (DESIGN.md §2.10 has the
// register figures of every instantiation): 16 chunks x 3 tokens fit at 2 x 2, and 4 x 8 at 8 chunks x 4 tokens becomes 4 x 4.
//
// 16-bit rows at 3 and 4 tokens (profiles/gemv_multi_geometry.md: a same-session sweep of every geometry the table builds without
// scratch over the 8B model's four decode shapes, bf16; each choice below beat pick_cfg's by more than the spread of pick_cfg's own
// five runs; nothing qualified at T = 2, and the wo shape keeps pick_cfg's choice at every T).  A 256-thread workgroup is one wave
// per SIMD, and the registers of an instantiation set how many workgroups a CU holds (§2.11's table):
//   - long rows (w2, XS = 8) at T = 4: 4 x 4 takes 260 registers — one wave per SIMD — and 2 x 4 takes 228, two: 31.0 -> 23.3 us;
//   - the SwiGLU pair at K <= 4096 and T >= 3: 2 x 2 takes 90 / 104 registers, 5 / 4 workgroups per CU, so 2048 workgroups are
//     a second, partial round of residency; 1024 are all resident and loop: 44.7 -> 42.5 us (T = 3), 50.9 -> 46.1 (T = 4);
//   - short plain rows whose row groups are no whole number of rounds of the 1024 (wqkv: 1536 groups of 4 rows) at T >= 3: 512
//     workgroups run three whole rounds: 16.7 -> 15.9 us (T = 3), 18.9 -> 17.3 (T = 4).
// CC_GEMV_CFG names the geometry itself: none of these applies under it.
static GvCfg pick_multi_cfg(const GemvArgs& a, int vec, int xs, int nt) {
  GvCfg c = pick_cfg(a, vec);
  GvCfg env;
  if (vec == 8 && nt >= 3 && !env_cfg(&env)) {
    const int groups = (a.N + c.rb - 1) / c.rb;
    if (xs == 8 && a.W3 == nullptr && nt == 4 && c.rb == 4 && c.cu == 4) c.rb = 2;
    else if (xs == 2 && a.W3 != nullptr && c.cap > 1024) c.cap = 1024;
    else if (xs == 2 && a.W3 == nullptr && a.N < 32768 && groups > c.cap && groups % c.cap != 0) c.cap = 512;
  }
  if (vec == 4 && xs == 16 && nt >= 3) c.rb = c.cu = 2;
  if (vec == 4 && xs == 8 && nt == 4 && c.rb == 4 && c.cu == 8) c.cu = 4;
  return c;
}

template <typename T, bool SWIGLU, int RB, int CU, int XS, int NT>
static void launch_cfg(const GemvArgs& a, hipStream_t st, int cap) {
  int blocks = (a.N + RB - 1) / RB;
  if (blocks > cap) blocks = cap;
  if constexpr (NT == 1) {
    hipLaunchKernelGGL((gemv_kernel<T, SWIGLU, RB, CU, XS>), dim3(blocks), dim3(kGvThreads), 0, st, a);
  } else {
    hipLaunchKernelGGL((gemv_multi_kernel<T, SWIGLU, RB, CU, XS, NT>), dim3(blocks), dim3(kGvThreads), 0, st, a);
  }
}

// NT = 1: the single-vector kernel (pick_multi_cfg is pick_cfg there, and every instantiation of the table is built)
template <typename T, int NT>
static int launch_gemv(const GemvArgs& a, hipStream_t st) {
  const int vec = 16 / (int)sizeof(T);
  const int nseg = (a.K / vec + 63) / 64, nstep = (nseg + kGvWaves - 1) / kGvWaves;
  const int xs = nstep <= 2 ? 2 : nstep <= 8 ? 8 : 16;  // input chunks kept per lane
  const GvCfg c = pick_multi_cfg(a, vec, xs, NT);
  if (nstep > 16 || c.cu > xs) return CC_ERR_UNSUPPORTED;
  const int key = (a.W3 ? 100000 : 0) + xs * 1000 + c.rb * 10 + c.cu;
  // (instantiations that would spill are not built: pick_multi_cfg never selects them)
  constexpr bool kF32 = sizeof(T) == 4;
  constexpr bool kWide16 = !(kF32 && NT >= 3), kNarrow16 = kF32 && NT == 3, kWide8 = !(kF32 && NT == 4);
  switch (key) {
    case 2022: launch_cfg<T, false, 2, 2, 2, NT>(a, st, c.cap); break;
    case 2042: launch_cfg<T, false, 4, 2, 2, NT>(a, st, c.cap); break;
    case 2082: launch_cfg<T, false, 8, 2, 2, NT>(a, st, c.cap); break;
    case 8022: launch_cfg<T, false, 2, 2, 8, NT>(a, st, c.cap); break;
    case 8024: launch_cfg<T, false, 2, 4, 8, NT>(a, st, c.cap); break;
    case 8044: launch_cfg<T, false, 4, 4, 8, NT>(a, st, c.cap); break;
    case 8028: launch_cfg<T, false, 2, 8, 8, NT>(a, st, c.cap); break;
    case 8048:
      if constexpr (kWide8) launch_cfg<T, false, 4, 8, 8, NT>(a, st, c.cap); else return CC_ERR_UNSUPPORTED;
      break;
    case 16044:
      if constexpr (kWide16) launch_cfg<T, false, 4, 4, 16, NT>(a, st, c.cap); else return CC_ERR_UNSUPPORTED;
      break;
    case 16028:
      if constexpr (kWide16) launch_cfg<T, false, 2, 8, 16, NT>(a, st, c.cap); else return CC_ERR_UNSUPPORTED;
      break;
    case 16022:
      if constexpr (kNarrow16) launch_cfg<T, false, 2, 2, 16, NT>(a, st, c.cap); else return CC_ERR_UNSUPPORTED;
      break;
    case 102022: launch_cfg<T, true, 2, 2, 2, NT>(a, st, c.cap); break;
    case 102042: launch_cfg<T, true, 4, 2, 2, NT>(a, st, c.cap); break;
    case 108022: launch_cfg<T, true, 2, 2, 8, NT>(a, st, c.cap); break;
    case 108024: launch_cfg<T, true, 2, 4, 8, NT>(a, st, c.cap); break;
    case 108028: launch_cfg<T, true, 2, 8, 8, NT>(a, st, c.cap); break;
    case 116024:
      if constexpr (kWide16) launch_cfg<T, true, 2, 4, 16, NT>(a, st, c.cap); else return CC_ERR_UNSUPPORTED;
      break;
    case 116022:
      if constexpr (kNarrow16) launch_cfg<T, true, 2, 2, 16, NT>(a, st, c.cap); else return CC_ERR_UNSUPPORTED;
      break;
    default: return CC_ERR_UNSUPPORTED;
  }
  CC_LAUNCH_CHECK();
  return CC_OK;
}

template <typename T>
static int launch_gemv_multi_t(const GemvArgs& a, int nt, hipStream_t st) {
  switch (nt) {
    case 1: return launch_gemv<T, 1>(a, st);  // one token: the single-vector kernel itself
    case 2: return launch_gemv<T, 2>(a, st);
    case 3: return launch_gemv<T, 3>(a, st);
    default: break;
  }
  if (sizeof(T) == 4 && (size_t)a.K * sizeof(T) > 32 * 1024) {
    // fp32 rows beyond 32 KiB (16 chunks per lane): four tokens' inputs are the whole register file (256 + 256), and every
    // geometry of that instantiation spills to scratch.  Two launches of two tokens each instead: the one shape class whose
    // weights pass twice (same bits: a row's arithmetic does not depend on its neighbours)
    GemvArgs b = a;
    const size_t es = sizeof(T);
    b.x = (const char*)a.x + 2 * (size_t)a.K * es;
    if (a.delta) b.delta = (const char*)a.delta + 2 * (size_t)a.K * es;
    if (a.h_out) b.h_out = (char*)a.h_out + 2 * (size_t)a.K * es;
    if (a.freqs) b.freqs = (const char*)a.freqs + 2 * (size_t)a.head_dim * es;
    b.y = (char*)a.y + 2 * (size_t)a.N * es;
    const int rc = launch_gemv<T, 2>(a, st);
    return rc != CC_OK ? rc : launch_gemv<T, 2>(b, st);
  }
  return launch_gemv<T, 4>(a, st);
}

}  // namespace

static int gemv_fused_entry(const void* W, const void* W3, const void* x, const void* delta, const void* norm_w, float eps, void* h_out,
                            const void* bias, const void* freqs, int32_t rope_rows, int32_t head_dim, void* y, int32_t N, int32_t K,
                            int32_t T, int32_t dtype, cc_stream_t stream) {
  if (const int rc = gv_check_args(W, W3, x, delta, norm_w, h_out, bias, freqs, rope_rows, head_dim, y, N, K, T, dtype)) return rc;
  const int vec = 16 / (int)cc_dt_size(dtype);
  if (K % vec) return CC_ERR_UNSUPPORTED;
  GemvArgs a{W, W3, x, delta, norm_w, bias, freqs, h_out, y, eps, N, K, freqs ? rope_rows : 0, freqs ? head_dim : 2};
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case CC_DT_F32: return launch_gemv_multi_t<float>(a, T, st);
    case CC_DT_BF16: return launch_gemv_multi_t<bf16_t>(a, T, st);
    default: return launch_gemv_multi_t<f16_t>(a, T, st);
  }
}

extern "C" int cc_gemv_fused_multi(const void* W, const void* W3, const void* x, const void* delta, const void* norm_w, float eps,
                                   void* h_out, const void* bias, const void* freqs, int32_t rope_rows, int32_t head_dim, void* y,
                                   int32_t N, int32_t K, int32_t T, int32_t dtype, cc_stream_t stream) {
  CC_ENTRY();
  return gemv_fused_entry(W, W3, x, delta, norm_w, eps, h_out, bias, freqs, rope_rows, head_dim, y, N, K, T, dtype, stream);
}

extern "C" int cc_gemv_fused(const void* W, const void* W3, const void* x, const void* delta, const void* norm_w, float eps,
                             void* h_out, const void* bias, const void* freqs, int32_t rope_rows, int32_t head_dim, void* y,
                             int32_t N, int32_t K, int32_t dtype, cc_stream_t stream) {
  CC_ENTRY();
  return gemv_fused_entry(W, W3, x, delta, norm_w, eps, h_out, bias, freqs, rope_rows, head_dim, y, N, K, 1, dtype, stream);
}
