// cc_gemv_w12.hip — cc_gemv.hip's single-vector bf16 GEMV over a LOSSLESS 12-bit packed copy of the weights ("w12"): the same
// five decode-layer forms, the same bits, three quarters of the HBM bytes.
//
// A bf16 weight is 1 sign, 8 exponent and 7 mantissa bits, and a weight tensor uses few exponents.  w12 keeps sign + mantissa as
// one byte and the exponent as a 4-bit index into a window of 16 consecutive exponents that starts at a per-tensor `base`.
//
// Codes: the 16-byte chunk of 8 weights that gemv_kernel gives a lane becomes 12 bytes (three dwords), at the same chunk index:
//   dword 0, 1 : byte i = (sign << 7) | mantissa of weight i (i = 0 .. 7)
//   dword 2    : exponent indices; weight 2 j at bits [4 j, 4 j + 4), weight 2 j + 1 at bits [16 + 4 j, 16 + 4 j + 4)
// A wave's 64 lanes read 768 contiguous bytes per (row, segment) with one 12-byte load each.  A pair of weights decodes to its
// packed bf16 dword in five VALU operations as written (v_perm doubles the two bytes, v_and_or keeps sign + mantissa and places the
// base, shift + and + shifted add place the two indices; the compiler emits six).  The decoded uint4 is exactly the dense chunk and
// feeds the unchanged Dot16 chain of gemv_body (cc_gemv_core.h).  Where it pays and where it does not: DESIGN.md §2.17.
//
// Escapes: a weight whose exponent lies outside the window (±0, subnormals, inf / NaN and outliers included) keeps an arbitrary
// code and is put right after the decode from a patch record.  A record is 32 bytes, one per (row group, issue phase, wave) — the
// RB x CU chunks a wave requests at once — at a wave-uniform address requested together with the tile:
//   dword 0      : count (0 .. 7), or 0xFFFFFFFF when the tile has more than 7 escapes
//   dword 1 .. 7 : entries  (tile element r * CU + u) << 25 | lane << 19 | weight in chunk << 16 | raw bf16 bits
// The kernel keeps a record in lanes 0 .. 7 of one register and reads it with v_readlane; patching sits behind a wave-uniform
// `count != 0` branch.  An overflowing record makes its wave read the tile again from the dense
// tensor, which stays resident (prefill and the block kernels use it).  Records follow the launch geometry, so a packed tensor is
// tied to the (RB, CU) it was packed for (cc_w12_geometry).  Built and tested: K <= 16384; measured faster than the dense kernel and
// therefore on by default in the harness: the pair and the LM-head classes at K <= 4096 only (cc_w12_geometry's fifth word).
//
// A second code layout, "planar" (layout id 1; the one above is 0), keeps chunk index, records, overflow rule and dense fallback and
// splits a weight by BYTES instead of by fields, so that one operation decodes four weights.  With `base` even and B = base / 2:
//   dword 0, 1 : byte k = the low byte of bf16 weight k resp. 4 + k as it is (exponent bit 0 in bit 7, the mantissa below)
//   dword 2    : byte k = sign of weight k << 7 | ((exponent >> 1) - B) of weight 4 + k << 4 | sign of weight 4 + ((k + 3) & 3) << 3
//                | ((exponent >> 1) - B) of weight k      (the sign of weight 4 + k sits in bit 3 of byte (k + 1) & 3)
// Decode: mask 0x87878787 and add B to all four bytes at once (no carries: B + 7 <= 127) gives the high bytes of weights 0 .. 3; the
// same on the dword rotated right by 4 gives those of weights 4 .. 7; four v_perm interleave high and low bytes.  Nine operations
// per chunk against 24.  The layout of a packed copy travels in bits 8 .. 15 of the `rb` word (include/coldcompress.h).
//
// Layout id 2, "long": planar codes with the records and the launch of gemv_w12_long_kernel below — plain matrices with 3 .. 8
// column steps per wave (4096 < K <= 16384), two register sets of 2 x 2 tiles, the next tile requested before the current one is
// decoded.  On by default for w2 (seven steps) and K = 8192 (four): DESIGN.md §2.17.
//
// Packer (cc_w12_pack, once per tensor): exponent histogram -> the window of 16 that covers most weights -> codes and records.
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <unordered_map>

#include "cc_common.h"
#include "cc_gemv_core.h"

namespace {

constexpr int kW12Threads = kGvCoreThreads;
constexpr int kW12Waves = kGvCoreWaves;
constexpr uint32_t kW12Overflow = 0xFFFFFFFFu;
constexpr int kW12Slots = 7;

struct GemvW12Args {
  GemvArgs g;           // g.W / g.W3: the dense tensors (read only by waves whose record overflowed)
  const uint32_t* P;    // codes [N, K / 8, 3]
  const uint32_t* P3;
  const uint32_t* R;    // records [row groups, phases, 4 waves][8]
  const uint32_t* R3;
  uint32_t bw, bw3;     // layout 0: base << 7 | base << 23; planar: base / 2 in every byte
};

constexpr int kW12Planar = 1, kW12Long = 2;  // layout ids (kW12Long: planar codes, the long-row launch and its records)

typedef unsigned int u32x3_t __attribute__((ext_vector_type(3)));

__device__ __forceinline__ uint32_t w12_pair(uint32_t sm, uint32_t sel, uint32_t ex, int j, uint32_t bw) {
  const uint32_t t = (__builtin_amdgcn_perm(sm, sm, sel) & 0x807f807fu) | bw;
  return (((ex >> (4 * j)) & 0x000f000fu) << 7) + t;
}
template <int LAY>
__device__ __forceinline__ uint4 w12_decode(u32x3_t q, uint32_t bw) {
  if constexpr (LAY == kW12Planar) {
    const uint32_t ha = (q.z & 0x87878787u) + bw;
    const uint32_t hb = (__builtin_amdgcn_alignbit(q.z, q.z, 4) & 0x87878787u) + bw;  // rotate right by 4
    // (v_perm: selector bytes 0 .. 3 name the second source, 4 .. 7 the first)
    return make_uint4(__builtin_amdgcn_perm(ha, q.x, 0x05010400u), __builtin_amdgcn_perm(ha, q.x, 0x07030602u),
                      __builtin_amdgcn_perm(hb, q.y, 0x05010400u), __builtin_amdgcn_perm(hb, q.y, 0x07030602u));
  }
  return make_uint4(w12_pair(q.x, 0x01010000u, q.z, 0, bw), w12_pair(q.x, 0x03030202u, q.z, 1, bw),
                    w12_pair(q.y, 0x01010000u, q.z, 2, bw), w12_pair(q.y, 0x03030202u, q.z, 3, bw));
}

// the record of a tile lives in lanes 0 .. 7 of one register (word i in lane i); entries are read out with v_readlane
__device__ __forceinline__ uint4 w12_patch(uint4 d, uint32_t rec, int cnt, int t, int lane) {
  for (int e = 0; e < cnt; e++) {  // wave-uniform trip count (an overflowing record reads as -1: the tile was read again)
    const uint32_t en = __builtin_amdgcn_readlane(rec, 1 + e);
    if ((int)(en >> 25) == t) {
      const bool hit = lane == (int)((en >> 19) & 63u);
      const int k = (en >> 16) & 7;
      const uint32_t sh = (k & 1) * 16;
      const uint32_t keep = ~(0xffffu << sh), v = (en & 0xffffu) << sh;
      const int word = k >> 1;
      d.x = (hit && word == 0) ? (d.x & keep) | v : d.x;
      d.y = (hit && word == 1) ? (d.y & keep) | v : d.y;
      d.z = (hit && word == 2) ? (d.z & keep) | v : d.z;
      d.w = (hit && word == 3) ? (d.w & keep) | v : d.w;
    }
  }
  return d;
}

template <int LAY, bool SWIGLU, int RB, int CU, int XS>
__global__ __launch_bounds__(kW12Threads) void gemv_w12_kernel(GemvW12Args a) {
  const int N = a.g.N, nch = a.g.K / 8;
  const int nstep = ((nch + 63) / 64 + kW12Waves - 1) / kW12Waves;
  const int nph = (nstep + CU - 1) / CU;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint4* Wv = reinterpret_cast<const uint4*>(a.g.W);
  const uint4* W3v = reinterpret_cast<const uint4*>(a.g.W3);
  u32x3_t q[RB][CU], q3[RB][CU];
  uint32_t rec = 0, rec3 = 0;  // this tile's records: word i in lane i < 8
  int tr0 = 0, ts0 = 0;    // this tile's first row and column step
  auto issue = [&](int r0, int s0) {
    tr0 = r0;
    ts0 = s0;
    // The record is requested FIRST and every code load is unconditional, in the order gemv_body consumes the chunks: the waits
    // then count down load by load (record, chunk 0, chunk 1, ...) and the decode of a chunk runs under the loads behind it.  With
    // the record last, or with loads skipped under a branch, every chunk waits for the whole tile.  A chunk outside the matrix
    // reads the nearest chunk inside it (row and column clamped) and is decoded without the base: exponents <= 15, finite, and it
    // meets a zero of x (columns) or a row that is never stored, so the sums keep their bits.
    const size_t at = (((size_t)(r0 / RB) * nph + s0 / CU) * kW12Waves + wave) * 8 + (lane & 7);
    rec = a.R[at];
    if (SWIGLU) rec3 = a.R3[at];
#pragma unroll
    for (int u = 0; u < CU; u++) {
      const int c = ((s0 + u) * kW12Waves + wave) * 64 + lane;
      const int cc = c < nch ? c : nch - 1;
#pragma unroll
      for (int r = 0; r < RB; r++) {
        const int rr = r0 + r < N ? r0 + r : N - 1;
        const size_t off = ((size_t)rr * nch + cc) * 3;
        q[r][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x3_t*>(a.P + off));
        if (SWIGLU) q3[r][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x3_t*>(a.P3 + off));
      }
    }
  };
  auto chunk = [&](u32x3_t code, uint32_t bw, uint32_t rc, const uint4* dense, int r, int u) {
    const int c = ((ts0 + u) * kW12Waves + wave) * 64 + lane;
    const bool in = (ts0 + u < nstep) && c < nch && (tr0 + r < N);
    uint4 d = w12_decode<LAY>(code, in ? bw : 0u);  // (outside the matrix: no base, see issue; zero codes decode to zeros)
    const uint32_t cnt = __builtin_amdgcn_readlane(rc, 0);
    if (cnt != 0u) {  // wave-uniform
      if (cnt == kW12Overflow) {
        d = in ? nt_load(dense + (size_t)(tr0 + r) * nch + c) : make_uint4(0, 0, 0, 0);
      } else {
        d = w12_patch(d, rc, (int)cnt, r * CU + u, lane);
      }
    }
    return d;
  };
  auto get = [&](int r, int u) { return chunk(q[r][u], a.bw, rec, Wv, r, u); };
  auto get3 = [&](int r, int u) { return chunk(q3[r][u], a.bw3, rec3, W3v, r, u); };
  gemv_body<bf16_t, SWIGLU, RB, CU, XS>(a.g, issue, get, get3);
}

// ---- layout id 2, "long": planar codes behind a launch of their own for LONG rows, 3 .. 8 column steps per wave (4096 < K <= 16384),
//      plain form only.  gemv_long_body (cc_gemv_core.h) keeps two small tiles of codes in two register sets and requests the tile
//      after the current one — with its record ahead of its codes, as above — before it decodes the current one, also across the
//      end of a row group.  Column steps beyond nstep are not requested (wave-uniform); rows beyond N and the chunks of a partial
//      last segment keep the clamped unconditional form.  Records are the packer's, laid out for this tile shape.
//      NORM false: the launch has no norm prologue (w2), and the registers that prologue needs (x, delta and the norm weight of
//      every input chunk at once) do not count against the kernel.
template <int RB, int CU, int NSTEP, bool NORM>
__global__ __launch_bounds__(kW12Threads) void gemv_w12_long_kernel(GemvW12Args a) {
  if (!NORM) a.g.norm_w = nullptr;  // (it is: launch_w12_long)
  const int N = a.g.N, nch = a.g.K / 8;
  constexpr int nph = (NSTEP + CU - 1) / CU;
  // (the wave index as a scalar: row and record addresses are then scalar too, and a load takes a 32-bit lane offset beside them)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const char* Wb = reinterpret_cast<const char*>(a.g.W);
  const char* Pb = reinterpret_cast<const char*>(a.P);
  uint32_t coff[NSTEP];  // byte offset of this lane's codes in a row, per column step (clamped into the row)
#pragma unroll
  for (int s = 0; s < NSTEP; s++) {
    const int c = (s * kW12Waves + wave) * 64 + lane;
    coff[s] = (uint32_t)(c < nch ? c : nch - 1) * 12u;
  }
  u32x3_t q0[RB][CU], q1[RB][CU];
  uint32_t rec0 = 0, rec1 = 0;  // the two tiles' records: word i in lane i < 8
  auto request = [&](u32x3_t (&q)[RB][CU], uint32_t& rec, int r0, int s0) {
    rec = a.R[(((size_t)(r0 / RB) * nph + s0 / CU) * kW12Waves + wave) * 8 + (lane & 7)];
#pragma unroll
    for (int u = 0; u < CU; u++) {
      if (s0 + u < NSTEP) {
#pragma unroll
        for (int r = 0; r < RB; r++) {
          const int rr = r0 + r < N ? r0 + r : N - 1;
          const char* row = Pb + (size_t)rr * nch * 12;
          q[r][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x3_t*>(row + coff[s0 + u < NSTEP ? s0 + u : 0]));
        }
      }
    }
  };
  auto chunk = [&](u32x3_t code, uint32_t rc, int r, int u, int r0, int s0) {  // (called for column steps below NSTEP only)
    const int c = ((s0 + u) * kW12Waves + wave) * 64 + lane;
    const bool in = c < nch && (r0 + r < N);
    uint4 d = w12_decode<kW12Planar>(code, in ? a.bw : 0u);
    const uint32_t cnt = __builtin_amdgcn_readlane(rc, 0);
    if (cnt != 0u) {  // wave-uniform
      if (cnt == kW12Overflow) {
        d = in ? nt_load(reinterpret_cast<const uint4*>(Wb + (size_t)(r0 + r) * nch * 16 + (uint32_t)c * 16u)) : make_uint4(0, 0, 0, 0);
      } else {
        d = w12_patch(d, rc, (int)cnt, r * CU + u, lane);
      }
    }
    return d;
  };
  auto issue = [&](auto set, int r0, int s0) {
    if constexpr (decltype(set)::value == 0) request(q0, rec0, r0, s0);
    else request(q1, rec1, r0, s0);
  };
  auto get = [&](auto set, int r, int u, int r0, int s0) {
    if constexpr (decltype(set)::value == 0) return chunk(q0[r][u], rec0, r, u, r0, s0);
    else return chunk(q1[r][u], rec1, r, u, r0, s0);
  };
  gemv_long_body<bf16_t, RB, CU, NSTEP>(a.g, issue, get);
}

// ---- launch geometry.  The starting point is cc_gemv.hip's pick_cfg (the same loads in flight per lane, each a quarter shorter).
//      Both layouts take it: for planar, w2 at 2 x 4 on 512 / 1024 workgroups measured 27.1 / 27.6 us against 28.1 at 4 x 4 and 20.6
//      dense (with the record still requested last: DESIGN.md §2.17), and wo / wqkv already run the dense kernel's own geometry;
//      that instantiation is not built.
// the long-row launch: the tile and the most workgroups that the same-session sweeps chose: 2 x 2 everywhere;
// one resident round of workgroups where the kernel runs at 3 waves per SIMD (5 .. 8 column steps: w2 17.4 us on 768 workgroups
// against 18.7 / 19.1 / 17.9 / 18.1 / 18.4 / 18.6 on 512 / 1024 / 1280 / 1536 / 1792 / 2048), 1024 at 3 and 4 column steps
// (8192 x 8192: 19.4 us against 19.8 / 19.5 on 1280 / 2048; 128256 x 8192: 239.5 against 244.9 / 243.4)
constexpr int kW12LongRb = 2, kW12LongCu = 2;
static int w12_long_cap(int K) {
  const int nstep = ((K / 8 + 63) / 64 + kGvCoreWaves - 1) / kGvCoreWaves;
  return nstep <= 4 ? 1024 : 768;
}

static GvCfg pick_w12_cfg(int N, int K, bool swiglu, int layout) {
  static int env_rb = -1, env_cu = -1, env_cap = 2048;
  if (env_rb < 0) {  // tuning hook: CC_GEMV_W12_CFG="RB,CU[,max workgroups]"
    env_rb = env_cu = 0;
    if (const char* e = getenv("CC_GEMV_W12_CFG")) sscanf(e, "%d,%d,%d", &env_rb, &env_cu, &env_cap);
  }
  if (env_rb > 0 && env_cu > 0) return {env_rb, env_cu, env_cap};
  if (layout == kW12Long) return {kW12LongRb, kW12LongCu, w12_long_cap(K)};
  const int nseg = (K / 8 + 63) / 64, nstep = (nseg + kW12Waves - 1) / kW12Waves;
  GvCfg c;
  c.cap = 2048;
  if (nstep <= 2 && !swiglu) {
    if (N >= 32768) {
      c.rb = 2; c.cu = 2;
    } else {
      c.rb = 4; c.cu = 2;
    }
    c.cap = 1024;
  } else if (nstep <= 2) {
    c.rb = 2; c.cu = 2;
  } else if (swiglu) {
    c.rb = 2; c.cu = 4;
  } else {
    c.rb = 4; c.cu = 4;
    c.cap = 512;
  }
  return c;
}

// the long-row launch: the tile and the most workgroups that the same-session sweep chose
static int w12_xs(int K) {
  const int nseg = (K / 8 + 63) / 64, nstep = (nseg + kW12Waves - 1) / kW12Waves;
  return nstep <= 2 ? 2 : nstep <= 8 ? 8 : 0;  // (rows beyond 8 steps per wave, K > 16384, are not served: CC_ERR_UNSUPPORTED)
}

static bool w12_cfg_built(int layout, bool swiglu, int xs, int rb, int cu) {
  const int key = (swiglu ? 100000 : 0) + xs * 1000 + rb * 10 + cu;
  if (layout == kW12Long) return key == 8022;  // (4 x 2 and 2 x 4 lost the sweep and are not built)
  switch (key) {  // (the same list in layouts 0 and 1)
    case 2022: case 2042: case 8044: case 102022: case 108024: return layout == 0 || layout == kW12Planar;
    default: return false;
  }
}

// the planar launch classes switched on by default (cc_w12_geometry): the SwiGLU pair and the LM head at K <= 4096, <true, 2, 2, 2>
// and <false, 2, 2, 2> on 1024 workgroups — 33.2 us against 34.9 (layout 0) and 39.6 (dense), 123.7 against 134.9 and 156.3.
// wqkv, wo and w2 lost to the dense kernel in this layout too (1.03x, 1.12x, 1.23x); wqkv and wo stay dense, w2 and the plain K = 8192
// shapes are served by layout 2's launch (w12_long_won); K = 8192 is not switched on in this layout.
static bool w12_planar_won(int nstep, bool swiglu, int N) { return nstep <= 2 && (swiglu || N >= 32768); }

// the long-row classes switched on by default (cc_w12_geometry, layout 2), by the same rule as planar's: the two that were measured
// (profiles/w12_long_gemv.jsonl) — seven column steps per wave (w2, 4096 x 14336: 17.5 us against 20.2 dense and 26.0 planar) and
// four (K = 8192: 8192 x 8192 and 128256 x 8192).  3, 5, 6 and 8 steps are served and tested, not measured, and stay off.
static bool w12_long_won(int nstep) { return nstep == 7 || nstep == 4; }

template <int RB, int CU>
static int launch_w12_long(const GemvW12Args& a, hipStream_t st, int cap) {
  int blocks = (a.g.N + RB - 1) / RB;
  if (blocks > cap) blocks = cap;
  const int nstep = ((a.g.K / 8 + 63) / 64 + kW12Waves - 1) / kW12Waves;
#define W12_LONG(NS)                                                                                                   \
  if (a.g.norm_w) hipLaunchKernelGGL((gemv_w12_long_kernel<RB, CU, NS, true>), dim3(blocks), dim3(kW12Threads), 0, st, a); \
  else hipLaunchKernelGGL((gemv_w12_long_kernel<RB, CU, NS, false>), dim3(blocks), dim3(kW12Threads), 0, st, a)
  switch (nstep) {  // (one kernel per number of column steps: which tiles exist is then known to the compiler)
    case 3: W12_LONG(3); break;
    case 4: W12_LONG(4); break;
    case 5: W12_LONG(5); break;
    case 6: W12_LONG(6); break;
    case 7: W12_LONG(7); break;
    case 8: W12_LONG(8); break;
    default: return CC_ERR_UNSUPPORTED;
  }
#undef W12_LONG
  return CC_OK;
}

template <int LAY, bool SWIGLU, int RB, int CU, int XS>
static void launch_w12_cfg(const GemvW12Args& a, hipStream_t st, int cap) {
  int blocks = (a.g.N + RB - 1) / RB;
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL((gemv_w12_kernel<LAY, SWIGLU, RB, CU, XS>), dim3(blocks), dim3(kW12Threads), 0, st, a);
}

// the layout every packed copy was written in, by the address of its codes: cc_gemv_fused_w12 refuses a copy handed in under the
// other layout's id before it launches anything.  (Host memory only; an address packed again takes its new layout; codes that
// cc_w12_pack of this process did not write are not known here and pass.)
static std::mutex w12_reg_mu;
static std::unordered_map<const void*, int> w12_reg;

static void w12_register(const void* codes, int layout) {
  std::lock_guard<std::mutex> g(w12_reg_mu);
  w12_reg[codes] = layout;
}
static bool w12_layout_ok(const void* codes, int layout) {
  std::lock_guard<std::mutex> g(w12_reg_mu);
  const auto it = w12_reg.find(codes);
  return it == w12_reg.end() || it->second == layout;
}

// ---- packer
constexpr int kW12MetaBase = 0, kW12MetaRecords = 1, kW12MetaOverflow = 2, kW12MetaEscapes = 3, kW12MetaHist = 8;

__global__ __launch_bounds__(256) void w12_hist_kernel(const uint16_t* W, size_t n, int32_t* meta) {
  __shared__ int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) atomicAdd(&h[(W[i] >> 7) & 0xff], 1);
  __syncthreads();
  // (int32 bins: cc_w12_pack rejects tensors of 2^31 weights or more)
  if (h[threadIdx.x]) atomicAdd(&meta[kW12MetaHist + threadIdx.x], h[threadIdx.x]);
}

__global__ void w12_base_kernel(int32_t* meta, int nrec, int layout) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long best = -1;
  int base = 0;
  // base + 15 <= 255: the decode's index add never carries into the sign.  Planar: even bases only (its index is exponent >> 1)
  for (int b = 0; b + 15 <= 255; b += (layout != 0 ? 2 : 1)) {
    long long s = 0;
    for (int i = 0; i < 16; i++) s += meta[kW12MetaHist + b + i];
    if (s > best) {
      best = s;
      base = b;
    }
  }
  meta[kW12MetaBase] = base;
  meta[kW12MetaRecords] = nrec;
}

// one wave per record: the RB x CU chunks per lane that gemv_w12_kernel's wave requests together
__global__ __launch_bounds__(64) void w12_pack_kernel(const uint4* W, int N, int K, int RB, int CU, int layout, uint32_t* P, uint32_t* R,
                                                      int32_t* meta) {
  __shared__ uint32_t rec[8];
  const int lane = threadIdx.x;
  const int nch = K / 8;
  const int nstep = ((nch + 63) / 64 + kW12Waves - 1) / kW12Waves;
  const int nph = (nstep + CU - 1) / CU;
  const int wave = blockIdx.x % kW12Waves;
  const int ph = (blockIdx.x / kW12Waves) % nph;
  const int rg = blockIdx.x / (kW12Waves * nph);
  const int base = meta[kW12MetaBase];
  if (lane < 8) rec[lane] = 0;
  __syncthreads();
  int count = 0;
  for (int t = 0; t < RB * CU; t++) {
    const int r = t / CU, u = t % CU;
    const int row = rg * RB + r;
    const int c = ((ph * CU + u) * kW12Waves + wave) * 64 + lane;
    const bool in = row < N && (ph * CU + u) < nstep && c < nch;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (in) v = W[(size_t)row * nch + c];
    const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
    uint32_t sm[2] = {0, 0}, ex = 0;
    for (int k = 0; k < 8; k++) {
      const uint32_t bits = (wd[k >> 1] >> ((k & 1) * 16)) & 0xffffu;
      const int idx = (int)((bits >> 7) & 0xffu) - base;
      const bool esc = in && (idx < 0 || idx > 15);
      if (!esc && layout != 0) {  // planar codes (layouts 1 and 2)
        if (in) {  // (base is even here: idx >> 1 = (exponent >> 1) - base / 2)
          const uint32_t hi = (uint32_t)idx >> 1, sg = bits >> 15;
          const int j = k & 3;
          sm[k >> 2] |= (bits & 0xffu) << (j * 8);
          ex |= k < 4 ? ((sg << 7) | hi) << (j * 8) : (hi << (j * 8 + 4)) | (sg << (((j + 1) & 3) * 8 + 3));
        }
      } else if (!esc) {
        sm[k >> 2] |= (((bits >> 8) & 0x80u) | (bits & 0x7fu)) << ((k & 3) * 8);
        ex |= (uint32_t)(in ? idx : 0) << ((k & 1) * 16 + (k >> 1) * 4);
      }
      const unsigned long long m = __ballot(esc);
      if (esc) {
        const int slot = count + __popcll(m & ((1ull << lane) - 1ull));
        if (slot < kW12Slots) rec[1 + slot] = ((uint32_t)t << 25) | ((uint32_t)lane << 19) | ((uint32_t)k << 16) | bits;
      }
      count += __popcll(m);
    }
    if (in) {
      uint32_t* p = P + ((size_t)row * nch + c) * 3;
      p[0] = sm[0];
      p[1] = sm[1];
      p[2] = ex;
    }
  }
  __syncthreads();
  if (lane == 0) {
    rec[0] = count > kW12Slots ? kW12Overflow : (uint32_t)count;
    if (count > kW12Slots) atomicAdd(&meta[kW12MetaOverflow], 1);
    if (count) atomicAdd(&meta[kW12MetaEscapes], count);
  }
  __syncthreads();
  if (lane < 8) R[(size_t)blockIdx.x * 8 + lane] = (count > kW12Slots && lane > 0) ? 0u : rec[lane];
}

}  // namespace

// (the layout id travels in bits 8 .. 15 of a word whose low byte keeps its old meaning: 0 = the first layout, as before)
static inline int w12_layout_of(int32_t word) { return (word >> 8) & 0xff; }
static inline bool w12_layout_known(int layout) { return layout == 0 || layout == kW12Planar || layout == kW12Long; }
// layout 2 serves plain matrices with 3 .. 8 column steps per wave only (4096 < K <= 16384)
static inline bool w12_long_serves(int K) {
  const int nstep = ((K / 8 + 63) / 64 + kW12Waves - 1) / kW12Waves;
  return nstep >= 3 && nstep <= 8;
}

extern "C" int cc_w12_geometry(int32_t N, int32_t K, int32_t swiglu, int32_t* out) {
  const int layout = w12_layout_of(swiglu);
  const bool pair = (swiglu & 0xff) != 0;
  if (!out || N <= 0 || K <= 0 || (swiglu >> 16) != 0 || !w12_layout_known(layout)) return CC_ERR_BAD_ARG;
  if (K % 8 || (size_t)K * 2 > 64 * 1024) return CC_ERR_UNSUPPORTED;
  if (layout == kW12Long && (pair || !w12_long_serves(K))) return CC_ERR_UNSUPPORTED;
  const GvCfg c = pick_w12_cfg(N, K, pair, layout);
  const int xs = w12_xs(K);
  if (xs == 0 || c.cu > xs || c.cap <= 0 || !w12_cfg_built(layout, pair, xs, c.rb, c.cu)) return CC_ERR_UNSUPPORTED;
  out[0] = c.rb;
  out[1] = c.cu;
  out[2] = xs;
  out[3] = c.cap;
  const int nstep = ((K / 8 + 63) / 64 + kW12Waves - 1) / kW12Waves;
  if (layout == kW12Long) {  // the same rule and regime
    out[4] = ((long long)N >= (long long)c.rb * c.cap && w12_long_won(nstep)) ? 1 : 0;
    return CC_OK;
  }
  if (layout == kW12Planar) {
    // planar: the launch classes that MEASURED faster than both the dense kernel and the first layout, by more than the dense
    // kernel's own spread (profiles/w12_planar_gemv.jsonl), in the regime measured: a grid that is full
    const bool full = (long long)N >= (long long)c.rb * c.cap;
    out[4] = (full && w12_planar_won(nstep, pair, N)) ? 1 : 0;
    return CC_OK;
  }
  // the launch classes that MEASURED faster than the dense kernel (the SwiGLU pair and the LM head at K = 4096,
  // <true, 2, 2, 2> and <false, 2, 2, 2> with 1024 workgroups); every other class is served but stays dense by default
  out[4] = (nstep <= 2 && (pair || N >= 32768)) ? 1 : 0;
  return CC_OK;
}

extern "C" size_t cc_w12_meta_words(void) { return kW12MetaHist + 256; }

extern "C" int cc_w12_pack(const void* W, int32_t N, int32_t K, int32_t rb, int32_t cu, void* codes, void* records, void* meta,
                           cc_stream_t stream) {
  CC_ENTRY();
  const int layout = w12_layout_of(rb);
  if ((rb >> 16) != 0 || !w12_layout_known(layout)) return CC_ERR_BAD_ARG;
  rb &= 0xff;
  if (!W || !codes || !records || !meta || N <= 0 || K <= 0 || rb <= 0 || cu <= 0 || rb * cu > 64) return CC_ERR_BAD_ARG;
  if (K % 8 || (size_t)K * 2 > 64 * 1024) return CC_ERR_UNSUPPORTED;
  if (layout == kW12Long && !w12_long_serves(K)) return CC_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int nch = K / 8;
  const int nstep = ((nch + 63) / 64 + kW12Waves - 1) / kW12Waves;
  const int nph = (nstep + cu - 1) / cu;
  const long long nrec = (long long)((N + rb - 1) / rb) * nph * kW12Waves;
  if (nrec > 0x7fffffffLL || (long long)N * K >= 0x80000000LL) return CC_ERR_UNSUPPORTED;  // (the histogram counts in int32)
  int32_t* m = reinterpret_cast<int32_t*>(meta);
  if (hipMemsetAsync(m, 0, (kW12MetaHist + 256) * sizeof(int32_t), st) != hipSuccess) return CC_ERR_HIP;
  const size_t n = (size_t)N * K;
  int hb = (int)((n + 256 * 64 - 1) / (256 * 64));
  if (hb > 2048) hb = 2048;
  hipLaunchKernelGGL(w12_hist_kernel, dim3(hb), dim3(256), 0, st, reinterpret_cast<const uint16_t*>(W), n, m);
  hipLaunchKernelGGL(w12_base_kernel, dim3(1), dim3(64), 0, st, m, (int)nrec, layout);
  hipLaunchKernelGGL(w12_pack_kernel, dim3((unsigned)nrec), dim3(64), 0, st, reinterpret_cast<const uint4*>(W), N, K, rb, cu, layout,
                     reinterpret_cast<uint32_t*>(codes), reinterpret_cast<uint32_t*>(records), m);
  CC_LAUNCH_CHECK();
  w12_register(codes, layout);
  return CC_OK;
}

extern "C" int cc_gemv_fused_w12(const void* codes, const void* records, int32_t base, const void* codes3, const void* records3,
                                 int32_t base3, int32_t rb, int32_t cu, const void* W, const void* W3, const void* x, const void* delta,
                                 const void* norm_w, float eps, void* h_out, const void* bias, const void* freqs, int32_t rope_rows,
                                 int32_t head_dim, void* y, int32_t N, int32_t K, int32_t dtype, cc_stream_t stream) {
  CC_ENTRY();
  const int layout = w12_layout_of(rb);
  if ((rb >> 16) != 0 || !w12_layout_known(layout)) return CC_ERR_BAD_ARG;
  rb &= 0xff;
  if (!codes || !records || !W || !x || !y || N <= 0 || K <= 0 || !cc_dt_ok(dtype)) return CC_ERR_BAD_ARG;
  if ((W3 != nullptr) != (codes3 != nullptr) || (W3 != nullptr) != (records3 != nullptr)) return CC_ERR_BAD_ARG;
  if (base < 0 || base > 240 || (W3 && (base3 < 0 || base3 > 240))) return CC_ERR_BAD_ARG;
  if (layout != 0 && ((base & 1) || (W3 && (base3 & 1)))) return CC_ERR_BAD_ARG;
  if ((delta || h_out) && !norm_w) return CC_ERR_BAD_ARG;
  if (freqs && (W3 || rope_rows < 0 || rope_rows > N || head_dim <= 0 || (head_dim & 1) || (rope_rows % head_dim))) return CC_ERR_BAD_ARG;
  if (W3 && bias) return CC_ERR_BAD_ARG;
  if (dtype != CC_DT_BF16) return CC_ERR_UNSUPPORTED;
  int32_t geo[5];
  const int rc = cc_w12_geometry(N, K, (W3 != nullptr ? 1 : 0) | (layout << 8), geo);
  if (rc != CC_OK) return rc;
  // (behind the shape's verdict: the registry is keyed by address and never forgets, so a fresh buffer at the address of a freed copy
  //  of another layout would otherwise turn the CC_ERR_UNSUPPORTED of a shape this id does not serve into CC_ERR_BAD_ARG)
  if (!w12_layout_ok(codes, layout) || (codes3 && !w12_layout_ok(codes3, layout))) return CC_ERR_BAD_ARG;  // packed in the other layout
  if (geo[0] != rb || geo[1] != cu) return CC_ERR_BAD_ARG;  // the records were laid out for another launch geometry
  GemvW12Args a;
  a.g = GemvArgs{W, W3, x, delta, norm_w, bias, freqs, h_out, y, eps, N, K, freqs ? rope_rows : 0, freqs ? head_dim : 2};
  a.P = reinterpret_cast<const uint32_t*>(codes);
  a.P3 = reinterpret_cast<const uint32_t*>(codes3);
  a.R = reinterpret_cast<const uint32_t*>(records);
  a.R3 = reinterpret_cast<const uint32_t*>(records3);
  if (layout != 0) {
    a.bw = (uint32_t)(base >> 1) * 0x01010101u;
    a.bw3 = (uint32_t)(base3 >> 1) * 0x01010101u;
  } else {
    a.bw = ((uint32_t)base << 7) | ((uint32_t)base << 23);
    a.bw3 = ((uint32_t)base3 << 7) | ((uint32_t)base3 << 23);
  }
  hipStream_t st = (hipStream_t)stream;
  const int key = layout * 1000000 + (W3 ? 100000 : 0) + geo[2] * 1000 + rb * 10 + cu;
  switch (key) {  // (w12_cfg_built's list)
    case 2022: launch_w12_cfg<0, false, 2, 2, 2>(a, st, geo[3]); break;
    case 2042: launch_w12_cfg<0, false, 4, 2, 2>(a, st, geo[3]); break;
    case 8044: launch_w12_cfg<0, false, 4, 4, 8>(a, st, geo[3]); break;
    case 102022: launch_w12_cfg<0, true, 2, 2, 2>(a, st, geo[3]); break;
    case 108024: launch_w12_cfg<0, true, 2, 4, 8>(a, st, geo[3]); break;
    case 1002022: launch_w12_cfg<kW12Planar, false, 2, 2, 2>(a, st, geo[3]); break;
    case 1002042: launch_w12_cfg<kW12Planar, false, 4, 2, 2>(a, st, geo[3]); break;
    case 1008044: launch_w12_cfg<kW12Planar, false, 4, 4, 8>(a, st, geo[3]); break;
    case 1102022: launch_w12_cfg<kW12Planar, true, 2, 2, 2>(a, st, geo[3]); break;
    case 1108024: launch_w12_cfg<kW12Planar, true, 2, 4, 8>(a, st, geo[3]); break;
    case 2008022:
      if (launch_w12_long<2, 2>(a, st, geo[3]) != CC_OK) return CC_ERR_UNSUPPORTED;
      break;
    default: return CC_ERR_UNSUPPORTED;
  }
  CC_LAUNCH_CHECK();
  return CC_OK;
}
