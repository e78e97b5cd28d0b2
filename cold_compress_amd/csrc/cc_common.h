// cc_common.h — device helpers shared by the gfx950 kernels (wave64, CDNA4 only; no CUDA paths).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/coldcompress.h"
#include "../../include/coldcompress_debug.h"

#define CC_WAVE 64

// ------------------------------------------------------------------ element types
struct bf16_t {
  uint16_t x;
};
struct f16_t {
  uint16_t x;
};

__device__ __forceinline__ float bf16_bits_to_f32(uint32_t h) { return __uint_as_float(h << 16); }

// round-to-nearest-even via the gfx950 v_cvt_pk_bf16_f32 instruction (one op instead of ~7); identical to
// oracle/cc_oracle.c f32_to_bf16 for every non-NaN input (NaN stays a quiet NaN).
__device__ __forceinline__ uint16_t f32_to_bf16_bits(float f) {
  const __bf16 b = (__bf16)f;
  uint16_t h;
  __builtin_memcpy(&h, &b, 2);
  return h;
}

__device__ __forceinline__ float f16_bits_to_f32(uint16_t h) {
  _Float16 v;
  __builtin_memcpy(&v, &h, 2);
  return (float)v;
}
__device__ __forceinline__ uint16_t f32_to_f16_bits(float f) {
  _Float16 v = (_Float16)f;  // v_cvt_f16_f32: round-to-nearest-even
  uint16_t h;
  __builtin_memcpy(&h, &v, 2);
  return h;
}

// An fp32 value the optimiser must treat as opaque: keeps `T(fmaf(a, b, c))` a TWO-step rounding (fp32, then T).  Without it the
// f16 instantiations fuse the pair into v_fma_mixlo_f16 (ONE rounding of the exact result) wherever the pattern is visible, and
// two kernels computing the same formula disagree by an ulp in the rare double-rounding cases.
__device__ __forceinline__ float cc_opaque_f32(float x) {
  asm("" : "+v"(x));
  return x;
}

template <typename T>
struct ElemTraits;
template <>
struct ElemTraits<float> {
  static constexpr int code = CC_DT_F32;
  __device__ static __forceinline__ float load(const float* p, size_t i) { return p[i]; }
  __device__ static __forceinline__ void store(float* p, size_t i, float v) { p[i] = v; }
  __device__ static __forceinline__ float rnd(float v) { return v; }
};
template <>
struct ElemTraits<bf16_t> {
  static constexpr int code = CC_DT_BF16;
  __device__ static __forceinline__ float load(const bf16_t* p, size_t i) { return bf16_bits_to_f32(p[i].x); }
  __device__ static __forceinline__ void store(bf16_t* p, size_t i, float v) { p[i].x = f32_to_bf16_bits(v); }
  __device__ static __forceinline__ float rnd(float v) { return bf16_bits_to_f32(f32_to_bf16_bits(v)); }
};
// two roundings in one v_cvt_pk_bf16_f32 (the conversion is a packed instruction: rounding values one at a time wastes
// half of it); `packed` = lo | hi << 16 is what a 16-bit MFMA operand wants, the floats are its two halves
__device__ __forceinline__ uint32_t bf16_round_pair(float a, float b, float& ra, float& rb) {
  typedef float cc_f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 cc_bf16x2 __attribute__((ext_vector_type(2)));
  const cc_f32x2 v = {a, b};
  const cc_bf16x2 r = __builtin_convertvector(v, cc_bf16x2);
  const uint32_t packed = __builtin_bit_cast(uint32_t, r);
  ra = __uint_as_float(packed << 16);
  rb = __uint_as_float(packed & 0xffff0000u);
  return packed;
}

template <>
struct ElemTraits<f16_t> {
  static constexpr int code = CC_DT_F16;
  __device__ static __forceinline__ float load(const f16_t* p, size_t i) { return f16_bits_to_f32(p[i].x); }
  __device__ static __forceinline__ void store(f16_t* p, size_t i, float v) { p[i].x = f32_to_f16_bits(v); }
  __device__ static __forceinline__ float rnd(float v) { return f16_bits_to_f32(f32_to_f16_bits(v)); }
};

// ------------------------------------------------------------------ FP8 (OCP e4m3fn) fused cache (CC_QUANT_FP8_E4M3)
// One power-of-two scale 2^e per (head, slot) row: e = the smallest exponent with amax <= 448 * 2^e (amax = m * 2^k, m in [0.5, 1):
// 448 = 0.875 * 2^9), clamped to [-120, 120]; 0 for an all-zero row.  No division, no saturation: the scaled values never exceed 448.
__device__ __forceinline__ int cc_fp8_row_exp(float amax) {
  if (!(amax > 0.f)) return 0;
  int k;
  const float m = frexpf(amax, &k);
  const int e = m <= 0.875f ? k - 9 : k - 8;
  return e < -120 ? -120 : (e > 120 ? 120 : e);
}
// |x| for the row maximum: non-finite values do not count
__device__ __forceinline__ float cc_fp8_abs_finite(float x) { return __builtin_isfinite(x) ? __builtin_fabsf(x) : 0.f; }
// e4m3 codes of four values already scaled by 2^-e (v_cvt_pk_fp8_f32: OCP e4m3fn, round to nearest even), byte j = value j; a
// non-finite value encodes to the e4m3 NaN with its sign (0x7f | sign — the instruction's own NaN does not keep the sign)
__device__ __forceinline__ uint32_t cc_fp8_pack4(float a, float b, float c, float d) {
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  uint32_t r = (uint32_t)w;
  const float x[4] = {a, b, c, d};
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (!__builtin_isfinite(x[j])) r = (r & ~(0xffu << (8 * j))) | ((0x7fu | (__builtin_signbit(x[j]) ? 0x80u : 0u)) << (8 * j));
  return r;
}
// two e4m3 codes (bytes 2 hi, 2 hi + 1 of w) -> two 16-bit values of T, times 2^e (scale = 2^e exactly): v_cvt_scalef32_pk_{bf16,f16}_fp8.
// One rounding of the exact product (bf16: exact; f16: inf past 65504, subnormals rounded to nearest even)
template <typename T>
__device__ __forceinline__ uint32_t cc_fp8_dequant2(uint32_t w, float scale, bool hi) {
  static_assert(ElemTraits<T>::code == CC_DT_BF16 || ElemTraits<T>::code == CC_DT_F16, "FP8 images decode to a 16-bit dtype");
  if constexpr (ElemTraits<T>::code == CC_DT_BF16) {
    typedef __bf16 cc_bf16x2 __attribute__((ext_vector_type(2)));
    const cc_bf16x2 r = hi ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, scale, true) : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, scale, false);
    return __builtin_bit_cast(uint32_t, r);
  } else {
    typedef _Float16 cc_f16x2 __attribute__((ext_vector_type(2)));
    const cc_f16x2 r = hi ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, scale, true) : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, scale, false);
    return __builtin_bit_cast(uint32_t, r);
  }
}

// ------------------------------------------------------------------ MXFP4 (OCP e2m1, one e8m0 scale per 32 values) fused cache (CC_QUANT_MXFP4)
// One power-of-two scale 2^e per block of 32 values: e = the smallest exponent with amax <= 6 * 2^e (amax = m * 2^k, m in [0.5, 1):
// 6 = 0.75 * 2^3), clamped to [-120, 120]; -120 for an all-zero block.  No division; nothing finite saturates inside the clamp.
__device__ __forceinline__ int cc_mx4_block_exp(float amax) {
  if (!(amax > 0.f)) return -120;
  int k;
  const float m = frexpf(amax, &k);
  const int e = m <= 0.75f ? k - 3 : k - 2;
  return e < -120 ? -120 : (e > 120 ? 120 : e);
}
// the block's e8m0 scale byte: e + 127, or 0xff (e8m0's NaN) when the block holds a non-finite value
__device__ __forceinline__ uint32_t cc_mx4_scale_byte(int e, bool nonfinite) { return nonfinite ? 0xffu : (uint32_t)(e + 127); }
// e2m1 code (sign | magnitude on {0, 0.5, 1, 1.5, 2, 3, 4, 6}) of x * inv (inv = 2^-e: exact), round to nearest, ties to the even
// mantissa (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); past 6 (the clamp's end, +-inf): 6; NaN: 0
// under its sign; -0 keeps its sign.  Spelled on the VALU: it runs once per inserted row.
__device__ __forceinline__ uint32_t cc_mx4_code(float x, float inv) {
  const float y = __builtin_fabsf(__fmul_rn(x, inv));
  const uint32_t m = (uint32_t)(y > 0.25f) + (uint32_t)(y >= 0.75f) + (uint32_t)(y > 1.25f) + (uint32_t)(y >= 1.75f) +
                     (uint32_t)(y > 2.5f) + (uint32_t)(y >= 3.5f) + (uint32_t)(y > 5.f);
  return m | ((__float_as_uint(x) >> 28) & 8u);
}
// the scale operand of the decode: byte b of the row's word as a float's exponent field (2^(byte - 127); 0xff: +inf)
__device__ __forceinline__ float cc_mx4_scale(uint32_t word, int block) { return __uint_as_float(((word >> (8 * block)) & 0xffu) << 23); }
// two e2m1 codes (byte SEL of w: low nibble = the first value) -> two 16-bit values of T, times the scale operand's power of two:
// v_cvt_scalef32_pk_{bf16,f16}_fp4.  One rounding of the exact product (bf16: exact for every scale byte 7 .. 247)
template <typename T, int SEL>
__device__ __forceinline__ uint32_t cc_mx4_dequant2(uint32_t w, float scale) {
  static_assert(ElemTraits<T>::code == CC_DT_BF16 || ElemTraits<T>::code == CC_DT_F16, "MXFP4 images decode to a 16-bit dtype");
  if constexpr (ElemTraits<T>::code == CC_DT_BF16) {
    typedef __bf16 cc_bf16x2 __attribute__((ext_vector_type(2)));
    const cc_bf16x2 r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, SEL);
    return __builtin_bit_cast(uint32_t, r);
  } else {
    typedef _Float16 cc_f16x2 __attribute__((ext_vector_type(2)));
    const cc_f16x2 r = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, scale, SEL);
    return __builtin_bit_cast(uint32_t, r);
  }
}

// 16-byte vector of T, unpacked to floats
template <typename T>
struct Vec16 {
  static constexpr int N = 16 / sizeof(T);
  uint4 raw;
  __device__ __forceinline__ void load(const T* p) { raw = *reinterpret_cast<const uint4*>(p); }
  // streamed-once data (K/V rows of a decode step, weights): non-temporal, do not displace what L2 / MALL hold
  __device__ __forceinline__ void load_nt(const T* p) {
    typedef unsigned int u32x4_nt __attribute__((ext_vector_type(4)));
    const u32x4_nt v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_nt*>(p));
    raw = make_uint4(v.x, v.y, v.z, v.w);
  }
  __device__ __forceinline__ void unpack(float* out) const;
};
template <>
__device__ __forceinline__ void Vec16<float>::unpack(float* o) const {
  o[0] = __uint_as_float(raw.x);
  o[1] = __uint_as_float(raw.y);
  o[2] = __uint_as_float(raw.z);
  o[3] = __uint_as_float(raw.w);
}
template <>
__device__ __forceinline__ void Vec16<bf16_t>::unpack(float* o) const {
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    o[2 * i] = __uint_as_float(w[i] << 16);
    o[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
template <>
__device__ __forceinline__ void Vec16<f16_t>::unpack(float* o) const {
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    o[2 * i] = f16_bits_to_f32((uint16_t)(w[i] & 0xffffu));
    o[2 * i + 1] = f16_bits_to_f32((uint16_t)(w[i] >> 16));
  }
}

// ------------------------------------------------------------------ torch.argmin ordering as a 64-bit key
// key = (orderable(value) << 32) | slot ; min over keys == first index of the minimum.
// NaN maps to 0 (torch.argmin returns the first NaN); -0.0 is canonicalised to +0.0 (they compare equal).
__device__ __forceinline__ uint32_t orderable_f32(float f) {
  if (f != f) return 0u;
  if (f == 0.0f) f = 0.0f;
  uint32_t u = __float_as_uint(f);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return u == 0u ? 1u : u;  // keep 0 reserved for NaN (only ~0x ffffffff = -NaN pattern could hit it)
}
__device__ __forceinline__ uint32_t orderable_i32(int32_t v) { return (uint32_t)v ^ 0x80000000u; }

__device__ __forceinline__ unsigned long long make_key(uint32_t ord, uint32_t slot) {
  return ((unsigned long long)ord << 32) | slot;
}

// Uniform draw of KVCacheRandom's in-kernel generator (include/coldcompress.h, cc_decode_step_random_rng): stateless, 24 bits.
__host__ __device__ static inline uint64_t cc_mix64(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}
__host__ __device__ static inline float cc_rng_uniform(uint64_t seed, int32_t pos, int32_t slot) {
  const uint64_t x = cc_mix64(cc_mix64(seed + (uint64_t)(uint32_t)pos * 0x9E3779B97F4A7C15ull + (uint64_t)(uint32_t)slot));
  return (float)(uint32_t)(x >> 40) * 5.9604644775390625e-08f;  // * 2^-24: exact
}

// Fused heavy-hitter decode step: the arg-min key of the next eviction is published as one partial minimum
// per 128-slot chunk of the cache (no atomics: same-address atomics from 8 XCDs serialise in the fabric and
// cost more than the whole pass); consumers take the minimum over a head's cc_next_key_slots(S) entries.
// A head's key row holds kNextKeyPerChunk entries per 128-slot chunk: the two-launch combine pass fills the first n_chunks (one
// key per block) and keeps the others at ~0; the single-launch step publishes one key per WAVE of its 64-slot workgroups
// (2 workgroups x 4 waves per chunk), so that its waves never wait for each other at the end of the launch.
constexpr int kNextKeyChunk = 128;
constexpr int kNextKeyPerChunk = 8;
// r6: behind the live entries every row carries kNextKeyTail more that no arg-min ever reads: reserved, unread.
constexpr int kNextKeyTail = 8;
static inline int cc_next_key_live(int S) { return kNextKeyPerChunk * ((S + kNextKeyChunk - 1) / kNextKeyChunk); }
static inline int cc_next_key_slots(int S) { return cc_next_key_live(S) + kNextKeyTail; }  // the row stride

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    unsigned long long o = __shfl_xor(v, off, CC_WAVE);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, CC_WAVE));
  return v;
}

// Block-wide min of 64-bit keys; result valid in every thread.  `sm` needs blockDim.x/64 + 1 slots.
__device__ __forceinline__ unsigned long long block_min_u64(unsigned long long v, unsigned long long* sm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  v = wave_min_u64(v);
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  if (wave == 0) {
    unsigned long long x = lane < nw ? sm[lane] : ~0ull;
    x = wave_min_u64(x);
    if (lane == 0) sm[nw] = x;
  }
  __syncthreads();
  return sm[nw];
}

// Correctly rounded fp32 square root (what torch.linalg.vector_norm's sqrt is on any IEEE backend): through fp64 —
// 53 >= 2 * 24 + 2 bits make the double rounding exact.  (__fsqrt_rn compiled to a 1-ulp v_sqrt_f32 here: fp32 key
// norms differed from the oracle in the last bit.)
__device__ __forceinline__ float cc_sqrt_rn(float x) { return (float)__dsqrt_rn((double)x); }

// Canonical sum of squares of a D-vector, evaluated by 16 cooperating lanes (lane16 = 0..15 of an aligned
// 16-lane group): a_j = sum_i x[j+16i]^2 (sequential in i; separate multiply and add, no fma), then the
// butterfly a_j += a_{j^8}, ^4, ^2, ^1.  oracle/cc_oracle.c sumsq_canonical() evaluates the same order,
// so row norms are bit-identical between device and oracle (the reference's own order is unspecified).
template <typename T>
__device__ __forceinline__ float sumsq_canonical_16(const T* x, int D, int lane16) {
  float a = 0.f;
  for (int d = lane16; d < D; d += 16) {
    float e = ElemTraits<T>::load(x, d);
    float sq = __fmul_rn(e, e);
    a = __fadd_rn(a, sq);
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) a = __fadd_rn(a, __shfl_xor(a, off, 16));
  return a;
}

// hipGetLastError() is per-thread state shared with every other HIP user in the process (PyTorch leaves
// benign codes such as hipErrorNotReady behind): CC_ENTRY() clears it on entry, CC_LAUNCH_CHECK() reads ours.
#define CC_ENTRY() (void)hipGetLastError()
#define CC_LAUNCH_CHECK()                               \
  do {                                                  \
    if (hipGetLastError() != hipSuccess) return CC_ERR_HIP; \
  } while (0)

static inline int cc_dt_ok(int dt) { return dt == CC_DT_F32 || dt == CC_DT_BF16 || dt == CC_DT_F16; }
static inline size_t cc_dt_size(int dt) { return dt == CC_DT_F32 ? 4 : 2; }
static inline int cc_view_ok(const cc_kv_view* c) {
  return c && c->k_cache && c->v_cache && c->pos && c->mask && c->cache_cts && c->H > 0 && c->S > 0 && c->D > 0 &&
         (c->Hp == 1 || c->Hp == c->H) && (c->Hc == 1 || c->Hc == c->H) && cc_dt_ok(c->dtype) &&
         ((size_t)c->D * cc_dt_size(c->dtype)) % 4 == 0;
}
