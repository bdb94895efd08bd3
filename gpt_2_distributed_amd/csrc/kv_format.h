// The key/value cache formats of the decode path: what a lane holds of a 64-wide cache row and how it is loaded, formed,
// stored and expanded, once per format (KvBf16, KvFp8). decode.hip's store and attention kernels and beam.hip's reorder
// kernel are written once over these types. All of it sits in an unnamed namespace: each unit has its own copy.
#ifndef GPT2MI_KV_FORMAT_H
#define GPT2MI_KV_FORMAT_H
#include "common.h"

namespace {

__device__ __forceinline__ void unpack8(bf16x8 v, float* f) {
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = bf2f(v[j]);
}

// ---------------------------------------------------------------------------------------------------------------
// The fp8 cache format (gpt2mi.h v23; generation.py kv_quantize / kv_dequantize are the rule, executable): a 64-wide
// row of K or V is 64 OCP e4m3 codes and one fp32 scale 2^e, e the smallest exponent with amax <= 448 * 2^e and
// >= -100. Scaling by a power of two is exact and |x * 2^-e| <= 448, so the conversion never saturates: the codes are
// a pure function of the row's 64 bf16 values. This pair is the one quantiser and the one dequantiser of the library:
// KvFp8 below calls it for every kernel that forms or expands a row (decode.hip's kv_store_kernel and attn_row), so the
// two writers of a cache position cannot disagree.
struct KvRow8 {
  uint2 codes;  // this lane's 8 codes, dim 8 dg + j in byte j
  float scale;  // 2^e of the whole row
};

// f: the lane's 8 values of a row held by 8 adjacent lanes (lane ^ 1, 2, 4 hold the rest of it).
__device__ __forceinline__ KvRow8 kv_quantize8(const float* f) {
  float amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
  amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
  amax = fmaxf(amax, __shfl_xor(amax, 4, 64));
  // amax = m 2^k, m in [1, 2): e = k - 8 + (m > 1.75). A zero or subnormal amax has exponent field 0 and clamps.
  const unsigned u = __float_as_uint(amax);
  const int e = max((int)(u >> 23) - 135 + ((u & 0x7FFFFFu) > 0x600000u ? 1 : 0), -100);
  const float inv = __uint_as_float((unsigned)(127 - e) << 23);  // e in [-100, 121]: both are normal numbers
  KvRow8 r;
  r.scale = __uint_as_float((unsigned)(127 + e) << 23);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0] * inv, f[1] * inv, lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2] * inv, f[3] * inv, lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4] * inv, f[5] * inv, hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6] * inv, f[7] * inv, hi, true);
  r.codes = uint2{(unsigned)lo, (unsigned)hi};
  return r;
}

// The 8 codes as fp32, without the scale (exact: every e4m3 value is an fp32 value).
__device__ __forceinline__ void kv_codes8(uint2 c, float* f) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.x, true);
  const f32x2 d = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, false), g = __builtin_amdgcn_cvt_pk_f32_fp8((int)c.y, true);
  f[0] = a[0], f[1] = a[1], f[2] = b[0], f[3] = b[1], f[4] = d[0], f[5] = d[1], f[6] = g[0], f[7] = g[1];
}

// code * 2^e: exact.
__device__ __forceinline__ void kv_dequantize8(const KvRow8& r, float* f) {
  kv_codes8(r.codes, f);
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] *= r.scale;
}

// ---------------------------------------------------------------------------------------------------------------
// A cache tensor, the keys or the values of a layer as [stream][Tcap] rows of 64, in one of the two formats. Each type
// says what lane dg of the 8 lanes of a row holds of it (dims 8 dg .. 8 dg + 7) and is the only code that knows how
// such a row is zeroed, loaded from (stream, key), formed from the same dims of a qkv row, stored and expanded to fp32.
// A row is stored in two steps: every lane `store`s its dims, and the dg == 0 lane alone calls `store_once` for what
// the row holds once (the fp8 scale; nothing in bf16). The caller owns that branch so that a key and its value share
// it: with a branch inside each store the compiler lays the stores of the second row out twice.
// The kernels that touch a cache (decode.hip's store and attention kernels, beam.hip's reorder) are written once over
// KV = KvBf16 or KvFp8; a kernel takes the keys and the values as two of them, by value.

// Lane dg's place in a stream, formed once per thread: its 8 dims of row `key` are elements at + 64 key .. + 7 of the
// tensor, the row's scale (fp8) is element row0 + key of the scales.
struct KvLane {
  size_t at, row0;
  __device__ __forceinline__ KvLane(size_t stream, int Tcap, int dg) : at(stream * Tcap * 64 + 8 * dg), row0(stream * Tcap) {}
};

struct KvBf16 {
  using Row = bf16x8;
  bf16* rows;  // [stream][Tcap][64]

  static __device__ __forceinline__ Row zero() { return Row{0, 0, 0, 0, 0, 0, 0, 0}; }
  static __device__ __forceinline__ Row from_qkv(bf16x8 x) { return x; }
  __device__ __forceinline__ Row load(const KvLane& w, int key) const {
    return *reinterpret_cast<const Row*>(rows + w.at + (size_t)key * 64);
  }
  __device__ __forceinline__ void store(const KvLane& w, int key, const Row& r) const {
    *reinterpret_cast<Row*>(rows + w.at + (size_t)key * 64) = r;
  }
  __device__ __forceinline__ void store_once(const KvLane&, int, const Row&) const {}
  // A key as 8 floats and the factor its score takes after the 8-lane sum; a value as 8 floats.
  static __device__ __forceinline__ void key8(const Row& r, float* f) { unpack8(r, f); }
  static __device__ __forceinline__ float score_scale(const Row&) { return 1.f; }
  static __device__ __forceinline__ void value8(const Row& r, float* f) { unpack8(r, f); }
  // The same tensor seen from `n` rows further on (a layer of a [L][stream][Tcap] tensor).
  __device__ __forceinline__ KvBf16 shifted(size_t n) const { return KvBf16{rows + n * 64}; }
};

// A key or value is held as (8 codes, scale) whichever source it has: loaded that way, or quantised in registers by
// kv_quantize8 (whose shuffles stay inside the 8 lanes of the row, which take a branch together), and stored as those
// codes and that scale. Both are dequantised at the one place that uses them. A key's scale is
// applied to its score after the sum (a power of two: the same bits as scaling the 64 products, short of underflow,
// where a score is 0 either way); a value is code * scale before use, exactly.
struct KvFp8 {
  using Row = KvRow8;
  uint8_t* codes;  // [stream][Tcap][64]
  float* scales;   // [stream][Tcap]

  static __device__ __forceinline__ Row zero() { return Row{uint2{0u, 0u}, 0.f}; }
  static __device__ __forceinline__ Row from_qkv(bf16x8 x) {
    float f[8];
    unpack8(x, f);
    return kv_quantize8(f);
  }
  __device__ __forceinline__ Row load(const KvLane& w, int key) const {
    return Row{*reinterpret_cast<const uint2*>(codes + w.at + (size_t)key * 64), scales[w.row0 + key]};
  }
  __device__ __forceinline__ void store(const KvLane& w, int key, const Row& r) const {
    *reinterpret_cast<uint2*>(codes + w.at + (size_t)key * 64) = r.codes;
  }
  __device__ __forceinline__ void store_once(const KvLane& w, int key, const Row& r) const {
    scales[w.row0 + key] = r.scale;
  }
  static __device__ __forceinline__ void key8(const Row& r, float* f) { kv_codes8(r.codes, f); }
  static __device__ __forceinline__ float score_scale(const Row& r) { return r.scale; }
  static __device__ __forceinline__ void value8(const Row& r, float* f) { kv_dequantize8(r, f); }
  __device__ __forceinline__ KvFp8 shifted(size_t n) const { return KvFp8{codes + n * 64, scales + n}; }
};

}  // namespace
#endif  // GPT2MI_KV_FORMAT_H
