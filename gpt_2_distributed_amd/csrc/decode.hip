// Autoregressive decode: one new token per sequence and step, against a per-layer key/value cache. gfx950, wave64.
//
// The training kernels cannot serve this step: gpt2mi_gemm tiles 256x256 and needs M % 64 == 0 (3 workgroups at
// M = batch, N = 768), gpt2mi_attn_fwd recomputes every query row of a 64-multiple T. At M <= 64 rows the cost of a
// Linear is streaming its weight once, and of the attention streaming the cached K and V once: both kernels here load
// the streamed operand straight to VGPRs in full 128-byte lines (no LDS round trip: nothing is shared between waves),
// and split the reduction (K, or the keys) over enough waves to cover the chip. No atomics: partial results are
// combined in a fixed order, so every output is bitwise reproducible.
// The attention of the step and of the multi-row extend are two __global__ entries over one body (attn_row). Their
// gfx950 disassemblies (the Makefile's flags, -S) were compared with those of the two separate kernels they replace:
// same registers, no scratch, occupancy 8; what differs is listed in DESIGN.md "Multi-token decode step".
// The cache is bf16 or, since v23, fp8 (e4m3 codes and a power-of-two scale per 64-wide row). What differs between the
// two is in one type per format (KvBf16, KvFp8: what a lane holds of a row and how it is loaded, formed, stored and
// expanded; kv_format.h); the store kernel, the attention bodies and their kernels are written once over that type.
// Since v24 rows that hold the same prompt can share its keys and values: attn_row's arithmetic is attn_range, which a
// second kind of wave (attn_shared) runs for several rows over one load; same bits (DESIGN.md "Shared prompt cache").
#include <limits.h>

#include <algorithm>

#include "common.h"
#include "gpt2mi.h"
#include "kv_format.h"

namespace {

enum { SK_BF16 = 0, SK_F32 = 1, SK_RESID = 2, SK_GELU = 3 };

// ---------------------------------------------------------------------------------------------------------------
// Skinny GEMM. One wave owns a strip of 16 weight rows (output columns) over a range of 64-wide K chunks; the MFMA is
// v_mfma_f32_16x16x32_bf16 with the weight strip as its 16-row operand and up to 4 tiles of 16 activation rows as its
// 16-column operand. Within a chunk lane (r = lane % 16, g = lane / 16) holds k = 16 g .. 16 g + 15 of row r as two
// 16-byte loads (the four lanes of a row read one 128-byte line); the first halves feed one MFMA and the second
// halves the next. Both operands use the same k assignment, so the product is the plain dot product.
// A block's waves take consecutive chunk ranges of the block's K slice and are summed in wave order through LDS; the
// blocks of one strip (gridDim.y K slices) write fp32 partials that skinny_reduce_kernel sums in slice order.
// acc[mt][j] = C[m = 16 mt + lane % 16][n = n0 + 4 (lane / 16) + j].
constexpr int SK_MAX_WAVES = 4;

__device__ __forceinline__ float gelu_tanh1(float u) {
  // NewGELU in the sigmoid form of gemm_epilogue.h gelu4: u / (1 + 2^(u (A + B u^2)))
  const float k0 = 0.7978845608028654f, k1 = 0.044715f, m2log2e = -2.0f * 1.4426950408889634f;
  const float arg = u * __builtin_fmaf(u * u, k0 * k1 * m2log2e, k0 * m2log2e);
  return u * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(arg) + 1.f);
}

template <int EPI>
__device__ __forceinline__ void skinny_epilogue(f32x4 v, void* __restrict__ C, size_t off,
                                                const float* __restrict__ bias, const float* __restrict__ resid,
                                                int n) {
  if (bias) v += *reinterpret_cast<const f32x4*>(bias + n);
  if constexpr (EPI == SK_BF16) {
    *reinterpret_cast<bf16x4*>((bf16*)C + off) = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
  } else if constexpr (EPI == SK_F32) {
    *reinterpret_cast<f32x4*>((float*)C + off) = v;
  } else if constexpr (EPI == SK_RESID) {
    *reinterpret_cast<f32x4*>((float*)C + off) = *reinterpret_cast<const f32x4*>(resid + off) + v;
  } else {
    *reinterpret_cast<bf16x4*>((bf16*)C + off) =
        bf16x4{f2bf(gelu_tanh1(v[0])), f2bf(gelu_tanh1(v[1])), f2bf(gelu_tanh1(v[2])), f2bf(gelu_tanh1(v[3]))};
  }
}

template <int MT, int EPI>
__global__ __launch_bounds__(64 * SK_MAX_WAVES) void skinny_gemm_kernel(
    const bf16* __restrict__ A, int lda, const bf16* __restrict__ W, int ldw, void* __restrict__ C, int ldc,
    const float* __restrict__ bias, const float* __restrict__ resid, float* __restrict__ partial, int M, int N,
    int chunks, int cpu) {
  __shared__ f32x4 red[SK_MAX_WAVES - 1][MT][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int unit = blockIdx.y * nw + wave;
  const int c0 = unit * cpu;
  const int c1 = min(c0 + cpu, chunks);

  const bf16* wp = W + (size_t)(n0 + r) * ldw + 16 * g;
  const bf16* ap[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) ap[mt] = A + (size_t)min(16 * mt + r, M - 1) * lda + 16 * g;  // rows >= M: not stored

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c = c0; c < c1; ++c) {
    const bf16x8 w0 = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wp + 64 * c));
    const bf16x8 w1 = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wp + 64 * c + 8));
    bf16x8 a0[MT], a1[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      a0[mt] = *reinterpret_cast<const bf16x8*>(ap[mt] + 64 * c);
      a1[mt] = *reinterpret_cast<const bf16x8*>(ap[mt] + 64 * c + 8);
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, a0[mt], acc[mt], 0, 0, 0);
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, a1[mt], acc[mt], 0, 0, 0);
    }
  }

  // waves 1.. hand their sums to wave 0, which adds them in wave order
  if (nw > 1) {
    if (wave > 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) red[wave - 1][mt][lane] = acc[mt];
    }
    __syncthreads();
    if (wave > 0) return;
    for (int w = 0; w < nw - 1; ++w)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] += red[w][mt][lane];
  }

  const int n = n0 + 4 * g;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = 16 * mt + r;
    if (m >= M) continue;
    if (partial)  // one of gridDim.y K slices: [slice][M][N] fp32
      *reinterpret_cast<f32x4*>(partial + ((size_t)blockIdx.y * M + m) * N + n) = acc[mt];
    else
      skinny_epilogue<EPI>(acc[mt], C, (size_t)m * ldc + n, bias, resid, n);
  }
}

template <int EPI>
__global__ __launch_bounds__(256) void skinny_reduce_kernel(const float* __restrict__ partial, int slices,
                                                            void* __restrict__ C, int ldc,
                                                            const float* __restrict__ bias,
                                                            const float* __restrict__ resid, int M, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // one thread per 4 columns
  const int n4 = N / 4;
  if (i >= M * n4) return;
  const int m = i / n4, n = 4 * (i % n4);
  f32x4 v = *reinterpret_cast<const f32x4*>(partial + (size_t)m * N + n);
  for (int s = 1; s < slices; ++s) v += *reinterpret_cast<const f32x4*>(partial + ((size_t)s * M + m) * N + n);
  skinny_epilogue<EPI>(v, C, (size_t)m * ldc + n, bias, resid, n);
}

// The K split of a shape, from (N, K) only (an output row's bits must not depend on M): `slices` blocks per strip until
// the grid reaches the CU count, `nw` waves per block, `cpu` chunks per wave. From 128 strips on (N >= 2048: qkv, fc1,
// the lm_head) the strips' own blocks of 4 waves are kept: a second K slice would add the reduction launch, which
// costs more than the idle CUs of a launch that streams a few megabytes.
struct SkinnySplit {
  int chunks, slices, nw, cpu;
};
SkinnySplit skinny_split(int N, int K) {
  SkinnySplit s;
  const int strips = N / 16;
  s.chunks = K / 64;
  s.slices = strips >= 128 ? 1 : std::max(1, std::min(s.chunks, (256 + strips - 1) / strips));
  s.nw = std::max(1, std::min(SK_MAX_WAVES, s.chunks / s.slices));
  const int units = s.slices * s.nw;
  s.cpu = (s.chunks + units - 1) / units;
  return s;
}

// (unpack8, the fp8 quantiser pair and the cache types KvLane / KvBf16 / KvFp8: kv_format.h)

// Cache fill of the prefill: one thread per 8 values of the K and V columns of the n valid rows of each sequence. The 8
// threads of a (b, t, K or V, h) row are 8 adjacent lanes (a row is 8 consecutive values of i and blocks start at
// multiples of 8), as from_qkv needs. Threads beyond the last row form row 0's values with them and store nothing.
template <class KV>
__global__ __launch_bounds__(256) void kv_store_kernel(const bf16* __restrict__ qkv, KV kc, KV vc, int B, int T_src,
                                                       int n, int t0, int H, int Tcap) {
  const int C = H * 64, per_row = 2 * C / 8;
  const size_t at = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = at < (size_t)B * n * per_row;
  const size_t i = live ? at : 0;
  const int j = (int)(i % per_row);
  const size_t row = i / per_row;
  const int t = (int)(row % n), b = (int)(row / n);
  const int col = 8 * j;  // in [0, 2C): K then V
  const int which = col / C, c = col % C, h = c / 64, d = c % 64;
  const typename KV::Row r =
      KV::from_qkv(*reinterpret_cast<const bf16x8*>(qkv + ((size_t)b * T_src + t) * 3 * C + C + col));
  if (!live) return;
  const KV& dst = which ? vc : kc;
  const KvLane w((size_t)b * H + h, Tcap, d / 8);
  dst.store(w, t0 + t, r);
  if (d == 0) dst.store_once(w, t0 + t, r);
}

// ---------------------------------------------------------------------------------------------------------------
// Single-query attention. One wave per (range of 32 keys, b, h): lane (kk = lane / 8, dg = lane % 8) holds dims
// 8 dg .. 8 dg + 7 of keys k0 + kk + 8 i, i < 4 (the 8 lanes of a key read its 128-byte row), so a K or V load of the
// wave is 8 whole rows. The key at pos is the new token's: its lanes take k and v from qkv and write them to the
// cache (no lane reads what another wrote). Scores in fp32, one softmax over the range, partial (max, sum, acc[64])
// to the workspace; attn_combine_kernel merges the ranges in order.
constexpr int AD_KEYS = 32;

// A position per row: the host array of the C entry, validated there and passed by value as a kernel argument, so a
// kernel never indexes memory with a position nobody checked. Indexed by blockIdx: scalar loads.
struct RowPos {
  int v[GPT2MI_DECODE_MAX_B];
};

// The arithmetic of one (row, range) once its 32 keys and values are in registers, written once for attn_row and for
// attn_shared below: q is the row's scaled query, the lane's key i is kr[i] and its value vr[i], and the partial
// (max, sum, acc[64]) goes to workspace slot `slot`. Same operations in the same order whoever loaded the keys: that is
// what makes a shared load bit-identical to the row's own.
template <class KV>
__device__ __forceinline__ void attn_range(const float* q, const typename KV::Row* kr, const typename KV::Row* vr,
                                           float* __restrict__ ws_ml, float* __restrict__ ws_acc, int range, int pos,
                                           size_t slot, int kk, int dg) {
  float s[4], mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float kf[8], d = 0.f;
    KV::key8(kr[i], kf);
#pragma unroll
    for (int j = 0; j < 8; ++j) d = __builtin_fmaf(q[j], kf[j], d);
    d += __shfl_xor(d, 1, 64);
    d += __shfl_xor(d, 2, 64);
    d += __shfl_xor(d, 4, 64);
    d *= KV::score_scale(kr[i]);
    s[i] = (range * AD_KEYS + kk + 8 * i <= pos) ? d : -INFINITY;
    mx = fmaxf(mx, s[i]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 8, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // finite: the range's first key is <= pos

  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, l = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float p = __expf(s[i] - mx);  // 0 for a masked key
    float vf[8];
    KV::value8(vr[i], vf);
    l += p;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(p, vf[j], acc[j]);
  }
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
    l += __shfl_xor(l, o, 64);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += __shfl_xor(acc[j], o, 64);
  }
  if (kk == 0) {
    float* a = ws_acc + slot * 64 + 8 * dg;
    *reinterpret_cast<f32x4*>(a) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4*>(a + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
    if (dg == 0) {
      ws_ml[2 * slot] = mx;
      ws_ml[2 * slot + 1] = l;
    }
  }
}

// The work of one wave, written once for both entries: row r of the launch at position pos, keys range * 32 .. + 31 of
// the cache stream `stream` = seq * H + h (formed by the entry, in the width its seq needs). The keys of a row come
// from two places: a key below `first` from the cache (written by an earlier call), a key in first..pos from the qkv
// row that sits at that position, r - (pos - key): the rows of a sequence in one launch are a contiguous run at
// consecutive positions and `first` is the position of the run's first row. The keys of this call are never read from
// the cache: other waves of this launch are writing them. The row at position t alone writes k / v to position t of
// its stream, so every position has one writer, and nothing above pos is read. The bits of a key are the same from
// either source (the cache holds what KV::from_qkv makes of the qkv row, and a key of the call is held as exactly that),
// so a row gets the same bits whether its run is fed in one call or one row per call. RUN = false is the run of one
// (first == pos, the only qkv row read is the row's own) as a compile-time choice: from first == pos alone the compiler
// does not drop the row offset (pos - key) * 3C.
// A wave whose range starts beyond pos leaves before any load or store (wave-uniform: one wave per block, range and
// row from blockIdx; the body has no barrier), so its workspace slot stays unwritten and attn_combine_kernel does not
// read it. The workspace slot is that of row r, not of the sequence.
template <bool RUN, class KV>
__device__ __forceinline__ void attn_row(const bf16* __restrict__ qkv, const KV& kc, const KV& vc,
                                         float* __restrict__ ws_ml, float* __restrict__ ws_acc, int H, int Tcap,
                                         int nr_max, int r, size_t stream, int pos, int first) {
  const int range = blockIdx.x, h = blockIdx.y;
  if (range * AD_KEYS > pos) return;
  const int lane = threadIdx.x, kk = lane >> 3, dg = lane & 7;
  const int C = H * 64;
  const bf16* tok = qkv + (size_t)r * 3 * C + h * 64 + 8 * dg;  // q; k at + C, v at + 2C
  float q[8];
  unpack8(*reinterpret_cast<const bf16x8*>(tok), q);
#pragma unroll
  for (int j = 0; j < 8; ++j) q[j] *= 0.125f;  // 1/sqrt(64), exact

  const KvLane w(stream, Tcap, dg);
  typename KV::Row kr[4], vr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int key = range * AD_KEYS + kk + 8 * i;
    kr[i] = vr[i] = KV::zero();
    if (key < first) {
      kr[i] = kc.load(w, key);
      vr[i] = vc.load(w, key);
    } else if (RUN ? key <= pos : key == pos) {  // (the 8 lanes of a key agree)
      const bf16* src = RUN ? tok - (ptrdiff_t)(pos - key) * 3 * C : tok;  // the run's row at position key
      kr[i] = KV::from_qkv(*reinterpret_cast<const bf16x8*>(src + C));
      vr[i] = KV::from_qkv(*reinterpret_cast<const bf16x8*>(src + 2 * C));
      if (!RUN || key == pos) {
        kc.store(w, key, kr[i]);
        vc.store(w, key, vr[i]);
        if (dg == 0) {
          kc.store_once(w, key, kr[i]);
          vc.store_once(w, key, vr[i]);
        }
      }
    }
  }

  attn_range<KV>(q, kr, vr, ws_ml, ws_acc, range, pos, (size_t)(r * H + h) * nr_max + range, kk, dg);
}

// Grid (ranges, H, B): row b at rows.v[b] of its own cache stream; the x extent is that of the longest row. b is a grid
// index of its own so that the position is one scalar load from the start of the wave: behind a division of a
// (b, h) index by H every cache load waited for it.
template <class KV>
__global__ __launch_bounds__(64) void attn_decode_kernel(const bf16* __restrict__ qkv, KV kc, KV vc,
                                                         float* __restrict__ ws_ml, float* __restrict__ ws_acc, int H,
                                                         int Tcap, RowPos rows, int nr_max) {
  const int b = blockIdx.z, bh = b * H + blockIdx.y;  // (b < 64: int)
  attn_row<false>(qkv, kc, vc, ws_ml, ws_acc, H, Tcap, nr_max, b, bh, rows.v[b], rows.v[b]);
}

// ---------------------------------------------------------------------------------------------------------------
// Rows that share a prefix (v24). A share group is a set of rows whose streams hold identical bits at positions
// [0, shared_len); a range of 32 keys is shared when it lies wholly below shared_len. The map is built and checked on
// the host (share_map) and travels by value, indexed by blockIdx and by a wave-uniform loop counter only.
// One grid holds both kinds of wave, so sharing adds no launch: z < B is row z, which runs attn_row for its ranges
// from own0[z] upward (the range that straddles shared_len and the key at pos included) and returns at once below;
// z >= B is chunk z - B, up to AD_SHARE_CHUNK members of one group: its wave loads a shared range's keys and values
// once, from the group's lowest row, and runs attn_range for each member with that member's q, into the member's own
// slot. Every slot therefore holds the bits attn_row would have put there and attn_combine_kernel is unchanged. The
// tile's bytes are read once per chunk instead of once per member. The members of a chunk run one after the other, so a
// wave's time grows with the chunk: measured, the smallest chunk is the fastest (half the bytes, twice the work per wave).
#ifndef GPT2MI_SHARE_CHUNK
#define GPT2MI_SHARE_CHUNK 2  // members per wave: DESIGN.md "Shared prompt cache" has the measurements of 2 .. 64
#endif
constexpr int AD_SHARE_CHUNK = GPT2MI_SHARE_CHUNK;
// A step (the plan entries) takes the shared form only when the rows of its sharing groups (two members and a full shared
// range) number at least this: a chunk's members run one after the other in one wave, and below it that wave outlasts
// the whole unshared launch, which is a single round of waves there (measurements: DESIGN.md). A launch choice: bits
// do not depend on it. Read from the map alone. The standalone entries share whatever the map lets them.
#ifndef GPT2MI_SHARE_MIN_ROWS
#define GPT2MI_SHARE_MIN_ROWS 16
#endif
constexpr int AD_SHARE_MIN_ROWS = GPT2MI_SHARE_MIN_ROWS;
constexpr int AD_MAX_CHUNKS = GPT2MI_DECODE_MAX_B;  // a group of n >= 2 rows has ceil(n / chunk) <= n - 1 chunks
static_assert(AD_SHARE_CHUNK >= 2, "a chunk of one member shares nothing");


struct ShareMap {
  int B, chunks;
  int pos[GPT2MI_DECODE_MAX_B];     // RowPos
  int own0[GPT2MI_DECODE_MAX_B];    // the first range row b computes from its own stream
  int member[GPT2MI_DECODE_MAX_B];  // the rows of the chunks, chunk after chunk
  int c_src[AD_MAX_CHUNKS], c_start[AD_MAX_CHUNKS], c_count[AD_MAX_CHUNKS], c_ranges[AD_MAX_CHUNKS];
};

// The wave of chunk c: ranges below c_ranges[c] (all 32 keys below shared_len <= every member's pos: no key of this call,
// no mask). The load is attn_row's `key < first` branch on the source row's stream.
template <class KV>
__device__ __forceinline__ void attn_shared(const bf16* __restrict__ qkv, const KV& kc, const KV& vc,
                                            float* __restrict__ ws_ml, float* __restrict__ ws_acc, int H, int Tcap,
                                            int nr_max, const ShareMap& m, int c) {
  const int range = blockIdx.x, h = blockIdx.y;
  if (range >= m.c_ranges[c]) return;
  const int lane = threadIdx.x, kk = lane >> 3, dg = lane & 7;
  const int C = H * 64;
  const KvLane w((size_t)(m.c_src[c] * H + h), Tcap, dg);
  typename KV::Row kr[4], vr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int key = range * AD_KEYS + kk + 8 * i;
    kr[i] = kc.load(w, key);
    vr[i] = vc.load(w, key);
  }
  // The members run one after the other, so a member's q is loaded while the one before it computes: the wave's time is
  // what a chunk costs, and a load's latency per member would be most of it.
  const int start = m.c_start[c], count = m.c_count[c];
  const bf16* q0 = qkv + h * 64 + 8 * dg;
  int r_next = m.member[start];
  bf16x8 q_next = *reinterpret_cast<const bf16x8*>(q0 + (size_t)r_next * 3 * C);
  for (int j = 0; j < count; ++j) {
    const int r = r_next;
    float q[8];
    unpack8(q_next, q);
    if (j + 1 < count) {
      r_next = m.member[start + j + 1];
      q_next = *reinterpret_cast<const bf16x8*>(q0 + (size_t)r_next * 3 * C);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] *= 0.125f;
    attn_range<KV>(q, kr, vr, ws_ml, ws_acc, range, m.pos[r], (size_t)(r * H + h) * nr_max + range, kk, dg);
  }
}

// Grid (ranges, H, B + chunks).
template <class KV>
__global__ __launch_bounds__(64) void attn_decode_shared_kernel(const bf16* __restrict__ qkv, KV kc, KV vc,
                                                                float* __restrict__ ws_ml, float* __restrict__ ws_acc,
                                                                int H, int Tcap, ShareMap m, int nr_max) {
  const int z = blockIdx.z;
  if (z >= m.B) return attn_shared(qkv, kc, vc, ws_ml, ws_acc, H, Tcap, nr_max, m, z - m.B);
  if ((int)blockIdx.x < m.own0[z]) return;
  attn_row<false>(qkv, kc, vc, ws_ml, ws_acc, H, Tcap, nr_max, z, z * H + blockIdx.y, m.pos[z], m.pos[z]);
}

// out[b, h*64 + d] = sum_r e^(m_r - m) acc_r[d] / sum_r e^(m_r - m) l_r over the pos[b] / 32 + 1 ranges of row b, in
// range order; lane d, grid (H, B).
__global__ __launch_bounds__(64) void attn_combine_kernel(const float* __restrict__ ws_ml,
                                                          const float* __restrict__ ws_acc, bf16* __restrict__ out,
                                                          int H, RowPos rows, int nr_max) {
  const int d = threadIdx.x, h = blockIdx.x, b = blockIdx.y, bh = b * H + h;
  const int nr = rows.v[b] / AD_KEYS + 1;
  const size_t slot0 = (size_t)bh * nr_max;
  float m = -INFINITY;
  for (int r = 0; r < nr; ++r) m = fmaxf(m, ws_ml[2 * (slot0 + r)]);
  float l = 0.f, o = 0.f;
  for (int r = 0; r < nr; ++r) {
    const float w = __expf(ws_ml[2 * (slot0 + r)] - m);
    l = __builtin_fmaf(w, ws_ml[2 * (slot0 + r) + 1], l);
    o = __builtin_fmaf(w, ws_acc[(slot0 + r) * 64 + d], o);
  }
  out[(size_t)bh * 64 + d] = f2bf(o / l);
}

// ---------------------------------------------------------------------------------------------------------------
// Several rows of one launch in the same sequence (gpt2mi_attn_extend): row r is (sequence seq[r], position pos[r]),
// the rows of a sequence are one contiguous run at consecutive positions and first[r] is the position of the run's
// first row. Validated on the host and passed by value like RowPos; indexed by blockIdx only.
struct RowMap {
  int seq[GPT2MI_DECODE_MAX_B], pos[GPT2MI_DECODE_MAX_B], first[GPT2MI_DECODE_MAX_B];
};

// Grid (ranges, H, R): several rows of one launch in the same sequence; the combine is attn_combine_kernel over R rows
// at pos[r].
template <class KV>
__global__ __launch_bounds__(64) void attn_extend_kernel(const bf16* __restrict__ qkv, KV kc, KV vc,
                                                         float* __restrict__ ws_ml, float* __restrict__ ws_acc, int H,
                                                         int Tcap, RowMap rows, int nr_max) {
  const int r = blockIdx.z;
  attn_row<true>(qkv, kc, vc, ws_ml, ws_acc, H, Tcap, nr_max, r, (size_t)rows.seq[r] * H + blockIdx.y, rows.pos[r],
                 rows.first[r]);
}

// One row per blockIdx.y, so that the row's position is a scalar load of the argument.
__global__ __launch_bounds__(256) void embed_decode_kernel(const int64_t* __restrict__ tok,
                                                           const float* __restrict__ wte,
                                                           const float* __restrict__ wpe, float* __restrict__ x, int C,
                                                           RowPos rows) {
  const int b = blockIdx.y, c = 4 * (blockIdx.x * 256 + threadIdx.x);  // one thread per 4 floats
  if (c >= C) return;
  const f32x4 e = *reinterpret_cast<const f32x4*>(wte + (size_t)tok[b] * C + c);
  const f32x4 p = *reinterpret_cast<const f32x4*>(wpe + (size_t)rows.v[b] * C + c);
  *reinterpret_cast<f32x4*>(x + (size_t)b * C + c) = e + p;
}

int attn_ranges(int Tcap) { return (Tcap + AD_KEYS - 1) / AD_KEYS; }

template <int MT>
int skinny_launch(int epi, const SkinnySplit& sp, const bf16* A, int lda, const bf16* W, int ldw, void* C, int ldc,
                  const float* bias, const float* resid, float* partial, int M, int N, hipStream_t s) {
  const dim3 grid(N / 16, sp.slices);
  const int threads = 64 * sp.nw;
#define X(E)                                                                                                     \
  if (epi == E)                                                                                                  \
    skinny_gemm_kernel<MT, E><<<grid, threads, 0, s>>>(A, lda, W, ldw, C, ldc, bias, resid, partial, M, N, sp.chunks, \
                                                       sp.cpu);
  X(SK_BF16) X(SK_F32) X(SK_RESID) X(SK_GELU)
#undef X
  return gpt2mi::check_launch("gemm_skinny");
}

}  // namespace

GPT2MI_EXPORT size_t gpt2mi_gemm_skinny_workspace(int M, int N, int K) {
  if (M < 1 || N < 64 || K < 64 || N % 64 || K % 64) return 0;
  const SkinnySplit sp = skinny_split(N, K);
  return sp.slices > 1 ? (size_t)sp.slices * M * N : 0;
}

GPT2MI_EXPORT int gpt2mi_gemm_skinny(int epilogue, int M, int N, int K, const uint16_t* A, int lda, const uint16_t* W,
                                     int ldw, void* C, int ldc, const float* bias, const float* resid,
                                     float* workspace, size_t workspace_floats, void* stream) {
  GPT2MI_REQUIRE(epilogue >= SK_BF16 && epilogue <= SK_GELU, "gemm_skinny: epilogue %d not in [0, 3]", epilogue);
  GPT2MI_REQUIRE(M >= 1 && M <= 64, "gemm_skinny: M=%d not in [1, 64] (larger M: gpt2mi_gemm)", M);
  GPT2MI_REQUIRE(N >= 64 && K >= 64 && N % 64 == 0 && K % 64 == 0,
                 "gemm_skinny: N=%d and K=%d must be positive multiples of 64", N, K);
  GPT2MI_REQUIRE(lda >= K && ldw >= K && ldc >= N && lda % 8 == 0 && ldw % 8 == 0 && ldc % 4 == 0,
                 "gemm_skinny: lda=%d, ldw=%d (>= K, multiples of 8) or ldc=%d (>= N, multiple of 4) invalid", lda, ldw,
                 ldc);
  const SkinnySplit sp = skinny_split(N, K);
  const size_t need = sp.slices > 1 ? (size_t)sp.slices * M * N : 0;
  GPT2MI_REQUIRE(workspace_floats >= need,
                 "gemm_skinny: workspace too small (%zu floats given, %zu needed for %d K slices)", workspace_floats, need,
                 sp.slices);
  GPT2MI_REQUIRE(A && W && C && (need == 0 || workspace), "gemm_skinny: A, W, C or a needed workspace is NULL");
  GPT2MI_REQUIRE(epilogue != SK_RESID || resid, "gemm_skinny: the RESID epilogue needs resid");
  hipStream_t s = (hipStream_t)stream;
  float* partial = need ? workspace : nullptr;
  const bf16 *a = (const bf16*)A, *w = (const bf16*)W;
  int rc;
  switch ((M + 15) / 16) {
    case 1: rc = skinny_launch<1>(epilogue, sp, a, lda, w, ldw, C, ldc, bias, resid, partial, M, N, s); break;
    case 2: rc = skinny_launch<2>(epilogue, sp, a, lda, w, ldw, C, ldc, bias, resid, partial, M, N, s); break;
    case 3: rc = skinny_launch<3>(epilogue, sp, a, lda, w, ldw, C, ldc, bias, resid, partial, M, N, s); break;
    default: rc = skinny_launch<4>(epilogue, sp, a, lda, w, ldw, C, ldc, bias, resid, partial, M, N, s); break;
  }
  if (rc || !partial) return rc;
  const int g = (M * (N / 4) + 255) / 256;
#define X(E) \
  if (epilogue == E) skinny_reduce_kernel<E><<<g, 256, 0, s>>>(partial, sp.slices, C, ldc, bias, resid, M, N);
  X(SK_BF16) X(SK_F32) X(SK_RESID) X(SK_GELU)
#undef X
  return gpt2mi::check_launch("gemm_skinny reduce");
}

namespace {
// The cache of one layer as an entry received it: the format, the two tensors (bf16, or the fp8 codes) and, with fp8,
// their scales. The entries and the plan's attention call form one; everything between them passes it on.
struct KvCache {
  int format;  // GPT2MI_KV_BF16 / GPT2MI_KV_FP8
  void *k, *v;
  float *ks, *vs;
};

// 22 with a message unless the scales an fp8 cache needs are there (a bf16 cache has none).
int kv_scales(const char* what, const KvCache& kv) {
  GPT2MI_REQUIRE(kv.format != GPT2MI_KV_FP8 || (kv.ks && kv.vs), "%s: kscale and vscale of the fp8 cache must not be NULL",
                 what);
  return 0;
}

// The one place that turns the format into the kernels' cache type: f(keys, values), as KvBf16 or as KvFp8.
template <class F>
void kv_typed(const KvCache& kv, F f) {
  if (kv.format == GPT2MI_KV_FP8)
    f(KvFp8{(uint8_t*)kv.k, kv.ks}, KvFp8{(uint8_t*)kv.v, kv.vs});
  else
    f(KvBf16{(bf16*)kv.k}, KvBf16{(bf16*)kv.v});
}

int kv_store_rows(const char* what, const uint16_t* qkv, const KvCache& kv, int B, int T_src, int n, int t0, int H,
                  int head_dim, int Tcap, void* stream) {
  GPT2MI_REQUIRE(head_dim == 64, "%s: head_dim=%d (the decode kernels implement 64)", what, head_dim);
  GPT2MI_REQUIRE(B >= 1 && H >= 1 && Tcap >= 1, "%s: B=%d, H=%d, Tcap=%d must be positive", what, B, H, Tcap);
  GPT2MI_REQUIRE(n >= 1 && n <= T_src, "%s: n=%d not in [1, T_src=%d]", what, n, T_src);
  GPT2MI_REQUIRE(t0 >= 0 && (long long)t0 + n <= Tcap, "%s: t0=%d + n=%d exceeds the cache length Tcap=%d", what, t0, n,
                 Tcap);
  if (const int rc = kv_scales(what, kv)) return rc;
  GPT2MI_REQUIRE(qkv && kv.k && kv.v, "%s: qkv and the caches must not be NULL", what);
  const size_t total = (size_t)B * n * (2 * H * 64 / 8);
  const unsigned grid = (unsigned)((total + 255) / 256);
  kv_typed(kv, [&](auto kc, auto vc) {
    kv_store_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const bf16*)qkv, kc, vc, B, T_src, n, t0, H, Tcap);
  });
  return gpt2mi::check_launch(what);
}
}  // namespace

GPT2MI_EXPORT int gpt2mi_kv_store(const uint16_t* qkv, uint16_t* kcache, uint16_t* vcache, int B, int T_src, int n,
                                  int t0, int H, int head_dim, int Tcap, void* stream) {
  return kv_store_rows("kv_store", qkv, KvCache{GPT2MI_KV_BF16, kcache, vcache, nullptr, nullptr}, B, T_src, n, t0, H,
                       head_dim, Tcap, stream);
}

GPT2MI_EXPORT int gpt2mi_kv_store_fp8(const uint16_t* qkv, uint8_t* kcache, uint8_t* vcache, float* kscale,
                                      float* vscale, int B, int T_src, int n, int t0, int H, int head_dim, int Tcap,
                                      void* stream) {
  return kv_store_rows("kv_store_fp8", qkv, KvCache{GPT2MI_KV_FP8, kcache, vcache, kscale, vscale}, B, T_src, n, t0, H,
                       head_dim, Tcap, stream);
}

GPT2MI_EXPORT size_t gpt2mi_attn_decode_workspace(int B, int H, int Tcap) {
  if (B < 1 || H < 1 || Tcap < 1) return 0;
  return (size_t)B * H * attn_ranges(Tcap) * 66;  // (max, sum) + acc[64] per range
}

namespace {
// The position array of an entry: B in [1, GPT2MI_DECODE_MAX_B] host ints, each in [0, limit). 22 with a message naming
// `what` otherwise; on success *out holds them (entries >= B are 0) and *max_pos the largest.
int row_positions(const char* what, const int* pos, int B, int limit, RowPos* out, int* max_pos) {
  GPT2MI_REQUIRE(B >= 1 && B <= GPT2MI_DECODE_MAX_B, "%s: B=%d not in [1, %d]", what, B, GPT2MI_DECODE_MAX_B);
  GPT2MI_REQUIRE(pos != nullptr, "%s: the position array (host, B ints) is NULL", what);
  *out = RowPos{};
  *max_pos = 0;
  for (int b = 0; b < B; ++b) {
    GPT2MI_REQUIRE(pos[b] >= 0 && pos[b] < limit, "%s: pos[%d]=%d not in [0, %d)", what, b, pos[b], limit);
    out->v[b] = pos[b];
    *max_pos = std::max(*max_pos, pos[b]);
  }
  return 0;
}

// The share map of an entry (v24), checked next to its positions and in their message format: share_group and share_len
// are HOST arrays of B ints, both NULL for no sharing. share_group[b] is the lowest row of b's group (b itself when
// alone), share_len[b] the group's shared length (0 when alone). 22 with a message naming `what` and the index
// otherwise. On success *out is the kernel's map at the positions rp: out->chunks == 0 when no group has two members and
// a full shared range, or when fewer than min_rows rows are in such groups, and the caller then launches the unshared
// kernels. What is shared is read from the map alone.
int share_map(const char* what, const int* share_group, const int* share_len, int B, const RowPos& rp, ShareMap* out,
              int min_rows = 2) {
  GPT2MI_REQUIRE((share_group == nullptr) == (share_len == nullptr),
                 "%s: share_group and share_len (host, B ints) go together: %s is NULL", what,
                 share_group ? "share_len" : "share_group");
  *out = ShareMap{};
  out->B = B;
  std::copy_n(rp.v, GPT2MI_DECODE_MAX_B, out->pos);
  if (!share_group) return 0;
  int members[GPT2MI_DECODE_MAX_B] = {};
  for (int b = 0; b < B; ++b) {
    const int g = share_group[b];
    GPT2MI_REQUIRE(g >= 0 && g <= b, "%s: share_group[%d]=%d not in [0, %d]", what, b, g, b);
    GPT2MI_REQUIRE(share_group[g] == g, "%s: share_group[%d]=%d is not its group's lowest row (share_group[%d]=%d)", what,
                   b, g, g, share_group[g]);
    GPT2MI_REQUIRE(share_len[b] >= 0, "%s: share_len[%d]=%d is negative", what, b, share_len[b]);
    GPT2MI_REQUIRE(share_len[b] <= rp.v[b], "%s: share_len[%d]=%d exceeds pos[%d]=%d", what, b, share_len[b], b, rp.v[b]);
    GPT2MI_REQUIRE(share_len[b] == share_len[g], "%s: share_len[%d]=%d differs from its group's share_len[%d]=%d", what, b,
                   share_len[b], g, share_len[g]);
    ++members[g];
  }
  for (int b = 0; b < B; ++b)
    GPT2MI_REQUIRE(members[share_group[b]] > 1 || share_len[b] == 0,
                   "%s: share_len[%d]=%d for a row alone in its group (must be 0)", what, b, share_len[b]);
  int at = 0;
  for (int g = 0; g < B; ++g) {
    const int ranges = share_len[g] / AD_KEYS;
    if (share_group[g] != g || members[g] < 2 || ranges < 1) continue;
    for (int b = g, n = 0; b < B; ++b) {
      if (share_group[b] != g) continue;
      if (n % AD_SHARE_CHUNK == 0) {
        const int c = out->chunks++;
        out->c_src[c] = g, out->c_start[c] = at, out->c_count[c] = 0, out->c_ranges[c] = ranges;
      }
      ++out->c_count[out->chunks - 1], ++n;
      out->member[at++] = b;
      out->own0[b] = ranges;
    }
  }
  if (at < min_rows) {  // too few rows share for the shared form to pay: every row reads its own stream
    out->chunks = 0;
    std::fill_n(out->own0, GPT2MI_DECODE_MAX_B, 0);
  }
  return 0;
}

using gpt2mi::SamePos;

// The tail the two attention entries share, after their own row checks: M rows whose kernel argument is `rows`, at the
// positions rp (the longest max_pos). The workspace is M * H * nr_max (max, sum) pairs, then as many acc[64].
// `kernel` names the entry's kernel template: KV_KERNEL(name) gives name<KV> for the cache type it is shown.
#define KV_KERNEL(name) [](auto kc) { return name<decltype(kc)>; }
template <class Rows, class Kernel>
int attn_launch(const char* what, Kernel kernel, const Rows& rows, const RowPos& rp, int max_pos, const uint16_t* qkv,
                const KvCache& kv, uint16_t* out, float* workspace, size_t workspace_floats, int M, int H, int Tcap,
                void* stream, int extra_z = 0) {
  const size_t need = gpt2mi_attn_decode_workspace(M, H, Tcap);
  GPT2MI_REQUIRE(workspace_floats >= need, "%s: workspace too small (%zu floats given, %zu needed)", what,
                 workspace_floats, need);
  if (const int rc = kv_scales(what, kv)) return rc;
  GPT2MI_REQUIRE(qkv && kv.k && kv.v && out && workspace, "%s: qkv, the caches, out and workspace must not be NULL",
                 what);
  hipStream_t s = (hipStream_t)stream;
  const int nr_max = attn_ranges(Tcap);
  float* ws_ml = workspace;
  float* ws_acc = workspace + (size_t)M * H * nr_max * 2;
  const dim3 grid(max_pos / AD_KEYS + 1, H, M + extra_z);  // (extra_z: the chunks of a shared launch)
  kv_typed(kv, [&](auto kc, auto vc) {
    kernel(kc)<<<grid, 64, 0, s>>>((const bf16*)qkv, kc, vc, ws_ml, ws_acc, H, Tcap, rows, nr_max);
  });
  if (const int rc = gpt2mi::check_launch(what)) return rc;
  attn_combine_kernel<<<dim3(H, M), 64, 0, s>>>(ws_ml, ws_acc, (bf16*)out, H, rp, nr_max);
  return gpt2mi::check_launch(what);
}

// One position per row, at checked positions rp and under a checked map sm (sm.pos is rp): the launch the map asks for.
int attn_decode_mapped(const char* what, const uint16_t* qkv, const KvCache& kv, uint16_t* out, float* workspace,
                       size_t workspace_floats, int B, int H, int Tcap, const RowPos& rp, int max_pos,
                       const ShareMap& sm, void* stream) {
  if (sm.chunks)  // some range is shared: the one launch that holds both kinds of wave
    return attn_launch(what, KV_KERNEL(attn_decode_shared_kernel), sm, rp, max_pos, qkv, kv, out, workspace,
                       workspace_floats, B, H, Tcap, stream, sm.chunks);
  return attn_launch(what, KV_KERNEL(attn_decode_kernel), rp, rp, max_pos, qkv, kv, out, workspace, workspace_floats, B,
                     H, Tcap, stream);
}

// Each operation below is written once, for one position per row; `what` is the entry's name in its messages. The
// standalone attention entries: they share whatever the map lets them (share_map's min_rows = 2).
int attn_decode_rows(const char* what, const uint16_t* qkv, const KvCache& kv, uint16_t* out, float* workspace,
                     size_t workspace_floats, int B, int H, int head_dim, int Tcap, const int* pos, void* stream,
                     const int* share_group = nullptr, const int* share_len = nullptr) {
  GPT2MI_REQUIRE(head_dim == 64, "%s: head_dim=%d (the decode kernels implement 64)", what, head_dim);
  GPT2MI_REQUIRE(B >= 1 && H >= 1 && H <= 65535 && Tcap >= 1, "%s: B=%d, H=%d (<= 65535), Tcap=%d must be positive", what,
                 B, H, Tcap);
  RowPos rp;
  int max_pos;
  if (const int rc = row_positions(what, pos, B, Tcap, &rp, &max_pos)) return rc;
  ShareMap sm;
  if (const int rc = share_map(what, share_group, share_len, B, rp, &sm)) return rc;
  return attn_decode_mapped(what, qkv, kv, out, workspace, workspace_floats, B, H, Tcap, rp, max_pos, sm, stream);
}

int embed_decode_rows(const char* what, const int64_t* tok, const float* wte, const float* wpe, float* x, int B, int C,
                      const int* pos, void* stream) {
  GPT2MI_REQUIRE(C >= 4 && C % 4 == 0, "%s: C=%d must be a positive multiple of 4", what, C);
  RowPos rp;
  int max_pos;
  if (const int rc = row_positions(what, pos, B, INT_MAX, &rp, &max_pos)) return rc;
  GPT2MI_REQUIRE(tok && wte && wpe && x, "%s: tok, wte, wpe and x must not be NULL", what);
  embed_decode_kernel<<<dim3((C / 4 + 255) / 256, B), 256, 0, (hipStream_t)stream>>>(tok, wte, wpe, x, C, rp);
  return gpt2mi::check_launch(what);
}
}  // namespace

GPT2MI_EXPORT int gpt2mi_attn_decode_ragged(const uint16_t* qkv, uint16_t* kcache, uint16_t* vcache, uint16_t* out,
                                            float* workspace, size_t workspace_floats, int B, int H, int head_dim,
                                            int Tcap, const int* pos, void* stream) {
  return attn_decode_rows("attn_decode_ragged", qkv, KvCache{GPT2MI_KV_BF16, kcache, vcache, nullptr, nullptr}, out,
                          workspace, workspace_floats, B, H, head_dim, Tcap, pos, stream);
}

GPT2MI_EXPORT int gpt2mi_attn_decode_fp8_ragged(const uint16_t* qkv, uint8_t* kcache, uint8_t* vcache, float* kscale,
                                                float* vscale, uint16_t* out, float* workspace,
                                                size_t workspace_floats, int B, int H, int head_dim, int Tcap,
                                                const int* pos, void* stream) {
  return attn_decode_rows("attn_decode_fp8_ragged", qkv, KvCache{GPT2MI_KV_FP8, kcache, vcache, kscale, vscale}, out,
                          workspace, workspace_floats, B, H, head_dim, Tcap, pos, stream);
}

GPT2MI_EXPORT int gpt2mi_attn_decode_shared(const uint16_t* qkv, uint16_t* kcache, uint16_t* vcache, uint16_t* out,
                                            float* workspace, size_t workspace_floats, int B, int H, int head_dim,
                                            int Tcap, const int* pos, const int* share_group, const int* share_len,
                                            void* stream) {
  return attn_decode_rows("attn_decode_shared", qkv, KvCache{GPT2MI_KV_BF16, kcache, vcache, nullptr, nullptr}, out,
                          workspace, workspace_floats, B, H, head_dim, Tcap, pos, stream, share_group, share_len);
}

GPT2MI_EXPORT int gpt2mi_attn_decode_shared_fp8(const uint16_t* qkv, uint8_t* kcache, uint8_t* vcache, float* kscale,
                                                float* vscale, uint16_t* out, float* workspace,
                                                size_t workspace_floats, int B, int H, int head_dim, int Tcap,
                                                const int* pos, const int* share_group, const int* share_len,
                                                void* stream) {
  return attn_decode_rows("attn_decode_shared_fp8", qkv, KvCache{GPT2MI_KV_FP8, kcache, vcache, kscale, vscale}, out,
                          workspace, workspace_floats, B, H, head_dim, Tcap, pos, stream, share_group, share_len);
}

GPT2MI_EXPORT int gpt2mi_attn_decode(const uint16_t* qkv, uint16_t* kcache, uint16_t* vcache, uint16_t* out,
                                     float* workspace, size_t workspace_floats, int B, int H, int head_dim, int Tcap,
                                     int pos, void* stream) {
  GPT2MI_REQUIRE(pos >= 0 && pos < Tcap, "attn_decode: pos=%d not in [0, Tcap=%d)", pos, Tcap);
  return attn_decode_rows("attn_decode", qkv, KvCache{GPT2MI_KV_BF16, kcache, vcache, nullptr, nullptr}, out, workspace,
                          workspace_floats, B, H, head_dim, Tcap, SamePos(pos).v, stream);
}

GPT2MI_EXPORT int gpt2mi_embed_decode_ragged(const int64_t* tok, const float* wte, const float* wpe, float* x, int B,
                                             int C, const int* pos, void* stream) {
  return embed_decode_rows("embed_decode_ragged", tok, wte, wpe, x, B, C, pos, stream);
}

GPT2MI_EXPORT int gpt2mi_embed_decode(const int64_t* tok, const float* wte, const float* wpe, float* x, int B, int C,
                                      int pos, void* stream) {
  GPT2MI_REQUIRE(pos >= 0, "embed_decode: pos=%d is negative", pos);
  return embed_decode_rows("embed_decode", tok, wte, wpe, x, B, C, SamePos(pos).v, stream);
}

namespace {
// The row map of an extend entry: R in [1, GPT2MI_DECODE_MAX_B] rows, seq and pos HOST arrays of R ints. seq[r] in
// [0, B) and non-decreasing, pos[r] in [0, Tcap), and within a sequence pos ascends by 1: so the rows of a sequence are
// one contiguous run, the run's row at position t (first[r] <= t <= pos[r]) is row r - (pos[r] - t) >= the run's first
// row, and every cache index (seq[r], h, t <= pos[r]) lies inside [B][H][Tcap]. 22 with a message otherwise.
int row_map(const char* what, const int* seq, const int* pos, int R, int B, int Tcap, RowMap* out, int* max_pos) {
  GPT2MI_REQUIRE(R >= 1 && R <= GPT2MI_DECODE_MAX_B, "%s: R=%d not in [1, %d]", what, R, GPT2MI_DECODE_MAX_B);
  GPT2MI_REQUIRE(seq != nullptr, "%s: the sequence array (host, R ints) is NULL", what);
  GPT2MI_REQUIRE(pos != nullptr, "%s: the position array (host, R ints) is NULL", what);
  *out = RowMap{};
  *max_pos = 0;
  for (int r = 0; r < R; ++r) {
    GPT2MI_REQUIRE(seq[r] >= 0 && seq[r] < B, "%s: seq[%d]=%d not in [0, B=%d)", what, r, seq[r], B);
    GPT2MI_REQUIRE(r == 0 || seq[r] >= seq[r - 1], "%s: seq[%d]=%d after seq[%d]=%d: the sequences must not decrease",
                   what, r, seq[r], r - 1, r ? seq[r - 1] : 0);
    GPT2MI_REQUIRE(pos[r] >= 0 && pos[r] < Tcap, "%s: pos[%d]=%d not in [0, %d)", what, r, pos[r], Tcap);
    const bool same = r > 0 && seq[r] == seq[r - 1];
    GPT2MI_REQUIRE(!same || pos[r] == pos[r - 1] + 1,
                   "%s: pos[%d]=%d does not follow pos[%d]=%d in sequence %d (a run ascends by 1)", what, r, pos[r],
                   r - 1, r ? pos[r - 1] : 0, seq[r]);
    out->seq[r] = seq[r];
    out->pos[r] = pos[r];
    out->first[r] = same ? out->first[r - 1] : pos[r];
    *max_pos = std::max(*max_pos, pos[r]);
  }
  return 0;
}

int attn_extend_rows(const char* what, const uint16_t* qkv, const KvCache& kv, uint16_t* out, float* workspace,
                     size_t workspace_floats, int R, int B, int H, int head_dim, int Tcap, const int* seq,
                     const int* pos, void* stream) {
  GPT2MI_REQUIRE(head_dim == 64, "%s: head_dim=%d (the decode kernels implement 64)", what, head_dim);
  GPT2MI_REQUIRE(B >= 1 && H >= 1 && H <= 65535 && Tcap >= 1, "%s: B=%d, H=%d (<= 65535), Tcap=%d must be positive", what,
                 B, H, Tcap);
  RowMap rm;
  int max_pos;
  if (const int rc = row_map(what, seq, pos, R, B, Tcap, &rm, &max_pos)) return rc;
  RowPos rp{};  // the combine is per row: row r merges its own pos[r] / 32 + 1 ranges
  std::copy_n(rm.pos, R, rp.v);
  return attn_launch(what, KV_KERNEL(attn_extend_kernel), rm, rp, max_pos, qkv, kv, out, workspace, workspace_floats, R,
                     H, Tcap, stream);
}
#undef KV_KERNEL  // its three users are above

// The launch list of a step over M rows at pos[m], shared by the step and the extend: they differ in the attention
// (`attn`, called once per layer between the qkv and the proj GEMM) and in what they checked before.
template <class Attn>
int decode_launches(const char* what, const gpt2mi_decode_plan* P, int M, const int64_t* tok, const int* pos,
                    void* stream, Attn attn) {
#define STEP(call)       \
  do {                   \
    const int rc = call; \
    if (rc) return rc;   \
  } while (0)
  const int C = P->C;
  float *x = P->x, *xmid = P->xmid;
  float* gws = P->gemm_ws;
  const size_t gwn = P->gemm_ws_floats;
  STEP(embed_decode_rows(what, tok, P->wte, P->wpe, x, M, C, pos, stream));
  for (int l = 0; l < P->L; ++l) {
    const gpt2mi_decode_layer& Y = P->layers[l];
    STEP(gpt2mi_layernorm_fwd(x, Y.ln1_w, Y.ln1_b, P->ln, nullptr, P->mean, P->rstd, M, C, P->eps, stream));
    STEP(gpt2mi_gemm_skinny(SK_BF16, M, 3 * C, C, P->ln, C, Y.qkv_w, C, P->qkv, 3 * C, Y.qkv_b, nullptr, gws, gwn, stream));
    STEP(attn(Y));
    STEP(gpt2mi_gemm_skinny(SK_RESID, M, C, C, P->ao, C, Y.proj_w, C, xmid, C, Y.proj_b, x, gws, gwn, stream));
    STEP(gpt2mi_layernorm_fwd(xmid, Y.ln2_w, Y.ln2_b, P->ln, nullptr, P->mean, P->rstd, M, C, P->eps, stream));
    STEP(gpt2mi_gemm_skinny(SK_GELU, M, 4 * C, C, P->ln, C, Y.fc1_w, C, P->h, 4 * C, Y.fc1_b, nullptr, gws, gwn, stream));
    STEP(gpt2mi_gemm_skinny(SK_RESID, M, C, 4 * C, P->h, 4 * C, Y.fc2_w, 4 * C, x, C, Y.fc2_b, xmid, gws, gwn, stream));
  }
  STEP(gpt2mi_layernorm_fwd(x, P->lnf_w, P->lnf_b, P->ln, nullptr, P->mean, P->rstd, M, C, P->eps, stream));
  STEP(gpt2mi_gemm_skinny(SK_F32, M, P->Vp, C, P->ln, C, P->wte_bf16, C, P->logits, P->Vp, nullptr, nullptr, gws, gwn,
                          stream));
#undef STEP
  return 0;
}

// The plan checks of the step and the extend, in two halves around the caller's own row checks: the shape of the plan,
// then its buffers for M rows.
int plan_shape(const char* what, const gpt2mi_decode_plan* P) {
  GPT2MI_REQUIRE(P != nullptr, "%s: plan is NULL", what);
  GPT2MI_REQUIRE(P->B >= 1 && P->B <= 64, "%s: B=%d not in [1, 64]", what, P->B);
  GPT2MI_REQUIRE(P->H >= 1 && P->C == 64 * P->H, "%s: head_dim = C/H must be 64 (C=%d, H=%d)", what, P->C, P->H);
  GPT2MI_REQUIRE(P->L >= 1 && P->Vp >= 64 && P->Vp % 64 == 0, "%s: L=%d, Vp=%d (a multiple of 64) invalid", what, P->L,
                 P->Vp);
  // the cache format: here and in layer_cache, nowhere else
  GPT2MI_REQUIRE(P->kv_format == GPT2MI_KV_BF16 || P->kv_format == GPT2MI_KV_FP8,
                 "%s: kv_format=%d is neither 0 (bf16) nor 1 (fp8 e4m3)", what, P->kv_format);
  if (P->kv_format == GPT2MI_KV_FP8) {
    GPT2MI_REQUIRE(P->layers != nullptr, "%s: layers is NULL", what);
    for (int l = 0; l < P->L; ++l)
      GPT2MI_REQUIRE(P->layers[l].kscale && P->layers[l].vscale,
                     "%s: kv_format=1 (fp8) needs layers[%d].kscale and .vscale: one is NULL", what, l);
  }
  return 0;
}

// The cache of layer Y in the plan's format, for the attention call.
KvCache layer_cache(const gpt2mi_decode_plan* P, const gpt2mi_decode_layer& Y) {
  return KvCache{P->kv_format, Y.kcache, Y.vcache, Y.kscale, Y.vscale};
}

int plan_buffers(const char* what, const gpt2mi_decode_plan* P, int M, const int64_t* tok) {
  const int C = P->C;
  GPT2MI_REQUIRE(P->attn_ws_floats >= gpt2mi_attn_decode_workspace(M, P->H, P->Tcap),
                 "%s: attention workspace too small (%zu floats)", what, P->attn_ws_floats);
  size_t need = 0;
  const int shapes[5][2] = {{3 * C, C}, {C, C}, {4 * C, C}, {C, 4 * C}, {P->Vp, C}};
  for (const auto& sh : shapes) need = std::max(need, gpt2mi_gemm_skinny_workspace(M, sh[0], sh[1]));
  GPT2MI_REQUIRE(P->gemm_ws_floats >= need, "%s: GEMM workspace too small (%zu floats given, %zu needed)", what,
                 P->gemm_ws_floats, need);
  GPT2MI_REQUIRE(P->layers && tok, "%s: layers and tok must not be NULL", what);
  return 0;
}

// One step with row b at pos[b]: gpt2mi_decode_step_ragged, and gpt2mi_decode_step with every pos[b] equal. launch = false:
// the checks alone (a loop's refusals before its first launch).
int decode_step_rows(const char* what, const gpt2mi_decode_plan* P, const int64_t* tok, const int* pos, void* stream,
                     bool launch = true) {
  if (const int rc = plan_shape(what, P)) return rc;
  const int B = P->B, H = P->H;
  RowPos rp;
  int max_pos;
  if (const int rc = row_positions(what, pos, B, P->Tcap, &rp, &max_pos)) return rc;
  GPT2MI_REQUIRE(H <= 65535, "%s: B=%d, H=%d (<= 65535), Tcap=%d must be positive", what, B, H, P->Tcap);
  ShareMap sm;  // refused here, before the first launch; every layer's attention call then launches from this one map
  if (const int rc = share_map(what, P->share_group, P->share_len, B, rp, &sm, AD_SHARE_MIN_ROWS)) return rc;
  if (const int rc = plan_buffers(what, P, B, tok)) return rc;
  if (!launch) return 0;
  return decode_launches(what, P, B, tok, pos, stream, [&](const gpt2mi_decode_layer& Y) {
    return attn_decode_mapped(what, P->qkv, layer_cache(P, Y), P->ao, P->attn_ws, P->attn_ws_floats, B, H, P->Tcap, rp,
                              max_pos, sm, stream);
  });
}
}  // namespace

namespace gpt2mi {
int decode_step_check(const char* what, const gpt2mi_decode_plan* P, const int64_t* tok, const int* pos) {
  return decode_step_rows(what, P, tok, pos, nullptr, false);
}
int decode_step_as(const char* what, const gpt2mi_decode_plan* P, const int64_t* tok, const int* pos, void* stream) {
  return decode_step_rows(what, P, tok, pos, stream);
}
}  // namespace gpt2mi

GPT2MI_EXPORT int gpt2mi_decode_step_ragged(const gpt2mi_decode_plan* P, const int64_t* tok, const int* pos,
                                            void* stream) {
  return decode_step_rows("decode_step_ragged", P, tok, pos, stream);
}

GPT2MI_EXPORT int gpt2mi_decode_step(const gpt2mi_decode_plan* P, const int64_t* tok, int pos, void* stream) {
  GPT2MI_REQUIRE(P != nullptr, "decode_step: plan is NULL");
  GPT2MI_REQUIRE(pos >= 0 && pos < P->Tcap, "decode_step: pos=%d not in [0, Tcap=%d)", pos, P->Tcap);
  return decode_step_rows("decode_step", P, tok, SamePos(pos).v, stream);
}

GPT2MI_EXPORT int gpt2mi_attn_extend(const uint16_t* qkv, uint16_t* kcache, uint16_t* vcache, uint16_t* out,
                                     float* workspace, size_t workspace_floats, int R, int B, int H, int head_dim,
                                     int Tcap, const int* seq, const int* pos, void* stream) {
  return attn_extend_rows("attn_extend", qkv, KvCache{GPT2MI_KV_BF16, kcache, vcache, nullptr, nullptr}, out, workspace,
                          workspace_floats, R, B, H, head_dim, Tcap, seq, pos, stream);
}

GPT2MI_EXPORT int gpt2mi_attn_extend_fp8(const uint16_t* qkv, uint8_t* kcache, uint8_t* vcache, float* kscale,
                                         float* vscale, uint16_t* out, float* workspace, size_t workspace_floats, int R,
                                         int B, int H, int head_dim, int Tcap, const int* seq, const int* pos,
                                         void* stream) {
  return attn_extend_rows("attn_extend_fp8", qkv, KvCache{GPT2MI_KV_FP8, kcache, vcache, kscale, vscale}, out, workspace,
                          workspace_floats, R, B, H, head_dim, Tcap, seq, pos, stream);
}

GPT2MI_EXPORT int gpt2mi_decode_extend(const gpt2mi_decode_plan* P, int R, const int64_t* tok, const int* seq,
                                       const int* pos, void* stream) {
  const char* what = "decode_extend";
  if (const int rc = plan_shape(what, P)) return rc;
  const int B = P->B, H = P->H;
  RowMap rm;
  int max_pos;
  if (const int rc = row_map(what, seq, pos, R, B, P->Tcap, &rm, &max_pos)) return rc;
  const int cap = P->rows ? P->rows : B;
  GPT2MI_REQUIRE(R <= cap, "%s: R=%d exceeds the plan's row capacity %d (plan->rows, 0: B)", what, R, cap);
  if (const int rc = plan_buffers(what, P, R, tok)) return rc;
  return decode_launches(what, P, R, tok, pos, stream, [&](const gpt2mi_decode_layer& Y) {
    return attn_extend_rows(what, P->qkv, layer_cache(P, Y), P->ao, P->attn_ws, P->attn_ws_floats, R, B, H, 64,
                            P->Tcap, seq, pos, stream);
  });
}

namespace {
// The arguments of a token loop as gpt2mi_decode_generate_constrained takes them; an entry without the penalty values,
// lp or con leaves them at these neutral ones.
struct GenerateCall {
  const gpt2mi_decode_plan* plan;
  int V;
  float temperature;
  int top_k;
  float top_p;
  uint64_t seed;
  int64_t eos;
  const int* pos0;
  const uint32_t* row_id;
  int n;
  int64_t *tok, *seq;
  int ld_seq;
  uint8_t* done;
  void* stream;
  float repetition = 1.f, presence = 0.f, frequency = 0.f;
  const int* gen_start = nullptr;
  const gpt2mi_logprobs* lp = nullptr;
  const gpt2mi_constraints* con = nullptr;
};

// The token loop with row b starting at pos0[b]: sample, then (but for the last token) step, n times. With non-neutral
// penalty values (gpt2mi_decode_generate_penalized) seq is the history the sampler reads, row b's own row of it. With
// `lp` (gpt2mi_decode_generate_logprobs; may be NULL) step i writes column pos0[b] + i of it: its col is NULL, the
// sampler's "col[b] = pos[b]". With a non-neutral `con` (gpt2mi_decode_generate_constrained; may be NULL) the draws are
// gpt2mi_sample_constrained's, seq again the history and gen_start where a row's generated part begins.
// The draws are sample_rows' (csrc/sample.hip) on one record, under the name of the sampler entry that takes what is on.
int decode_generate_rows(const char* what, const GenerateCall& g) {
  const gpt2mi_decode_plan* P = g.plan;
  const int V = g.V, n = g.n;
  GPT2MI_REQUIRE(P != nullptr, "%s: plan is NULL", what);
  GPT2MI_REQUIRE(V >= 1 && V <= P->Vp, "%s: V=%d not in [1, Vp=%d]", what, V, P->Vp);
  GPT2MI_REQUIRE(n >= 0, "%s: n=%d must be >= 0", what, n);
  RowPos rp;
  int max_pos;
  if (const int rc = row_positions(what, g.pos0, P->B, P->Tcap, &rp, &max_pos)) return rc;
  for (int b = 0; b < P->B; ++b)
    GPT2MI_REQUIRE(g.pos0[b] >= 1, "%s: pos0[%d]=%d must be >= 1 (after a prefill)", what, b, g.pos0[b]);
  ShareMap sm;  // at pos0: the positions only grow from there, so a map that passes here passes at every step
  if (const int rc = share_map(what, P->share_group, P->share_len, P->B, rp, &sm)) return rc;
  GPT2MI_REQUIRE((long long)max_pos + n <= P->Tcap, "%s: max pos0=%d + n=%d exceeds the cache length Tcap=%d", what,
                 max_pos, n, P->Tcap);
  GPT2MI_REQUIRE(!g.seq || (long long)max_pos + n <= g.ld_seq, "%s: max pos0=%d + n=%d exceeds ld_seq=%d", what, max_pos,
                 n, g.ld_seq);
  bool on;
  if (const int rc = gpt2mi::check_penalty_values(what, g.repetition, g.presence, g.frequency, &on)) return rc;
  const gpt2mi_penalties pen = {g.repetition, g.presence, g.frequency, g.seq, g.ld_seq, P->B, nullptr, g.gen_start};
  if (on) {
    GPT2MI_REQUIRE(g.seq != nullptr, "%s: penalties need seq, the history buffer: it is NULL", what);
    GPT2MI_REQUIRE((long long)max_pos + n - 1 <= GPT2MI_PENALTY_MAX_HISTORY,
                   "%s: max pos0=%d + n=%d - 1 above the history cap %d", what, max_pos, n, GPT2MI_PENALTY_MAX_HISTORY);
  }
  if (g.lp) {
    if (const int rc = gpt2mi::check_logprobs(what, g.lp, V)) return rc;
    GPT2MI_REQUIRE(g.lp->col == nullptr, "%s: logprobs col must be NULL in the loop (step i writes column pos0[b] + i)",
                   what);
    GPT2MI_REQUIRE((long long)max_pos + n <= g.lp->ld, "%s: max pos0=%d + n=%d exceeds the logprobs ld=%d", what, max_pos,
                   n, g.lp->ld);
  }
  bool con_on = false;
  if (g.con) {
    int bias_row[GPT2MI_DECODE_MAX_B];
    if (const int rc = gpt2mi::check_constraints(what, g.con, P->B, V, g.eos, g.done, bias_row, &con_on)) return rc;
    GPT2MI_REQUIRE(g.con->n_stop == 0 || g.seq != nullptr, "%s: stop sequences need seq, the history buffer: it is NULL",
                   what);
  }
  for (int b = 0; b < P->B && g.gen_start && (on || con_on); ++b)
    GPT2MI_REQUIRE(g.gen_start[b] >= 0 && g.gen_start[b] <= g.pos0[b], "%s: gen_start[%d]=%d not in [0, pos0=%d]", what, b,
                   g.gen_start[b], g.pos0[b]);
  GPT2MI_REQUIRE(g.tok != nullptr && P->logits != nullptr, "%s: tok and plan->logits must not be NULL", what);
  if (const int rc = plan_shape(what, P)) return rc;  // (before the first draw, not only before the first step)
  // the sampler entry that takes what is on: a neutral pen or con is not passed on, as that entry would not get it
  const char* draw = con_on ? "sample_constrained" : g.lp ? "sample_logprobs" : "sample_penalized";
  gpt2mi::SampleCall c = {.logits = P->logits, .ldl = P->Vp, .B = P->B, .V = V, .temperature = g.temperature,
                          .top_k = g.top_k, .top_p = g.top_p, .seed = g.seed, .pos = rp.v, .row_id = g.row_id,
                          .eos = g.eos, .done = g.done, .tok_out = g.tok, .seq_out = g.seq, .ld_seq = g.ld_seq,
                          .stream = g.stream, .pen = on || con_on ? &pen : nullptr, .lp = g.lp,
                          .con = con_on ? g.con : nullptr};
  for (int i = 0; i < n; ++i) {
    for (int b = 0; b < P->B; ++b) rp.v[b] = g.pos0[b] + i;
    int rc = gpt2mi::sample_rows(draw, c);
    if (rc) return rc;
    if (i + 1 < n) {
      rc = decode_step_rows(what, P, g.tok, rp.v, g.stream);
      if (rc) return rc;
    }
  }
  return 0;
}
}  // namespace

#define GENERATE_CALL_ARGS                                                                                            \
  .plan = P, .V = V, .temperature = temperature, .top_k = top_k, .top_p = top_p, .seed = seed, .eos = eos, .pos0 = pos0, \
  .row_id = row_id, .n = n, .tok = tok, .seq = seq, .ld_seq = ld_seq, .done = done, .stream = stream
#define GENERATE_CALL_PENALTIES \
  .repetition = repetition, .presence = presence, .frequency = frequency, .gen_start = gen_start

GPT2MI_EXPORT int gpt2mi_decode_generate_ragged(const gpt2mi_decode_plan* P, int V, float temperature, int top_k,
                                                float top_p, uint64_t seed, int64_t eos, const int* pos0,
                                                const uint32_t* row_id, int n, int64_t* tok, int64_t* seq, int ld_seq,
                                                uint8_t* done, void* stream) {
  return decode_generate_rows("decode_generate_ragged", {GENERATE_CALL_ARGS});
}

GPT2MI_EXPORT int gpt2mi_decode_generate_penalized(const gpt2mi_decode_plan* P, int V, float temperature, int top_k,
                                                   float top_p, uint64_t seed, int64_t eos, const int* pos0,
                                                   const uint32_t* row_id, int n, int64_t* tok, int64_t* seq,
                                                   int ld_seq, uint8_t* done, void* stream, float repetition,
                                                   float presence, float frequency, const int* gen_start) {
  return decode_generate_rows("decode_generate_penalized", {GENERATE_CALL_ARGS, GENERATE_CALL_PENALTIES});
}

GPT2MI_EXPORT int gpt2mi_decode_generate_logprobs(const gpt2mi_decode_plan* P, int V, float temperature, int top_k,
                                                  float top_p, uint64_t seed, int64_t eos, const int* pos0,
                                                  const uint32_t* row_id, int n, int64_t* tok, int64_t* seq, int ld_seq,
                                                  uint8_t* done, void* stream, float repetition, float presence,
                                                  float frequency, const int* gen_start, const gpt2mi_logprobs* lp) {
  return decode_generate_rows("decode_generate_logprobs", {GENERATE_CALL_ARGS, GENERATE_CALL_PENALTIES, .lp = lp});
}

GPT2MI_EXPORT int gpt2mi_decode_generate_constrained(const gpt2mi_decode_plan* P, int V, float temperature, int top_k,
                                                     float top_p, uint64_t seed, int64_t eos, const int* pos0,
                                                     const uint32_t* row_id, int n, int64_t* tok, int64_t* seq,
                                                     int ld_seq, uint8_t* done, void* stream, float repetition,
                                                     float presence, float frequency, const int* gen_start,
                                                     const gpt2mi_logprobs* lp, const gpt2mi_constraints* con) {
  return decode_generate_rows("decode_generate_constrained",
                              {GENERATE_CALL_ARGS, GENERATE_CALL_PENALTIES, .lp = lp, .con = con});
}

GPT2MI_EXPORT int gpt2mi_decode_generate(const gpt2mi_decode_plan* P, int V, float temperature, int top_k, float top_p,
                                         uint64_t seed, int64_t eos, int pos, int n, int64_t* tok, int64_t* seq,
                                         int ld_seq, uint8_t* done, void* stream) {
  GPT2MI_REQUIRE(P != nullptr, "decode_generate: plan is NULL");
  GPT2MI_REQUIRE(n >= 0 && pos >= 1, "decode_generate: n=%d must be >= 0 and pos0=%d >= 1 (after a prefill)", n, pos);
  GPT2MI_REQUIRE((long long)pos + n <= P->Tcap, "decode_generate: pos0=%d + n=%d exceeds the cache length Tcap=%d", pos,
                 n, P->Tcap);
  const SamePos same(pos);
  const int* pos0 = same.v;
  const uint32_t* row_id = nullptr;
  return decode_generate_rows("decode_generate", {GENERATE_CALL_ARGS});
}
#undef GENERATE_CALL_ARGS
#undef GENERATE_CALL_PENALTIES
