// Prefill over a live cache: causal flash attention of a chunk of new queries whose keys and values ALL come from the
// key/value cache (bf16 or fp8), gfx950, head_dim 64. The trunk's forward (attention.hip) takes every key from the qkv
// activations of its own call and so cannot see a cache; the decode attention (decode.hip) runs one wave per 32 keys
// and row on the VALU, built for a handful of rows. This kernel serves what lies between: tens to hundreds of rows
// appended to a row that already holds some (DecodeSession.append, a shared prompt prefix).
//
// Key-source rule: the caller has stored the chunk's own keys and values at cache positions base .. base + count - 1
// (gpt2mi_kv_store[_fp8] at t0 = base, an earlier launch on the same stream), so query i reads positions 0 .. base + i
// of its stream and nothing else: with an fp8 cache the chunk's own keys are the quantised ones, as in the step and the
// extend (a token's key has the same bits whoever reads it). Nothing in the cache is written here.
//
// Work split: a workgroup of 4 waves owns (64-query tile, head, sequence, key split); a wave owns 16 queries as one
// MFMA group in the forward's "key on the lane" formulation (S^T = K Q^T with v_mfma_f32_16x16x32_bf16, softmax
// statistics per lane in fp32, P^T from the accumulators in registers, V^T by the transposed LDS read). K and V tiles of
// 64 keys go through LDS as [64][64] bf16 in attention.hip's 16-byte-chunk swizzle, two stages: the next tile's cache
// rows (whole 128-byte lines in bf16, 64 codes and a scale in fp8) are loaded into registers while this tile computes,
// expanded to bf16 (exact for e4m3 * 2^e) and stored to the other stage behind it. Cache access goes through KvBf16 /
// KvFp8 (kv_format.h) alone. Rows of a tile at or above base + count are zeros in LDS and never loaded. Key tiles
// wholly above a wave's last query are skipped wave-uniformly; the tiles that straddle a query's position mask by it.
//
// Key splits: a 64-token chunk at one sequence gives only H workgroups, so the key tiles of a sequence are cut into
// chunk_splits(base + count) contiguous ranges of whole tiles, a function of the sequence's own key count only (its
// output does not depend on what else is in the call). With one split the kernel normalises and writes out itself;
// with more each item writes fp32 (max, sum, acc[64]) per row to the workspace and attn_chunk_combine_kernel merges
// them in range order. No atomics: two runs give the same bits.
//
// (t_off .. store_row64 below repeat attention.hip's LDS and fragment helpers, which live in that unit's unnamed
// namespace: the training kernels' file is left as it is.)
#include <algorithm>

#include "common.h"
#include "gpt2mi.h"
#include "kv_format.h"

// key tiles (of 64) per split, at most 8 splits; an A/B knob (tools/prefix_bench.py measures the product value
// against a library built with a value no sequence reaches, i.e. without splits)
#ifndef GPT2MI_CHUNK_SPLIT_TILES
#define GPT2MI_CHUNK_SPLIT_TILES 4
#endif
GPT2MI_PRODUCT_KNOB(GPT2MI_CHUNK_SPLIT_TILES, 4);

namespace {

constexpr int BKV = 64;           // keys per tile
constexpr int BQ = 64;            // queries per workgroup (16 per wave): the engine's pad unit
constexpr int kTile = BKV * 128;  // bytes of a [64][64] bf16 tile
constexpr int kMaxSplits = 8;
constexpr int kMaxS = GPT2MI_DECODE_MAX_B;
constexpr float kLog2e = 1.4426950408889634f;
// The running max starts here, not at -inf: a row of a later split (or of a skipped wave) may see no key at all, and
// -inf - (-inf) would be NaN. With a finite start exp2(-inf - m) = 0, and the merge weights such a partial by
// exp2(-1e30 - real max) = 0.
constexpr float kMaxInit = -1e30f;

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef short s16x8 __attribute__((ext_vector_type(8)));

__host__ __device__ __forceinline__ int chunk_splits(int keys) {
  const int tiles = (keys + BKV - 1) / BKV;
  const int ns = (tiles + GPT2MI_CHUNK_SPLIT_TILES - 1) / GPT2MI_CHUNK_SPLIT_TILES;
  return ns < 1 ? 1 : (ns > kMaxSplits ? kMaxSplits : ns);
}

__device__ __forceinline__ int t_off(int row, int chunk) { return row * 128 + 16 * (chunk ^ (row & 6)); }
// row read: lane gets tile[row0 + (l&15)][32kk + 8g + 0..7]
__device__ __forceinline__ bf16x8 row_frag(const char* base, int row0, int kk, int lane) {
  return *reinterpret_cast<const bf16x8*>(base + t_off(row0 + (lane & 15), 4 * kk + (lane >> 4)));
}
// permuted transposed read: lane (g, i) gets, for j = 0..7, tile[16*(2kk + (j>>2)) + 4g + (j&3)][c0 + i]
__device__ __forceinline__ bf16x8 tr_frag(const char* base, int kk, int c0, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int chunk = (c0 >> 3) + (p >> 1);
  const int r1 = 32 * kk + 4 * g + q;
  const int r2 = r1 + 16;
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + t_off(r1, chunk) + 8 * (p & 1)));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + t_off(r2, chunk) + 8 * (p & 1)));
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}
// max over the 4 lanes l, l^16, l^32, l^48 (one query's keys in the S^T accumulators)
__device__ __forceinline__ float xor_max(float v) {
  auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
// pack accumulator registers acc[2kk + (j>>2)][j&3] (j = 0..7) to a bf16 operand fragment
__device__ __forceinline__ bf16x8 pack_perm(const f32x4* acc, int kk) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = f2bf(acc[2 * kk + (j >> 2)][j & 3]);
  return r;
}
// one 64-wide output row of a wave's accumulators (v[fd][r] at d = 16fd + 4g + r), scaled and stored as bf16 with two
// 16-byte stores per lane (attention.hip store_row64)
__device__ __forceinline__ void store_row64(bf16* row, const f32x4 (&v)[4], float sc, int lane) {
  const int g = lane >> 4;
#pragma unroll
  for (int pr = 0; pr < 2; ++pr) {
    const bf16x4 a = {f2bf(v[2 * pr][0] * sc), f2bf(v[2 * pr][1] * sc), f2bf(v[2 * pr][2] * sc), f2bf(v[2 * pr][3] * sc)};
    const bf16x4 b = {f2bf(v[2 * pr + 1][0] * sc), f2bf(v[2 * pr + 1][1] * sc), f2bf(v[2 * pr + 1][2] * sc),
                      f2bf(v[2 * pr + 1][3] * sc)};
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 ua = __builtin_bit_cast(u32x2, a), ub = __builtin_bit_cast(u32x2, b);
    const auto x = __builtin_amdgcn_permlane16_swap(ua[0], ub[0], false, false);
    const auto y = __builtin_amdgcn_permlane16_swap(ua[1], ub[1], false, false);
    *reinterpret_cast<u32x4*>(row + 32 * pr + 16 * (g & 1) + 8 * (g >> 1)) = u32x4{x[0], y[0], x[1], y[1]};
  }
}

// The sequences of a call: the host arrays of the C entry, validated there and passed by value (as RowPos / RowMap of
// decode.hip), so a kernel never indexes memory with a number nobody checked. Indexed by blockIdx: scalar loads.
struct ChunkMap {
  int seq[kMaxS], base[kMaxS], count[kMaxS];
};

// The key tiles of query tile qt of a sequence, as the kernel and the merge both see them: the sequence's tiles are cut
// into ns ranges of tps tiles, and query tile qt needs the tiles up to hi (the one that holds its last valid query's
// position).
struct TileRange {
  int ns, tps, hi;
  __device__ __forceinline__ TileRange(int base, int count, int qt) {
    const int kend = base + count, nt = (kend + BKV - 1) / BKV;
    ns = chunk_splits(kend);
    tps = (nt + ns - 1) / ns;
    hi = (base + min(BQ * qt + BQ - 1, count - 1)) / BKV;
  }
};

// Grid (query tiles * nsx, H, S): blockIdx.x = qt * nsx + split, nsx the largest split count of the call.
// ws_ml / ws_acc: per (s, h, row, split) slot (max, sum) and acc[64], the slot stride per row is nsx.
template <class KV>
__global__ __launch_bounds__(256, 2) void attn_chunk_kernel(const bf16* __restrict__ qkv, KV kc, KV vc,
                                                            bf16* __restrict__ out, float* __restrict__ ws_ml,
                                                            float* __restrict__ ws_acc, int H, int Tcap, int T_src,
                                                            int nsx, ChunkMap map) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * kTile];  // 2 stages x (K, V)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4;
  const int s = blockIdx.z, h = blockIdx.y;
  const int qt = blockIdx.x / nsx, sp = blockIdx.x % nsx;
  const int base = map.base[s], count = map.count[s];
  const int C = H * 64;
  const int kend = base + count;  // keys of the sequence; nothing at or above it is read

  // rows of the tile at or above count: zeros, written by the first split's item (32 bytes per thread)
  if (sp == 0) {
    const int r = tid >> 2;
    if (BQ * qt + r >= count) {
      bf16* z = out + ((size_t)s * T_src + BQ * qt + r) * C + h * 64 + 16 * (tid & 3);
      *reinterpret_cast<u32x4*>(z) = u32x4{0u, 0u, 0u, 0u};
      *reinterpret_cast<u32x4*>(z + 8) = u32x4{0u, 0u, 0u, 0u};
    }
  }
  if (BQ * qt >= count) return;  // (block-uniform, as every return ahead of the barriers)
  const TileRange tr(base, count, qt);
  const int t0 = sp * tr.tps;
  if (sp >= tr.ns || t0 > tr.hi) return;
  const int t1 = min(t0 + tr.tps, tr.hi + 1);

  const int i_w = BQ * qt + 16 * w;        // the wave's first query row
  const int i = i_w + (lane & 15);          // the lane's query row, at position base + i
  const bool valid = i < count;
  const bool wave_valid = i_w < count;
  const int p_lo = base + i_w, p_hi = base + min(i_w + 15, count - 1);  // the wave's first / last valid position

  // a pad row's query is never loaded (it may hold anything): zeros, whose scores are finite
  bf16x8 qf[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    qf[kk] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (valid)
      qf[kk] = *reinterpret_cast<const bf16x8*>(qkv + ((size_t)s * T_src + i) * 3 * C + h * 64 + 32 * kk + 8 * g);
  }
  const float sl2 = 0.125f * kLog2e;  // 1/sqrt(64) in log2 units
  float m = kMaxInit;
  // o[4] holds the row sums l = P.1: one more PV-shaped MFMA against a ones operand; every row of it is l
  f32x4 o[5];
#pragma unroll
  for (int f = 0; f < 5; ++f) o[f] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16 one = (bf16)1.f;
  const bf16x8 ones = {one, one, one, one, one, one, one, one};

  // tile loads: thread t holds 16-byte chunk t & 7 of rows (t >> 3) and (t >> 3) + 32 of the K and of the V tile
  const KvLane kl((size_t)map.seq[s] * H + h, Tcap, tid & 7);
  typename KV::Row kr[2], vr[2];
  auto gload = [&](int j) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int key = BKV * j + (tid >> 3) + 32 * u;
      kr[u] = vr[u] = KV::zero();
      if (key < kend) {
        kr[u] = kc.load(kl, key);
        vr[u] = vc.load(kl, key);
      }
    }
  };
  auto sstore = [&](char* stage) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int off = t_off((tid >> 3) + 32 * u, tid & 7);
      *reinterpret_cast<bf16x8*>(stage + off) = KV::tile8(kr[u]);
      *reinterpret_cast<bf16x8*>(stage + kTile + off) = KV::tile8(vr[u]);
    }
  };
  gload(t0);
  sstore(smem);
  __syncthreads();

  for (int j = t0; j < t1; ++j) {
    const int cur = (j - t0) & 1;
    const char* Ks = smem + cur * 2 * kTile;
    const char* Vs = Ks + kTile;
    const int k_lo = j * BKV;
    // the next tile's cache rows into registers, behind this tile's LDS reads
    if (j + 1 < t1) gload(j + 1);
    // wave-uniform: a key of the tile is visible to a valid query of the wave
    if (wave_valid && k_lo <= p_hi) {
      f32x4 sc[4];
#pragma unroll
      for (int fi = 0; fi < 4; ++fi) {
        sc[fi] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          sc[fi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(Ks, 16 * fi, kk, lane), qf[kk], sc[fi], 0, 0, 0);
      }
      if (k_lo + BKV - 1 > p_lo) {  // a tile that straddles a query's position masks by it (wave-uniform branch)
#pragma unroll
        for (int fi = 0; fi < 4; ++fi)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (k_lo + 16 * fi + 4 * g + r > base + i) sc[fi][r] = -INFINITY;
      }
      float lmax = fmaxf(fmaxf(sc[0][0], sc[0][1]), fmaxf(sc[0][2], sc[0][3]));
#pragma unroll
      for (int fi = 1; fi < 4; ++fi) lmax = fmaxf(lmax, fmaxf(fmaxf(sc[fi][0], sc[fi][1]), fmaxf(sc[fi][2], sc[fi][3])));
      const float mn = fmaxf(m, xor_max(lmax) * sl2);  // finite: m starts finite
      const float corr = __builtin_amdgcn_exp2f(m - mn);
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[f][r] *= corr;
      o[4][0] *= corr;  // only row 0 of the row-sum accumulator is read
      m = mn;
#pragma unroll
      for (int fi = 0; fi < 4; ++fi)
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[fi][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[fi][r], sl2, -m));  // masked: 0
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const bf16x8 p = pack_perm(sc, kk);  // the row sum and P.V read the same bf16 probabilities
        o[4] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, p, o[4], 0, 0, 0);
#pragma unroll
        for (int fd = 0; fd < 4; ++fd)
          o[fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(Vs, kk, 16 * fd, lane), p, o[fd], 0, 0, 0);
      }
    }
    // the other stage was last read in tile j - 1, released by that tile's barrier
    if (j + 1 < t1) sstore(smem + (cur ^ 1) * 2 * kTile);
    __syncthreads();
  }
  // rows at or above count were zeroed above. (The lane swaps of store_row64 pair lanes l and l ^ 16, which hold the
  // same query: a row's four lanes stay or leave together.)
  if (!valid) return;

  const f32x4 ov[4] = {o[0], o[1], o[2], o[3]};
  if (tr.ns == 1) {  // the only split: normalise and write the row
    store_row64(out + ((size_t)s * T_src + i) * C + h * 64, ov, 1.f / o[4][0], lane);
    return;
  }
  const size_t slot = (((size_t)s * H + h) * T_src + i) * nsx + sp;
#pragma unroll
  for (int fd = 0; fd < 4; ++fd) *reinterpret_cast<f32x4*>(ws_acc + slot * 64 + 16 * fd + 4 * g) = ov[fd];
  if (g == 0) {
    ws_ml[2 * slot] = m;  // log2 units
    ws_ml[2 * slot + 1] = o[4][0];
  }
}

// out[s, i, h*64 + d] = sum_r 2^(m_r - m) acc_r[d] / sum_r 2^(m_r - m) l_r over the splits r that hold a tile of row
// i's query tile, in range order; lane d, grid (rows, H, S). Sequences of one split wrote out themselves.
__global__ __launch_bounds__(64) void attn_chunk_combine_kernel(const float* __restrict__ ws_ml,
                                                                const float* __restrict__ ws_acc,
                                                                bf16* __restrict__ out, int H, int T_src, int nsx,
                                                                ChunkMap map) {
  const int d = threadIdx.x, i = blockIdx.x, h = blockIdx.y, s = blockIdx.z;
  const int base = map.base[s], count = map.count[s];
  if (i >= count) return;
  const TileRange tr(base, count, i / BQ);
  if (tr.ns == 1) return;
  const int nr = tr.hi / tr.tps + 1;  // (<= ns: hi is below the sequence's tile count)
  const size_t slot0 = (((size_t)s * H + h) * T_src + i) * nsx;
  float m = kMaxInit;
  for (int r = 0; r < nr; ++r) m = fmaxf(m, ws_ml[2 * (slot0 + r)]);
  float l = 0.f, o = 0.f;
  for (int r = 0; r < nr; ++r) {
    const float wgt = __builtin_amdgcn_exp2f(ws_ml[2 * (slot0 + r)] - m);
    l = __builtin_fmaf(wgt, ws_ml[2 * (slot0 + r) + 1], l);
    o = __builtin_fmaf(wgt, ws_acc[(slot0 + r) * 64 + d], o);
  }
  out[((size_t)s * T_src + i) * H * 64 + h * 64 + d] = f2bf(o / l);
}

// x[s, t, :] = wte[idx[s, t], :] + wpe[pos0[s] + t, :] for t < T_valid, zeros above (the padding to the attention
// tile, where neither table is read): gpt2mi_embed_fwd at p = 0 with a sequence's positions starting at pos0[s].
// One thread per 4 floats, grid (C / 1024, T, S).
struct ChunkPos {
  int v[kMaxS];
};
__global__ __launch_bounds__(256) void embed_fwd_at_kernel(const int64_t* __restrict__ idx, const float* __restrict__ wte,
                                                           const float* __restrict__ wpe, float* __restrict__ x, int T,
                                                           int T_valid, int C, ChunkPos pos0) {
  const int c = 4 * (blockIdx.x * 256 + threadIdx.x), t = blockIdx.y, s = blockIdx.z;
  if (c >= C) return;
  const size_t row = (size_t)s * T + t;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (t < T_valid)
    v = *reinterpret_cast<const f32x4*>(wte + (size_t)idx[row] * C + c) +
        *reinterpret_cast<const f32x4*>(wpe + (size_t)(pos0.v[s] + t) * C + c);
  *reinterpret_cast<f32x4*>(x + row * C + c) = v;
}

struct ChunkCache {
  bool fp8;
  void *k, *v;
  float *ks, *vs;
};

int attn_chunk_rows(const char* what, const uint16_t* qkv, const ChunkCache& kv, uint16_t* out, float* workspace,
                    size_t workspace_floats, int S, int B, int H, int head_dim, int Tcap, int T_src, const int* seq,
                    const int* base, const int* count, void* stream) {
  GPT2MI_REQUIRE(head_dim == 64, "%s: head_dim=%d (the decode kernels implement 64)", what, head_dim);
  GPT2MI_REQUIRE(B >= 1 && H >= 1 && H <= 65535 && Tcap >= 1, "%s: B=%d, H=%d (<= 65535), Tcap=%d must be positive", what,
                 B, H, Tcap);
  GPT2MI_REQUIRE(S >= 1 && S <= kMaxS, "%s: S=%d not in [1, %d]", what, S, kMaxS);
  GPT2MI_REQUIRE(T_src >= BQ && T_src % BQ == 0, "%s: T_src=%d must be a positive multiple of %d", what, T_src, BQ);
  GPT2MI_REQUIRE(seq && base && count, "%s: seq, base and count (host, S ints each) must not be NULL", what);
  ChunkMap map{};
  int nsx = 1;
  for (int s = 0; s < S; ++s) {
    GPT2MI_REQUIRE(seq[s] >= 0 && seq[s] < B, "%s: seq[%d]=%d not in [0, B=%d)", what, s, seq[s], B);
    GPT2MI_REQUIRE(s == 0 || seq[s] > seq[s - 1], "%s: seq[%d]=%d after seq[%d]=%d: the sequences must increase", what, s,
                   seq[s], s - 1, s ? seq[s - 1] : 0);
    GPT2MI_REQUIRE(count[s] >= 1 && count[s] <= T_src, "%s: count[%d]=%d not in [1, T_src=%d]", what, s, count[s], T_src);
    GPT2MI_REQUIRE(base[s] >= 0 && (long long)base[s] + count[s] <= Tcap,
                   "%s: base[%d]=%d + count[%d]=%d not in [0, Tcap=%d]", what, s, base[s], s, count[s], Tcap);
    map.seq[s] = seq[s], map.base[s] = base[s], map.count[s] = count[s];
    nsx = std::max(nsx, chunk_splits(base[s] + count[s]));
  }
  const size_t need = nsx > 1 ? (size_t)S * H * T_src * nsx * 66 : 0;  // (max, sum) + acc[64] per (row, split)
  GPT2MI_REQUIRE(workspace_floats >= need, "%s: workspace too small (%zu floats given, %zu needed for %d key splits)",
                 what, workspace_floats, need, nsx);
  GPT2MI_REQUIRE(!kv.fp8 || (kv.ks && kv.vs), "%s: kscale and vscale of the fp8 cache must not be NULL", what);
  GPT2MI_REQUIRE(qkv && kv.k && kv.v && out && (need == 0 || workspace),
                 "%s: qkv, the caches, out and a needed workspace must not be NULL", what);
  GPT2MI_REQUIRE((long long)(T_src / BQ) * nsx <= 0x7fffffffLL, "%s: T_src=%d is too long", what, T_src);
  hipStream_t st = (hipStream_t)stream;
  float* ws_ml = workspace;
  float* ws_acc = need ? workspace + (size_t)S * H * T_src * nsx * 2 : nullptr;
  const dim3 grid(T_src / BQ * nsx, H, S);
  if (kv.fp8)
    attn_chunk_kernel<<<grid, 256, 0, st>>>((const bf16*)qkv, KvFp8{(uint8_t*)kv.k, kv.ks}, KvFp8{(uint8_t*)kv.v, kv.vs},
                                            (bf16*)out, ws_ml, ws_acc, H, Tcap, T_src, nsx, map);
  else
    attn_chunk_kernel<<<grid, 256, 0, st>>>((const bf16*)qkv, KvBf16{(bf16*)kv.k}, KvBf16{(bf16*)kv.v}, (bf16*)out,
                                            ws_ml, ws_acc, H, Tcap, T_src, nsx, map);
  if (const int rc = gpt2mi::check_launch(what)) return rc;
  if (nsx == 1) return 0;
  int rows = 0;
  for (int s = 0; s < S; ++s) rows = std::max(rows, count[s]);
  attn_chunk_combine_kernel<<<dim3(rows, H, S), 64, 0, st>>>(ws_ml, ws_acc, (bf16*)out, H, T_src, nsx, map);
  return gpt2mi::check_launch(what);
}

}  // namespace

GPT2MI_EXPORT int gpt2mi_attn_chunk_splits(int keys) { return keys < 1 ? 0 : chunk_splits(keys); }

GPT2MI_EXPORT size_t gpt2mi_attn_chunk_workspace(int S, int H, int Tcap, int T_src) {
  if (S < 1 || H < 1 || Tcap < 1 || T_src < 1) return 0;
  const int ns = chunk_splits(Tcap);
  return ns > 1 ? (size_t)S * H * T_src * ns * 66 : 0;
}

GPT2MI_EXPORT int gpt2mi_attn_chunk(const uint16_t* qkv, const uint16_t* kcache, const uint16_t* vcache, uint16_t* out,
                                    float* workspace, size_t workspace_floats, int S, int B, int H, int head_dim,
                                    int Tcap, int T_src, const int* seq, const int* base, const int* count,
                                    void* stream) {
  return attn_chunk_rows("attn_chunk", qkv, ChunkCache{false, (void*)kcache, (void*)vcache, nullptr, nullptr}, out,
                         workspace, workspace_floats, S, B, H, head_dim, Tcap, T_src, seq, base, count, stream);
}

GPT2MI_EXPORT int gpt2mi_attn_chunk_fp8(const uint16_t* qkv, const uint8_t* kcache, const uint8_t* vcache,
                                        const float* kscale, const float* vscale, uint16_t* out, float* workspace,
                                        size_t workspace_floats, int S, int B, int H, int head_dim, int Tcap, int T_src,
                                        const int* seq, const int* base, const int* count, void* stream) {
  return attn_chunk_rows("attn_chunk_fp8", qkv,
                         ChunkCache{true, (void*)kcache, (void*)vcache, (float*)kscale, (float*)vscale}, out, workspace,
                         workspace_floats, S, B, H, head_dim, Tcap, T_src, seq, base, count, stream);
}

GPT2MI_EXPORT int gpt2mi_embed_fwd_at(const int64_t* idx, const float* wte, const float* wpe, float* x, int S, int T,
                                      int T_valid, int C, const int* pos0, void* stream) {
  GPT2MI_REQUIRE(S >= 1 && S <= kMaxS, "embed_fwd_at: S=%d not in [1, %d]", S, kMaxS);
  GPT2MI_REQUIRE(C >= 4 && C % 4 == 0, "embed_fwd_at: C=%d must be a positive multiple of 4", C);
  GPT2MI_REQUIRE(T >= 1 && T <= 65535 && T_valid >= 1 && T_valid <= T, "embed_fwd_at: T_valid=%d not in [1, T=%d <= 65535]",
                 T_valid, T);
  GPT2MI_REQUIRE(pos0 != nullptr, "embed_fwd_at: pos0 (host, S ints) is NULL");
  ChunkPos p{};
  for (int s = 0; s < S; ++s) {
    GPT2MI_REQUIRE(pos0[s] >= 0, "embed_fwd_at: pos0[%d]=%d is negative", s, pos0[s]);
    p.v[s] = pos0[s];
  }
  GPT2MI_REQUIRE(idx && wte && wpe && x, "embed_fwd_at: idx, wte, wpe and x must not be NULL");
  embed_fwd_at_kernel<<<dim3((C / 4 + 255) / 256, T, S), 256, 0, (hipStream_t)stream>>>(idx, wte, wpe, x, T, T_valid, C, p);
  return gpt2mi::check_launch("embed_fwd_at");
}
