// The deterministic mode's backward kernels. gfx950, wave64.
//
// Every float atomicAdd that the whole-model backward reaches has a replacement here that adds in an order fixed by the
// inputs: bias-gradient column sums (two stages through a partials table), the LayerNorm backward's column sums (the
// row body of csrc/norm_embed.hip with its flush redirected to a partials table, then the same second stage) and the
// token-table gradient of the embedding backward (sort the (token, row) pairs, sum runs of equal tokens chunk by
// chunk, join the runs that cross chunks). Raw pointers, a stream and a caller-supplied workspace
// (gpt2mi_det_workspace_bytes); no float atomics, no host synchronisation, nothing read back.
#include <algorithm>

#include "common.h"

namespace {

// ---- the second stage of every column sum ----------------------------------------------------------------------
// dst[c] += sum_{i < n} part[i * stride + c]. A block owns kFoldCols columns; its kFoldSubs thread rows each add a
// contiguous share of the n partials in index order, kFoldLoads loads in flight; the shares meet in LDS and are added
// in share order. The order depends on n alone. blockIdx.y picks one of up to three (partials slot, destination) pairs
// (the LayerNorm backward's dw, db, dbias_out); a null destination has nothing to do.
constexpr int kFoldCols = 32, kFoldSubs = 8, kFoldLoads = 8;

__global__ __launch_bounds__(256) void fold_kernel(const float* __restrict__ part, int n, size_t stride, size_t slot,
                                                   float* __restrict__ d0, float* __restrict__ d1,
                                                   float* __restrict__ d2, int N) {
  float* dst = blockIdx.y == 0 ? d0 : blockIdx.y == 1 ? d1 : d2;
  if (!dst) return;
  const int x = threadIdx.x % kFoldCols, sub = threadIdx.x / kFoldCols;
  const int c = blockIdx.x * kFoldCols + x;
  const int q = (n + kFoldSubs - 1) / kFoldSubs;
  const int i1 = min(n, (sub + 1) * q);
  float s = 0.f;
  if (c < N) {
    const float* p = part + blockIdx.y * slot + c;
    int i = sub * q;
    for (; i + kFoldLoads <= i1; i += kFoldLoads) {
      float v[kFoldLoads];
#pragma unroll
      for (int u = 0; u < kFoldLoads; ++u) v[u] = p[(size_t)(i + u) * stride];
#pragma unroll
      for (int u = 0; u < kFoldLoads; ++u) s += v[u];
    }
    for (; i < i1; ++i) s += p[(size_t)i * stride];
  }
  __shared__ float red[kFoldSubs][kFoldCols];
  red[sub][x] = s;
  __syncthreads();
  if (sub == 0 && c < N) {
    float t = red[0][x];
#pragma unroll
    for (int k = 1; k < kFoldSubs; ++k) t += red[k][x];
    dst[c] += t;
  }
}

void fold(const float* part, int n, size_t stride, size_t slot, float* d0, float* d1, float* d2, int N, int dsts,
          hipStream_t s) {
  fold_kernel<<<dim3((N + kFoldCols - 1) / kFoldCols, dsts), 256, 0, s>>>(part, n, stride, slot, d0, d1, d2, N);
}

// ---- a. ordered column sums --------------------------------------------------------------------------------------
// Stage one is colsum_kernel's walk (csrc/norm_embed.hip): a thread owns 4 adjacent columns, blockIdx.y a chunk of
// rows_per_block rows, four row groups per block that meet in LDS. The block's 256 sums are stored to part[chunk][N].
__device__ __forceinline__ f32x4 load4(const bf16* p) {
  const bf16x4 t = *reinterpret_cast<const bf16x4*>(p);
  return f32x4{bf2f(t[0]), bf2f(t[1]), bf2f(t[2]), bf2f(t[3])};
}
__device__ __forceinline__ f32x4 load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

template <typename TG>
__global__ __launch_bounds__(256) void colsum_part_kernel(const TG* __restrict__ g, float* __restrict__ part, int M,
                                                          int N, int ld, int rows_per_block) {
  const int col4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
  const int sub = threadIdx.x >> 6;
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = min(M, r0 + rows_per_block);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (col4 < N)
    for (int r = r0 + sub; r < r1; r += 4) s += load4(g + (size_t)r * ld + col4);
  __shared__ float red[4][256];
#pragma unroll
  for (int j = 0; j < 4; ++j) red[sub][(threadIdx.x & 63) * 4 + j] = s[j];
  __syncthreads();
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < N)
    part[(size_t)blockIdx.y * N + c] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// rows per chunk: a function of (M, N) only (about 1024 blocks, 8..256 rows each, as gpt2mi_colsum_*)
int colsum_rows(int M, int N) {
  const int gx = (N + 255) / 256;
  const int want_y = (1024 + gx - 1) / gx;
  return std::max(8, std::min(256, (M + want_y - 1) / want_y));
}
// an upper bound of chunks * N floats for any M' <= M, N' <= N: a chunk count is at most 1024 / gx + 2 when the rows
// per chunk follow M', and at most M' / 256 + 1 when they are capped at 256
size_t colsum_floats(size_t M, size_t N) {
  return 1024 * 256 + 512 * ((N + 255) / 256) + (M / 256 + 1) * N;
}

// ---- c. ordered token-table gradient -------------------------------------------------------------------------------
// Keys (token << 32) | row of the n = B * T_valid valid rows, row = b * T + t; sorted, a token's rows are adjacent and
// ascend. The keys are unique, so the sorted sequence does not depend on how it is reached.
constexpr int kSortN = 2048;  // keys per block of the LDS sort (16 KB)
constexpr uint64_t kPadKey = ~0ull;

// Forms the keys of [2048 k, 2048 (k + 1)), pad keys past n, and sorts them in LDS (bitonic, 4 compare-exchanges per
// thread and step).
__global__ __launch_bounds__(256) void embed_sort_kernel(const int64_t* __restrict__ idx, uint64_t* __restrict__ keys,
                                                         int n, int T, int T_valid) {
  __shared__ uint64_t k[kSortN];
  const int base = blockIdx.x * kSortN;
#pragma unroll
  for (int u = 0; u < kSortN / 256; ++u) {
    const int i = base + u * 256 + threadIdx.x;
    uint64_t key = kPadKey;
    if (i < n) {
      const int b = i / T_valid;
      const uint32_t row = (uint32_t)(b * T + (i - b * T_valid));
      key = ((uint64_t)(uint32_t)idx[row] << 32) | row;
    }
    k[u * 256 + threadIdx.x] = key;
  }
  __syncthreads();
  for (int size = 2; size <= kSortN; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
      for (int u = 0; u < kSortN / 512; ++u) {
        const int pid = u * 256 + threadIdx.x;
        const int i = 2 * pid - (pid & (stride - 1)), j = i + stride;
        const uint64_t a = k[i], b = k[j];
        if ((a > b) == ((i & size) == 0)) {
          k[i] = b;
          k[j] = a;
        }
      }
      __syncthreads();
    }
#pragma unroll
  for (int u = 0; u < kSortN / 256; ++u) keys[base + u * 256 + threadIdx.x] = k[u * 256 + threadIdx.x];
}

// One merge pass over sorted runs of `run` keys: a key goes to its index in its own run plus the number of keys of the
// partner run that precede it (binary search; the left run's keys precede equal keys of the right one, which only pad
// keys are). A last run without a partner is copied.
__global__ __launch_bounds__(256) void embed_merge_kernel(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst,
                                                          int npad, int run) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npad) return;
  const int r = i / run, rs = r * run, ps = (r ^ 1) * run;
  const uint64_t key = src[i];
  if (ps >= npad) {
    dst[i] = key;
    return;
  }
  const bool left = (r & 1) == 0;
  int lo = 0, hi = min(run, npad - ps);
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const uint64_t v = src[ps + mid];
    if (left ? v < key : v <= key) lo = mid + 1;
    else hi = mid;
  }
  dst[min(rs, ps) + (i - rs) + lo] = key;
}

// The chunked segmented sum. The sorted list is cut into chunks of kSegChunk entries; a wave takes a chunk and a slab
// of 64 * kSegCh channels (blockIdx.y), a lane owning channels lane + 64 k, so the work follows the occurrences, not
// the vocabulary: a token that fills thousands of entries is spread over as many waves. The wave walks its chunk in
// order, kSegGroup rows' loads in flight, the dropout decision hashed once per element, s += drop(dres[row, c]). When
// the token changes, the finished run goes
//   - to part[chunk][0][C] if it is the chunk's first run (it may continue the previous chunk's last run),
//   - to dwte[token, c] += s otherwise: the run lies inside the chunk, and no other wave touches these channels of
//     that row;
// and at the end the last run goes to part[chunk][1][C] (it may continue in the next chunk), or to part[chunk][0] if
// it is also the first. embed_fix_kernel joins them.
constexpr int kSegChunk = 32, kSegCh = 4, kSegGroup = 8;

__global__ __launch_bounds__(256) void embed_seg_kernel(const uint64_t* __restrict__ keys,
                                                        const float* __restrict__ dres, float* __restrict__ dwte,
                                                        float* __restrict__ part, int n, int C, uint64_t seed,
                                                        uint32_t thr, float inv_keep) {
  const int lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int e0 = chunk * kSegChunk;
  if (e0 >= n) return;  // (no barrier below: waves are independent)
  const int cnt = min(kSegChunk, n - e0);
  const int c0 = blockIdx.y * (64 * kSegCh) + lane;
  const uint64_t mine = lane < cnt ? keys[e0 + lane] : 0;
  const int my_tok = (int)(uint32_t)(mine >> 32), my_row = (int)(uint32_t)mine;
  float* head = part + (size_t)chunk * 2 * C;
  float s[kSegCh];
#pragma unroll
  for (int k = 0; k < kSegCh; ++k) s[k] = 0.f;
  uint32_t cur = (uint32_t)__shfl(my_tok, 0, 64);
  bool first = true;  // the running run is the chunk's first

  auto flush = [&](bool last) {
    if (first || last) {
      float* dst = first ? head : head + C;
#pragma unroll
      for (int k = 0; k < kSegCh; ++k)
        if (c0 + 64 * k < C) dst[c0 + 64 * k] = s[k];
    } else {
      float* dst = dwte + (size_t)cur * C;
#pragma unroll
      for (int k = 0; k < kSegCh; ++k)
        if (c0 + 64 * k < C) dst[c0 + 64 * k] += s[k];
    }
  };

  for (int j = 0; j < cnt; j += kSegGroup) {
    float g[kSegGroup][kSegCh];
    uint32_t tok[kSegGroup], row[kSegGroup];
#pragma unroll
    for (int u = 0; u < kSegGroup; ++u) {  // the group's loads first
      tok[u] = (uint32_t)__shfl(my_tok, j + u, 64);
      row[u] = (uint32_t)__shfl(my_row, j + u, 64);
#pragma unroll
      for (int k = 0; k < kSegCh; ++k)
        g[u][k] = (j + u < cnt && c0 + 64 * k < C) ? dres[(size_t)row[u] * C + c0 + 64 * k] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kSegGroup; ++u) {
      if (j + u >= cnt) break;
      if (tok[u] != cur) {
        flush(false);
        first = false;
        cur = tok[u];
#pragma unroll
        for (int k = 0; k < kSegCh; ++k) s[k] = 0.f;
      }
#pragma unroll
      for (int k = 0; k < kSegCh; ++k) {
        float v = g[u][k];
        if (thr) v = drop_keep(seed, (uint64_t)row[u] * C + c0 + 64 * k, thr) ? v * inv_keep : 0.f;
        s[k] += v;
      }
    }
  }
  flush(true);
}

// The fix-up. The chunks' boundary partials, read in the order head(0), tail(0), head(1), tail(1), ..., fall into
// groups of one token each: a group starts at head(k) when chunk k starts with a new token, or at tail(k) (a chunk
// has a tail when its last token differs from its first), and goes on through head(k + 1) .. head(last), the chunk
// that holds the token's last entry (found by a binary search of the sorted keys). The block of the group's first
// chunk adds the group in that order, a thread per channel, eight loads in flight, and does the one dwte[token, c] +=.
__global__ __launch_bounds__(256) void embed_fix_kernel(const uint64_t* __restrict__ keys,
                                                        const float* __restrict__ part, float* __restrict__ dwte,
                                                        int n, int C) {
  const int chunk = blockIdx.x;
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= C) return;
  const int e0 = chunk * kSegChunk, e1 = min(n, e0 + kSegChunk) - 1;
  const uint32_t htok = (uint32_t)(keys[e0] >> 32), ltok = (uint32_t)(keys[e1] >> 32);
  auto group = [&](uint32_t tok, const float* begin) {
    int lo = e1 + 1, hi = n;  // the first entry past e1 whose token is larger
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((uint32_t)(keys[mid] >> 32) > tok) hi = mid;
      else lo = mid + 1;
    }
    const int last = (lo - 1) / kSegChunk;
    float s = begin[c];
    const float* p = part + c;
    int j = chunk + 1;
    for (; j + 8 <= last + 1; j += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(j + u) * 2 * C];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; j <= last; ++j) s += p[(size_t)j * 2 * C];
    dwte[(size_t)tok * C + c] += s;
  };
  const float* head = part + (size_t)chunk * 2 * C;
  if (chunk == 0 || (uint32_t)(keys[e0 - 1] >> 32) != htok) group(htok, head);
  if (ltok != htok) group(ltok, head + C);
}

// dwpe of the absolute-position form: embed_bwd_kernel's walk (csrc/norm_embed.hip) without its token-table atomics,
// one thread per (t, c) over the batch in batch order, so the same bits. The product is rounded on its own as there
// (where the atomic needs it): no fused multiply-add into the sum.
__global__ __launch_bounds__(256) void embed_wpe_kernel(const float* __restrict__ dres, float* __restrict__ dwpe,
                                                        int B, int T, int T_valid, int C, uint64_t seed, uint32_t thr,
                                                        float inv_keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T_valid * C) return;
  const int t = i / C, c = i % C;
  float s = 0.f;
  auto one = [&](int b, float g) {
    const size_t row = (size_t)b * T + t;
    if (thr) g = drop_keep(seed, row * C + c, thr) ? __fmul_rn(g, inv_keep) : 0.f;
    s += g;
  };
  int b = 0;
  for (; b + 4 <= B; b += 4) {
    float g[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) g[u] = dres[((size_t)(b + u) * T + t) * C + c];
#pragma unroll
    for (int u = 0; u < 4; ++u) one(b + u, g[u]);
  }
  for (; b < B; ++b) one(b, dres[((size_t)b * T + t) * C + c]);
  dwpe[i] += s;
}

size_t round_up(size_t a, size_t b) { return (a + b - 1) / b * b; }

// workspace of the token-table gradient for n rows: two key arrays of n rounded up to the block sort, then the
// boundary partials [chunks][2][C]
size_t embed_key_bytes(size_t n) { return 2 * round_up(n, kSortN) * sizeof(uint64_t); }
size_t embed_bytes(size_t n, size_t C) {
  return embed_key_bytes(n) + (n + kSegChunk - 1) / kSegChunk * 2 * C * sizeof(float);
}

int embed_dwte(const char* what, const int64_t* idx, const float* dres, float* dwte, int B, int T, int T_valid, int C,
               float p, uint64_t seed, void* workspace, hipStream_t s) {
  GPT2MI_REQUIRE(workspace != nullptr, "%s: workspace is null", what);
  GPT2MI_REQUIRE(T_valid > 0 && T_valid <= T, "%s: T_valid=%d not in [1, T=%d]", what, T_valid, T);
  GPT2MI_REQUIRE(B > 0 && C > 0 && (size_t)B * T < (1ull << 31), "%s: B=%d, T=%d, C=%d out of range", what, B, T, C);
  GPT2MI_REQUIRE(p <= 0.f || (size_t)B * T * C < (1ull << 33), "%s: B*T*C exceeds the 32-bit dropout pair index", what);
  const int n = B * T_valid;
  const int npad = (int)round_up(n, kSortN);
  uint64_t* a = (uint64_t*)workspace;
  uint64_t* b = a + npad;
  float* part = (float*)((char*)workspace + embed_key_bytes(n));
  embed_sort_kernel<<<npad / kSortN, 256, 0, s>>>(idx, a, n, T, T_valid);
  for (int64_t run = kSortN; run < npad; run *= 2) {
    embed_merge_kernel<<<npad / 256, 256, 0, s>>>(a, b, npad, (int)run);
    std::swap(a, b);
  }
  const uint32_t thr = drop_threshold(p);
  const float ik = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const int chunks = (n + kSegChunk - 1) / kSegChunk;
  const int slabs = (C + 64 * kSegCh - 1) / (64 * kSegCh);
  embed_seg_kernel<<<dim3((chunks + 3) / 4, slabs), 256, 0, s>>>(a, dres, dwte, part, n, C, seed, thr, ik);
  embed_fix_kernel<<<dim3(chunks, (C + 255) / 256), 256, 0, s>>>(a, part, dwte, n, C);
  return 0;
}

template <typename TG>
int colsum_det_t(const TG* g, float* db, int M, int N, int ld, void* workspace, void* stream) {
  GPT2MI_REQUIRE(workspace != nullptr, "colsum_det: workspace is null");
  GPT2MI_REQUIRE(M > 0 && N > 0 && N % 4 == 0 && ld % 4 == 0 && ld >= N,
                 "colsum_det: M=%d, N=%d, ld=%d (N and ld multiples of 4, ld >= N)", M, N, ld);
  hipStream_t s = (hipStream_t)stream;
  const int rpb = colsum_rows(M, N);
  const int chunks = (M + rpb - 1) / rpb;
  float* part = (float*)workspace;
  colsum_part_kernel<TG><<<dim3((N + 255) / 256, chunks), 256, 0, s>>>(g, part, M, N, ld, rpb);
  fold(part, chunks, N, 0, db, nullptr, nullptr, N, 1, s);
  return gpt2mi::check_launch("colsum_det");
}

int layernorm_bwd_det_t(int f32, const float* x, const float* w, const float* mean, const float* rstd, const void* dy,
                        float* dres, float* dw, float* db, void* out, float* dbias_out, int M, int C, float p_out,
                        uint64_t seed_out, int dres_init, void* workspace, void* stream) {
  GPT2MI_REQUIRE(workspace != nullptr, "layernorm_bwd_det: workspace is null");
  GPT2MI_REQUIRE(M > 0, "layernorm_bwd_det: M=%d", M);
  float* part = (float*)workspace;
  int blocks = 0;
  const bool emit = dbias_out && out;
  const int rc = gpt2mi::layernorm_bwd_partials(f32, x, w, mean, rstd, dy, dres, dw != nullptr, db != nullptr, out,
                                                dbias_out != nullptr, M, C, p_out, seed_out, dres_init, part, &blocks,
                                                stream);
  if (rc) return rc;
  fold(part, blocks, (size_t)3 * C, C, dw, db, emit ? dbias_out : nullptr, C, 3, (hipStream_t)stream);
  return gpt2mi::check_launch("layernorm_bwd_det");
}

}  // namespace

GPT2MI_EXPORT size_t gpt2mi_det_workspace_bytes(int B, int T, int C, int Nmax) {
  if (B <= 0 || T <= 0 || C <= 0 || Nmax <= 0) return 0;
  const size_t M = (size_t)B * T;
  const size_t col = colsum_floats(M, (size_t)std::max(Nmax, C)) * sizeof(float);
  const size_t ln = (size_t)512 * 3 * C * sizeof(float);
  return round_up(std::max(std::max(col, ln), embed_bytes(M, C)), 256);
}

GPT2MI_EXPORT int gpt2mi_colsum_det_bf16(const uint16_t* g, float* db, int M, int N, int ld, void* workspace,
                                         void* stream) {
  return colsum_det_t<bf16>((const bf16*)g, db, M, N, ld, workspace, stream);
}

GPT2MI_EXPORT int gpt2mi_colsum_det_f32(const float* g, float* db, int M, int N, int ld, void* workspace,
                                        void* stream) {
  return colsum_det_t<float>(g, db, M, N, ld, workspace, stream);
}

GPT2MI_EXPORT int gpt2mi_layernorm_bwd_det(const float* x, const float* w, const float* mean, const float* rstd,
                                           const uint16_t* dy, float* dres, float* dw, float* db, uint16_t* out_bf16,
                                           float* dbias_out, int M, int C, float p_out, uint64_t seed_out,
                                           int dres_init, void* workspace, void* stream) {
  return layernorm_bwd_det_t(0, x, w, mean, rstd, dy, dres, dw, db, out_bf16, dbias_out, M, C, p_out, seed_out,
                             dres_init, workspace, stream);
}

GPT2MI_EXPORT int gpt2mi_layernorm_bwd_det_f32(const float* x, const float* w, const float* mean, const float* rstd,
                                               const float* dy, float* dres, float* dw, float* db, float* out_f32,
                                               float* dbias_out, int M, int C, float p_out, uint64_t seed_out,
                                               int dres_init, void* workspace, void* stream) {
  return layernorm_bwd_det_t(1, x, w, mean, rstd, dy, dres, dw, db, out_f32, dbias_out, M, C, p_out, seed_out,
                             dres_init, workspace, stream);
}

GPT2MI_EXPORT int gpt2mi_embed_bwd_det(const int64_t* idx, const float* dres, float* dwte, float* dwpe, int B, int T,
                                       int T_valid, int C, float p, uint64_t seed, void* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int rc = embed_dwte("embed_bwd_det", idx, dres, dwte, B, T, T_valid, C, p, seed, workspace, s);
  if (rc) return rc;
  embed_wpe_kernel<<<(T_valid * C + 255) / 256, 256, 0, s>>>(dres, dwpe, B, T, T_valid, C, seed, drop_threshold(p),
                                                            p > 0.f ? 1.f / (1.f - p) : 1.f);
  return gpt2mi::check_launch("embed_bwd_det");
}

GPT2MI_EXPORT int gpt2mi_embed_bwd_doc_det(const int64_t* idx, const float* dres, float* dwte, float* dwpe,
                                           const int* start, int B, int T, int T_valid, int C, float p, uint64_t seed,
                                           void* workspace, void* stream) {
  GPT2MI_REQUIRE(start != nullptr, "embed_bwd_doc_det: start is null");
  const int rc = embed_dwte("embed_bwd_doc_det", idx, dres, dwte, B, T, T_valid, C, p, seed, workspace,
                            (hipStream_t)stream);
  if (rc) return rc;
  return gpt2mi::embed_bwd_doc_wpe(dres, start, dwpe, B, T, T_valid, C, p, seed, stream);
}
