// Fused tied-lm_head + cross-entropy forward for evaluation (gpt2mi_lm_loss): the loss rows of
// F.cross_entropy(x @ w[:V].T, labels) without the [M, V] logits ever leaving the registers.
//
// Kernel 1 (lm_loss_partial_kernel): grid = row panels x vocabulary splits. A workgroup owns 128 rows of x and a
// contiguous range of 128-column vocabulary tiles. Per tile it runs gemm.hip's 128x128 bf16 MFMA K-loop (256 threads =
// 2x2 waves, BK = 64, register-staged double buffer, the same swizzled k-contiguous LDS images); the loop is flat over
// (tile, K-tile) pairs, so the first operand tiles of the next vocabulary tile are already in flight while the last
// MFMAs of this one run. The x panel is re-read per vocabulary tile (from L2). When a tile's accumulators are complete
// they are folded, in registers, into a running (max, sum of exp) that every LANE keeps for each of its 16 rows over
// the columns that lane owns (column = lane & 15 mod 16): no cross-lane traffic per tile, one exp per logit plus one
// rescale per row. The logit at a row's label is stored by the one lane of the one workgroup that holds it. At the end
// of the range the 16 column lanes are merged by shuffles, the two column waves through LDS, and the workgroup writes
// one (max, sum) per row to workspace[split][row].
// Kernel 2 (lm_loss_finish_kernel, one workgroup): merges the splits of every row in split order, writes loss_rows /
// lse and reduces the sum and the count in a fixed order. No float atomics: two calls give the same bits.
// Columns >= V are masked to -inf in the (only) tile that holds them, whatever w holds there; rows of w at or past
// w_rows and rows of x at or past M are never read (the loaders clamp the row).
#include "common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int kThreads = 256;
constexpr int kStageBytes = (BM + BN) * BK * 2;  // 32 KiB
constexpr int kLdsBytes = 2 * kStageBytes;
// "no column seen yet": finite, so merging two empty states forms exp(0) * 0 instead of exp(-inf + inf)
constexpr float kEmpty = -3.0e38f;
constexpr int kNoLabel = -(1 << 30);
constexpr int kMaxSplits = 64;
constexpr int kTargetBlocks = 512;  // two workgroups per CU

__device__ __forceinline__ int kc_off(int row, int chunk) { return row * 128 + 16 * (chunk ^ (row & 7)); }

__device__ __forceinline__ bf16x8 read_frag_kc(const char* base, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(base + kc_off(row, chunk));
}

// [128 rows][BK] tile of a k-contiguous operand: 4 x 16-B chunks per thread; rows past rmax read row rmax
__device__ __forceinline__ void load_tile(u32x4* r, const bf16* src, int ld, int row0, int k0, int rmax) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = threadIdx.x + kThreads * i;
    r[i] = *reinterpret_cast<const u32x4*>(src + (size_t)min(row0 + id / 8, rmax) * ld + k0 + 8 * (id % 8));
  }
}
__device__ __forceinline__ void store_tile(char* base, const u32x4* r) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = threadIdx.x + kThreads * i;
    *reinterpret_cast<u32x4*>(base + kc_off(id / 8, id % 8)) = r[i];
  }
}

__device__ __forceinline__ void merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  s = s * __expf(m - nm) + os * __expf(om - nm);
  m = nm;
}

struct LmLossParams {
  const bf16* x;
  const bf16* w;
  const int64_t* labels;
  float* part_m;     // [splits][M]
  float* part_s;     // [splits][M]
  float* lab_logit;  // [M]
  int ldx, ldw, w_rows, M, V, K, ignore_index;
  int panels, splits, tiles_per_split, tiles_n;
};

// one finished 128x128 tile of logits -> the lanes' running (max, sum) and the label logits
template <bool MASK>
__device__ __forceinline__ void fold_tile(const f32x4 (&acc)[4][4], float (&rm)[16], float (&rs)[16],
                                          const int (&rl)[16], int n0, int colbase, int row_base, const LmLossParams& P) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = 4 * i + r;
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = acc[i][j][r];
        if constexpr (MASK) v[j] = (n0 + colbase + 16 * j < P.V) ? v[j] : -INFINITY;
      }
      const int d = rl[q] - n0;  // the label's column relative to this lane's first column of the tile
      if ((uint32_t)d < 64u && (d & 15) == 0) {
        const int j = d >> 4;
        P.lab_logit[row_base + 16 * i + r] = j == 0 ? v[0] : j == 1 ? v[1] : j == 2 ? v[2] : v[3];
      }
      const float nm = fmaxf(rm[q], fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
      rs[q] = rs[q] * __expf(rm[q] - nm) + ((__expf(v[0] - nm) + __expf(v[1] - nm)) + (__expf(v[2] - nm) + __expf(v[3] - nm)));
      rm[q] = nm;
    }
}

__global__ __launch_bounds__(kThreads, 2) void lm_loss_partial_kernel(LmLossParams P) {
  __shared__ __attribute__((aligned(16))) char smem[kLdsBytes];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;

  // an XCD takes a contiguous range of panels of one split: its workgroups walk the same tiles of w together
  const int pid = xcd_remap(blockIdx.x, P.panels * P.splits);
  const int split = pid / P.panels, panel = pid % P.panels;
  const int m0 = panel * BM;
  const int t0 = split * P.tiles_per_split, t1 = min(t0 + P.tiles_per_split, P.tiles_n);
  const int nk = P.K / BK;
  const int total = (t1 - t0) * nk;
  const int colbase = wn * 64 + (lane & 15);
  const int row_base = m0 + wm * 64 + 4 * (lane >> 4);  // this lane's rows: row_base + 16 i + r

  float rm[16], rs[16];
  int rl[16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row_base + 16 * i + r;
      rm[4 * i + r] = kEmpty;
      rs[4 * i + r] = 0.f;
      int64_t y = -1;
      if (row < P.M) y = P.labels[row];
      rl[4 * i + r] = (y != P.ignore_index && y >= 0 && y < P.V) ? (int)y - colbase : kNoLabel;
    }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 ra[4], rb[4];
  load_tile(ra, P.x, P.ldx, m0, 0, P.M - 1);
  load_tile(rb, P.w, P.ldw, t0 * BN, 0, P.w_rows - 1);
  store_tile(smem, ra);
  store_tile(smem + BM * BK * 2, rb);
  __syncthreads();

  int tile = t0, kt = 0;
  for (int it = 0; it < total; ++it) {
    const int cur = it & 1;
    const char* As = smem + cur * kStageBytes;
    const char* Bs = As + BM * BK * 2;
    int nkt = kt + 1, ntile = tile;
    if (nkt == nk) {
      nkt = 0;
      ++ntile;
    }
    if (it + 1 < total) {
      load_tile(ra, P.x, P.ldx, m0, nkt * BK, P.M - 1);
      load_tile(rb, P.w, P.ldw, ntile * BN, nkt * BK, P.w_rows - 1);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        af[f] = read_frag_kc(As, wm * 64 + 16 * f + (lane & 15), 4 * kk + (lane >> 4));
        bfr[f] = read_frag_kc(Bs, wn * 64 + 16 * f + (lane & 15), 4 * kk + (lane >> 4));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (it + 1 < total) {
      char* nxt = smem + (cur ^ 1) * kStageBytes;
      store_tile(nxt, ra);
      store_tile(nxt + BM * BK * 2, rb);
    }
    __syncthreads();
    if (nkt == 0) {  // the tile's last K-tile: fold the logits and start the next tile from zero
      const int n0 = tile * BN;
      if (n0 + BN > P.V) fold_tile<true>(acc, rm, rs, rl, n0, colbase, row_base, P);
      else fold_tile<false>(acc, rm, rs, rl, n0, colbase, row_base, P);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    kt = nkt;
    tile = ntile;
  }

  // the 16 column lanes of a row (xor butterfly: every lane ends with the same bits)
#pragma unroll
  for (int q = 0; q < 16; ++q)
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const float om = __shfl_xor(rm[q], o, 64), os = __shfl_xor(rs[q], o, 64);
      merge(rm[q], rs[q], om, os);
    }
  // the two column waves (the loop's last barrier released the operand stages)
  float* red = reinterpret_cast<float*>(smem);  // [wm][64 rows][2]
  if (wn == 1 && (lane & 15) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = 16 * i + 4 * (lane >> 4) + r;
        red[(wm * 64 + lr) * 2] = rm[4 * i + r];
        red[(wm * 64 + lr) * 2 + 1] = rs[4 * i + r];
      }
  }
  __syncthreads();
  if (wn == 0 && (lane & 15) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int lr = 16 * i + 4 * (lane >> 4) + r;
        const int row = row_base + 16 * i + r;
        float m = rm[4 * i + r], s = rs[4 * i + r];
        merge(m, s, red[(wm * 64 + lr) * 2], red[(wm * 64 + lr) * 2 + 1]);
        if (row < P.M) {
          P.part_m[(size_t)split * P.M + row] = m;
          P.part_s[(size_t)split * P.M + row] = s;
        }
      }
  }
}

__global__ __launch_bounds__(1024) void lm_loss_finish_kernel(const float* __restrict__ part_m,
                                                             const float* __restrict__ part_s,
                                                             const float* __restrict__ lab_logit,
                                                             const int64_t* __restrict__ labels, int M, int V,
                                                             int splits, int ignore_index, float* __restrict__ loss_rows,
                                                             float* __restrict__ lse_out, float* __restrict__ loss_sum,
                                                             float* __restrict__ count, int accumulate,
                                                             float* __restrict__ loss_mean) {
  float s_loss = 0.f, n_valid = 0.f;
  for (int row = threadIdx.x; row < M; row += 1024) {
    float m = part_m[row], s = part_s[row];
    for (int sp = 1; sp < splits; ++sp) merge(m, s, part_m[(size_t)sp * M + row], part_s[(size_t)sp * M + row]);
    const float lse = m + __logf(s);
    const int64_t y = labels[row];
    // a label outside [0, V) (other than ignore_index) poisons its row with NaN, as gpt2mi_xent_fwd does
    const float l = (y == ignore_index) ? 0.f : (y < 0 || y >= V) ? __builtin_nanf("") : lse - lab_logit[row];
    if (loss_rows) loss_rows[row] = l;
    if (lse_out) lse_out[row] = lse;
    s_loss += l;
    n_valid += (y == ignore_index) ? 0.f : 1.f;
  }
  s_loss = wave_sum(s_loss);
  n_valid = wave_sum(n_valid);
  __shared__ float rs[16], rn[16];
  if ((threadIdx.x & 63) == 0) {
    rs[threadIdx.x >> 6] = s_loss;
    rn[threadIdx.x >> 6] = n_valid;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float S = 0.f, N = 0.f;
    for (int w = 0; w < 16; ++w) {
      S += rs[w];
      N += rn[w];
    }
    if (loss_mean) loss_mean[0] = S / N;  // NaN when every label is ignored, as gpt2mi_xent_fwd's loss
    if (loss_sum) loss_sum[0] = accumulate ? loss_sum[0] + S : S;
    if (count) count[0] = accumulate ? count[0] + N : N;
  }
}

// vocabulary splits: enough workgroups for two per CU, every split at least one tile
void plan_splits(int M, int V, int& panels, int& tiles_n, int& tiles_per_split, int& splits) {
  panels = (M + BM - 1) / BM;
  tiles_n = (V + BN - 1) / BN;
  int want = (kTargetBlocks + panels - 1) / panels;
  want = want < 1 ? 1 : want > kMaxSplits ? kMaxSplits : want;
  if (want > tiles_n) want = tiles_n;
  tiles_per_split = (tiles_n + want - 1) / want;
  splits = (tiles_n + tiles_per_split - 1) / tiles_per_split;
}

}  // namespace

GPT2MI_EXPORT size_t gpt2mi_lm_loss_workspace(int M, int V) {
  if (M < 1 || V < 1) return 0;
  int panels, tiles_n, tps, splits;
  plan_splits(M, V, panels, tiles_n, tps, splits);
  return (size_t)(2 * splits + 1) * (size_t)M * sizeof(float);
}

GPT2MI_EXPORT int gpt2mi_lm_loss(const uint16_t* x, int ldx, const uint16_t* w, int ldw, int w_rows,
                                 const int64_t* labels, int M, int V, int K, int ignore_index, float* loss_rows,
                                 float* lse, float* loss_sum, float* count, int accumulate, float* loss_mean,
                                 float* workspace, void* stream) {
  GPT2MI_REQUIRE(M >= 64 && M % 64 == 0, "lm_loss: M=%d must be a positive multiple of 64", M);
  GPT2MI_REQUIRE(K >= 64 && K % 64 == 0, "lm_loss: K=%d must be a positive multiple of 64", K);
  GPT2MI_REQUIRE(V >= 1, "lm_loss: V=%d must be >= 1", V);
  GPT2MI_REQUIRE(w_rows >= V, "lm_loss: w_rows=%d < V=%d", w_rows, V);
  GPT2MI_REQUIRE(ldx >= K && ldx % 8 == 0 && ldw >= K && ldw % 8 == 0,
                 "lm_loss: row strides must be multiples of 8 and >= K (ldx=%d ldw=%d K=%d)", ldx, ldw, K);
  GPT2MI_REQUIRE(x && w && labels && workspace, "lm_loss: x, w, labels and workspace must not be NULL");
  LmLossParams P;
  plan_splits(M, V, P.panels, P.tiles_n, P.tiles_per_split, P.splits);
  P.x = (const bf16*)x;
  P.w = (const bf16*)w;
  P.labels = labels;
  P.part_m = workspace;
  P.part_s = workspace + (size_t)P.splits * M;
  P.lab_logit = workspace + (size_t)2 * P.splits * M;
  P.ldx = ldx;
  P.ldw = ldw;
  P.w_rows = w_rows;
  P.M = M;
  P.V = V;
  P.K = K;
  P.ignore_index = ignore_index;
  hipStream_t s = (hipStream_t)stream;
  lm_loss_partial_kernel<<<P.panels * P.splits, kThreads, 0, s>>>(P);
  int rc = gpt2mi::check_launch("lm_loss_partial");
  if (rc) return rc;
  lm_loss_finish_kernel<<<1, 1024, 0, s>>>(P.part_m, P.part_s, P.lab_logit, labels, M, V, P.splits, ignore_index,
                                           loss_rows, lse, loss_sum, count, accumulate, loss_mean);
  return gpt2mi::check_launch("lm_loss_finish");
}
