// Muon for gfx950: momentum + normalisation, the batched Newton-Schulz products and the weight update, each ONE launch
// over every hidden weight matrix of the model (gpt2mi.h v24.8; the rule: gpt_2_distributed_amd/muon.py).
//
// Batch description (built once per optimizer, device memory; muon.py muon_tables):
//   mats  int64 [count][8]: off (arena element of W[0][0]), rows, cols, ld, xoff (element offset of the matrix in the
//         compact buffers: momentum fp32 [rows][cols]; X / X' bf16 [m][n], m = min(rows, cols), n = max), aoff (offset
//         in the A / B buffers, bf16 [m][m]), pstart, ptiles (the matrix's slice of the sum-of-squares partials)
//   items int32 [n][4]: (matrix, tile row, tile col, 0), one per block; the tiles of one matrix are consecutive, and
//         xcd_remap hands every XCD a consecutive range, so a matrix's operand panels meet in one L2.
//   Three item lists: 64x64 tiles of W as stored (prepare, update), the 128x128 tiles with col >= row of [m][m]
//   (gram, poly), the 128x128 tiles of [m][n] (apply).
//
// Products (one iteration: A = X X^T; B = b A + c A A; X' = a X + B X; every result rounded once to bf16):
//   gram / poly: C = S S^T for S = X ([m][n]) or S = A ([m][m], symmetric, so A A = A A^T): both MFMA operands are
//     k-contiguous row panels of the same matrix. Only tiles with tj >= ti are computed. An off-diagonal tile is
//     stored twice from the same fp32 values: row-major through LDS (16-B stores), and transposed straight from the
//     accumulators (a lane holds 4 consecutive rows of one column = 4 consecutive columns of the mirrored row: one
//     8-B store). A diagonal tile stores its upper triangle into both halves, so the result is symmetric bit for bit
//     whatever order the matrix unit adds in. poly adds b A in fp32 before the rounding; it reads the A element of
//     (row, col) as the 8-B group at (col, row..row+3), which is the same bits.
//   apply: B [m][m] k-contiguous, X [k = m][n] n-contiguous: X's fragments by the LDS transpose read
//     (ds_read_b64_tr_b16, the m-contiguous image of gemm.hip), no transposed copy of X. a X is added in the store pass.
//   Tile 128x128x64, 4 waves (2x2) of 4x4 v_mfma_f32_16x16x32_bf16, register-staged double-buffered LDS: the
//   matrices are C or 4C wide, so at C = 768 a 128-tile leaves 21 / 36 / 144 tiles per matrix and several hundred per
//   launch. m, n are multiples of 64: the last tile may be half, its operand rows / columns are
//   clamped into the matrix (they feed only outputs that are not stored).
// No floating-point atomics anywhere: two runs give the same bits.
#include "common.h"

namespace {

struct MuonMat {
  int64_t off, rows, cols, ld, xoff, aoff, pstart, ptiles;
};

// ---------------------------------------------------------------------------------------------------------------
// prepare / update: 64x64 tiles of W as stored, 256 threads, 4 x f32x4 per thread
// ---------------------------------------------------------------------------------------------------------------
constexpr int kT = 64;

__device__ __forceinline__ float muon_u(float gg, float bnew, float momentum, int nesterov) {
  return nesterov ? gg + momentum * bnew : bnew;
}

// buf = momentum buf + g; partials[item] = sum of u^2 over the tile (wave sums, then the 4 waves in order)
__global__ __launch_bounds__(256) void muon_momentum_kernel(const float* __restrict__ grad, float* __restrict__ buf,
                                                            const MuonMat* __restrict__ mats,
                                                            const int4* __restrict__ items, float grad_scale,
                                                            float momentum, int nesterov,
                                                            float* __restrict__ partials) {
  const int4 it = items[blockIdx.x];
  const MuonMat M = mats[it.x];
  const int r0 = it.y * kT, c0 = it.z * kT;
  const int tr = threadIdx.x >> 4, c4 = 4 * (threadIdx.x & 15);
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = r0 + tr + 16 * i;
    const f32x4 g = *reinterpret_cast<const f32x4*>(grad + M.off + row * M.ld + c0 + c4);
    float* bp = buf + M.xoff + row * M.cols + c0 + c4;
    f32x4 b = *reinterpret_cast<const f32x4*>(bp);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gg = g[j] * grad_scale;
      b[j] = momentum * b[j] + gg;
      const float u = muon_u(gg, b[j], momentum, nesterov);
      sq += u * u;
    }
    *reinterpret_cast<f32x4*>(bp) = b;
  }
  sq = wave_sum(sq);
  __shared__ float r[4];
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) partials[M.pstart + (int64_t)it.y * (M.cols / kT) + it.z] = r[0] + r[1] + r[2] + r[3];
}

// X0 = bf16(u / (||u|| + 1e-7)) in wide form; every block sums its matrix's partials in the same fixed order
__global__ __launch_bounds__(256) void muon_x0_kernel(const float* __restrict__ grad, const float* __restrict__ buf,
                                                      const MuonMat* __restrict__ mats,
                                                      const int4* __restrict__ items, float grad_scale,
                                                      float momentum, int nesterov,
                                                      const float* __restrict__ partials, bf16* __restrict__ x0) {
  const int4 it = items[blockIdx.x];
  const MuonMat M = mats[it.x];
  __shared__ double red[256];
  __shared__ float tile[kT][kT + 1];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < M.ptiles; i += 256) s += partials[M.pstart + i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  const float den = (float)sqrt(red[0]) + 1e-7f;
  const int r0 = it.y * kT, c0 = it.z * kT;
  const int tr = threadIdx.x >> 4, c4 = 4 * (threadIdx.x & 15);
  const bool tall = M.rows > M.cols;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t row = r0 + tr + 16 * i;
    const f32x4 g = *reinterpret_cast<const f32x4*>(grad + M.off + row * M.ld + c0 + c4);
    const f32x4 b = *reinterpret_cast<const f32x4*>(buf + M.xoff + row * M.cols + c0 + c4);
    float x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = muon_u(g[j] * grad_scale, b[j], momentum, nesterov) / den;
    if (!tall) {
      *reinterpret_cast<bf16x4*>(x0 + M.xoff + row * M.cols + c0 + c4) =
          bf16x4{f2bf(x[0]), f2bf(x[1]), f2bf(x[2]), f2bf(x[3])};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[tr + 16 * i][c4 + j] = x[j];
    }
  }
  if (tall) {  // X0 is W^T-shaped: [cols][rows]
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = tr + 16 * i;  // a column of the stored tile = a row of X0
      *reinterpret_cast<bf16x4*>(x0 + M.xoff + (int64_t)(c0 + rr) * M.rows + r0 + c4) =
          bf16x4{f2bf(tile[c4][rr]), f2bf(tile[c4 + 1][rr]), f2bf(tile[c4 + 2][rr]), f2bf(tile[c4 + 3][rr])};
    }
  }
}

// W = W (1 - lr wd) - lr sqrt(max(1, rows / cols)) O, and its bf16 shadow; O is [m][n]: W^T-shaped for a tall matrix
__global__ __launch_bounds__(256) void muon_update_kernel(float* __restrict__ p, bf16* __restrict__ pb,
                                                          const bf16* __restrict__ o,
                                                          const MuonMat* __restrict__ mats,
                                                          const int4* __restrict__ items, float lr, float wd) {
  const int4 it = items[blockIdx.x];
  const MuonMat M = mats[it.x];
  __shared__ float tile[kT][kT + 1];
  const int r0 = it.y * kT, c0 = it.z * kT;
  const int tr = threadIdx.x >> 4, c4 = 4 * (threadIdx.x & 15);
  const bool tall = M.rows > M.cols;
  if (tall) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = tr + 16 * i;
      const bf16x4 v = *reinterpret_cast<const bf16x4*>(o + M.xoff + (int64_t)(c0 + rr) * M.rows + r0 + c4);
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[rr][c4 + j] = bf2f(v[j]);
    }
    __syncthreads();
  }
  const float decay = 1.f - lr * wd;
  const float step = lr * sqrtf(fmaxf(1.f, (float)M.rows / (float)M.cols));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int rl = tr + 16 * i;
    const int64_t row = r0 + rl;
    float ov[4];
    if (!tall) {
      const bf16x4 v = *reinterpret_cast<const bf16x4*>(o + M.xoff + row * M.cols + c0 + c4);
#pragma unroll
      for (int j = 0; j < 4; ++j) ov[j] = bf2f(v[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) ov[j] = tile[c4 + j][rl];
    }
    float* pp = p + M.off + row * M.ld + c0 + c4;
    f32x4 w = *reinterpret_cast<const f32x4*>(pp);
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = w[j] * decay - step * ov[j];
    *reinterpret_cast<f32x4*>(pp) = w;
    if (pb)
      *reinterpret_cast<bf16x4*>(pb + M.off + row * M.ld + c0 + c4) =
          bf16x4{f2bf(w[0]), f2bf(w[1]), f2bf(w[2]), f2bf(w[3])};
  }
}

// ---------------------------------------------------------------------------------------------------------------
// the three products
// ---------------------------------------------------------------------------------------------------------------
constexpr int BM = 128, BN = 128, BK = 64;
constexpr int kThreads = 256;
constexpr int kStageBytes = (BM + BN) * BK * 2;  // 32 KiB
constexpr int kEpiLd = BN + 4;                   // fp32 epilogue row stride (floats)
constexpr int kLdsBytes = (2 * kStageBytes > BM * kEpiLd * 4) ? 2 * kStageBytes : BM * kEpiLd * 4;

enum { GRAM = 0, POLY = 1, APPLY = 2 };

// LDS images (those of gemm.hip): k-contiguous [rows][64], 16-B chunk c at c ^ (row & 7); n-contiguous [64 k][128],
// chunk c at c ^ 2*((k&3)|((k>>3&1)<<2)), read by two ds_read_b64_tr_b16 per fragment
__device__ __forceinline__ int kc_off(int row, int chunk) { return row * 128 + 16 * (chunk ^ (row & 7)); }
__device__ __forceinline__ int mc_swz(int k) { return 2 * ((k & 3) | (((k >> 3) & 1) << 2)); }
__device__ __forceinline__ int mc_off(int k, int chunk) { return k * 256 + 16 * ((chunk ^ mc_swz(k)) & 15); }

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ bf16x8 read_frag_kc(const char* base, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(base + kc_off(row, chunk));
}
// lane (g = l>>4, q = (l&15)>>2, p = l&3) gets X[k0 + 8g + j][n0 + (l&15)], j = 0..7
__device__ __forceinline__ bf16x8 read_frag_mc(const char* base, int k0, int n0, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int k1 = k0 + 8 * g + q;
  const int chunk = (n0 >> 3) + (p >> 1);
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + mc_off(k1, chunk) + 8 * (p & 1)));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + mc_off(k1 + 4, chunk) + 8 * (p & 1)));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

// a [128 rows][64 k] panel of a k-contiguous matrix: rows clamped to rmax (reads stay inside the matrix)
__device__ __forceinline__ void load_kc(u32x4* r, const bf16* src, int64_t ld, int row0, int k0, int rmax) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = threadIdx.x + kThreads * i;
    r[i] = *reinterpret_cast<const u32x4*>(src + (int64_t)min(row0 + id / 8, rmax) * ld + k0 + 8 * (id % 8));
  }
}
__device__ __forceinline__ void store_kc(char* base, const u32x4* r) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = threadIdx.x + kThreads * i;
    *reinterpret_cast<u32x4*>(base + kc_off(id / 8, id % 8)) = r[i];
  }
}
// a [64 k][128 cols] panel of a row-major [K][N] matrix: the 8-column chunk clamped to the row's last chunk
__device__ __forceinline__ void load_mc(u32x4* r, const bf16* src, int64_t ld, int col0, int k0, int cmax8) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = threadIdx.x + kThreads * i;
    r[i] = *reinterpret_cast<const u32x4*>(src + (int64_t)(k0 + id / 16) * ld + min(col0 + 8 * (id % 16), cmax8));
  }
}
__device__ __forceinline__ void store_mc(char* base, const u32x4* r) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = threadIdx.x + kThreads * i;
    *reinterpret_cast<u32x4*>(base + mc_off(id / 16, id % 16)) = r[i];
  }
}

// GRAM: out = bf16(S S^T), S = s0 = X.  POLY: out = bf16(c0 S + c1 S S^T), S = s0 = A.
// APPLY: out = bf16(c0 X + B X), s0 = B, s1 = X.
template <int MODE>
__global__ __launch_bounds__(kThreads, 2) void muon_mm_kernel(const bf16* __restrict__ s0, const bf16* __restrict__ s1,
                                                              bf16* __restrict__ out,
                                                              const MuonMat* __restrict__ mats,
                                                              const int4* __restrict__ items, int n_items, float c0,
                                                              float c1) {
  __shared__ __attribute__((aligned(16))) char smem[kLdsBytes];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;

  const int4 it = items[xcd_remap(blockIdx.x, n_items)];
  const MuonMat Mt = mats[it.x];
  const int m = (int)min(Mt.rows, Mt.cols), n = (int)max(Mt.rows, Mt.cols);
  // C [M][N] = A-operand [M][K] x B-operand
  const int M = m, N = MODE == APPLY ? n : m, K = MODE == GRAM ? n : m;
  const bf16* Ap = s0 + (MODE == GRAM ? Mt.xoff : Mt.aoff);
  const bf16* Bp = MODE == APPLY ? s1 + Mt.xoff : Ap;
  const int64_t lda = K, ldb = MODE == APPLY ? n : K, ldo = N;
  bf16* Cp = out + (MODE == APPLY ? Mt.xoff : Mt.aoff);
  const int m0 = it.y * BM, n0 = it.z * BN;
  const int nk = K / BK;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 ra[4], rb[4];
  auto load = [&](int k0) {
    load_kc(ra, Ap, lda, m0, k0, M - 1);
    if constexpr (MODE == APPLY) load_mc(rb, Bp, ldb, n0, k0, N - 8);
    else load_kc(rb, Bp, ldb, n0, k0, N - 1);
  };
  auto store = [&](char* stage) {
    store_kc(stage, ra);
    if constexpr (MODE == APPLY) store_mc(stage + BM * BK * 2, rb);
    else store_kc(stage + BM * BK * 2, rb);
  };
  load(0);
  store(smem);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const char* As = smem + cur * kStageBytes;
    const char* Bs = As + BM * BK * 2;
    if (kt + 1 < nk) load((kt + 1) * BK);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        af[f] = read_frag_kc(As, wm * 64 + 16 * f + (lane & 15), 4 * kk + (lane >> 4));
        if constexpr (MODE == APPLY) bfr[f] = read_frag_mc(Bs, 32 * kk, wn * 64 + 16 * f, lane);
        else bfr[f] = read_frag_kc(Bs, wn * 64 + 16 * f + (lane & 15), 4 * kk + (lane >> 4));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) store(smem + (cur ^ 1) * kStageBytes);
    __syncthreads();
  }

  // ---- epilogue: final fp32 values -> LDS [BM][kEpiLd]; the mirrored tile straight from the registers ----
  float* ep = reinterpret_cast<float*>(smem);
  const bool diag = MODE != APPLY && it.y == it.z;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rl = wm * 64 + 16 * i + 4 * (lane >> 4), cl = wn * 64 + 16 * j + (lane & 15);
      const int gr = m0 + rl, gc = n0 + cl;
      f32x4 v = acc[i][j];
      if constexpr (MODE != APPLY) {
        const bool inside = gr < M && gc < N;  // (M, N multiples of 64: the 4 rows are inside together)
        if constexpr (MODE == POLY) {
          // S[gr + r][gc] read as S[gc][gr + r]: S (gram's output) is symmetric bit for bit
          bf16x4 a = bf16x4{(bf16)0.f, (bf16)0.f, (bf16)0.f, (bf16)0.f};
          if (inside) a = *reinterpret_cast<const bf16x4*>(Ap + (int64_t)gc * lda + gr);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = c1 * v[r] + c0 * bf2f(a[r]);
        }
        if (!diag && inside)
          *reinterpret_cast<bf16x4*>(Cp + (int64_t)gc * ldo + gr) = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) ep[(rl + r) * kEpiLd + cl] = v[r];
    }
  __syncthreads();

#pragma unroll 2
  for (int t = 0; t < (BM * BN) / (8 * kThreads); ++t) {
    const int id = threadIdx.x + kThreads * t;
    const int row = id / (BN / 8), c8 = 8 * (id % (BN / 8));
    const int gm = m0 + row, gn = n0 + c8;
    if (gm >= M || gn >= N) continue;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = c8 + j;
      // a diagonal tile: the lower triangle takes the upper one's values
      v[j] = (diag && col < row) ? ep[col * kEpiLd + row] : ep[row * kEpiLd + col];
    }
    if constexpr (MODE == APPLY) {
      const bf16x8 x = *reinterpret_cast<const bf16x8*>(Bp + (int64_t)gm * ldb + gn);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += c0 * bf2f(x[j]);
    }
    *reinterpret_cast<bf16x8*>(Cp + (int64_t)gm * ldo + gn) =
        bf16x8{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3]), f2bf(v[4]), f2bf(v[5]), f2bf(v[6]), f2bf(v[7])};
  }
}

int check_batch(const char* what, const void* mats, const void* items, int n_items) {
  GPT2MI_REQUIRE(mats && items, "%s: the matrix and item tables are required", what);
  GPT2MI_REQUIRE(n_items > 0, "%s: n_items=%d", what, n_items);
  return 0;
}

}  // namespace

GPT2MI_EXPORT int gpt2mi_muon_prepare(const float* grad, float* buf, const int64_t* mats, const int* items,
                                      int n_items, float grad_scale, float momentum, int nesterov, float* partials,
                                      uint16_t* x0, void* stream) {
  if (int rc = check_batch("muon_prepare", mats, items, n_items)) return rc;
  GPT2MI_REQUIRE(grad && buf && partials && x0, "muon_prepare: grad, buf, partials and x0 are required");
  hipStream_t s = (hipStream_t)stream;
  muon_momentum_kernel<<<n_items, 256, 0, s>>>(grad, buf, (const MuonMat*)mats, (const int4*)items, grad_scale,
                                               momentum, nesterov, partials);
  muon_x0_kernel<<<n_items, 256, 0, s>>>(grad, buf, (const MuonMat*)mats, (const int4*)items, grad_scale, momentum,
                                         nesterov, partials, (bf16*)x0);
  return gpt2mi::check_launch("muon_prepare");
}

GPT2MI_EXPORT int gpt2mi_muon_gram(const uint16_t* x, uint16_t* a, const int64_t* mats, const int* items, int n_items,
                                   void* stream) {
  if (int rc = check_batch("muon_gram", mats, items, n_items)) return rc;
  GPT2MI_REQUIRE(x && a, "muon_gram: x and a are required");
  muon_mm_kernel<GRAM><<<n_items, kThreads, 0, (hipStream_t)stream>>>((const bf16*)x, nullptr, (bf16*)a,
                                                                      (const MuonMat*)mats, (const int4*)items,
                                                                      n_items, 0.f, 0.f);
  return gpt2mi::check_launch("muon_gram");
}

GPT2MI_EXPORT int gpt2mi_muon_poly(const uint16_t* a, uint16_t* b, const int64_t* mats, const int* items, int n_items,
                                   float cb, float cc, void* stream) {
  if (int rc = check_batch("muon_poly", mats, items, n_items)) return rc;
  GPT2MI_REQUIRE(a && b && a != b, "muon_poly: a and b are required and distinct");
  muon_mm_kernel<POLY><<<n_items, kThreads, 0, (hipStream_t)stream>>>((const bf16*)a, nullptr, (bf16*)b,
                                                                      (const MuonMat*)mats, (const int4*)items,
                                                                      n_items, cb, cc);
  return gpt2mi::check_launch("muon_poly");
}

GPT2MI_EXPORT int gpt2mi_muon_apply(const uint16_t* b, const uint16_t* x, uint16_t* x_out, const int64_t* mats,
                                    const int* items, int n_items, float ca, void* stream) {
  if (int rc = check_batch("muon_apply", mats, items, n_items)) return rc;
  GPT2MI_REQUIRE(b && x && x_out && x != x_out, "muon_apply: b, x and x_out are required, x_out distinct from x");
  muon_mm_kernel<APPLY><<<n_items, kThreads, 0, (hipStream_t)stream>>>((const bf16*)b, (const bf16*)x, (bf16*)x_out,
                                                                       (const MuonMat*)mats, (const int4*)items,
                                                                       n_items, ca, 0.f);
  return gpt2mi::check_launch("muon_apply");
}

GPT2MI_EXPORT int gpt2mi_muon_update(float* p, uint16_t* p_bf16, const uint16_t* o, const int64_t* mats,
                                     const int* items, int n_items, float lr, float wd, void* stream) {
  if (int rc = check_batch("muon_update", mats, items, n_items)) return rc;
  GPT2MI_REQUIRE(p && o, "muon_update: p and o are required");
  muon_update_kernel<<<n_items, 256, 0, (hipStream_t)stream>>>(p, (bf16*)p_bf16, (const bf16*)o, (const MuonMat*)mats,
                                                               (const int4*)items, lr, wd);
  return gpt2mi::check_launch("muon_update");
}
