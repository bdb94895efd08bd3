// bf16 MFMA GEMM for gfx950 with fused epilogues, 128x128 block tile: the fallback kernel of the step's Linears (any
// 64-multiple shape, the atomic split-K epilogue). The C ABI entry points are in gemm_api.hip.
//
//   C[m,n] (op)= epilogue( alpha * sum_k A(m,k) * B(n,k) )
//
// Operand layouts (template):
//   A_T=0: A stored [M][K] (row m, k contiguous)     A_T=1: A stored [K][M] (m contiguous)
//   B_T=0: B stored [N][K] (nn.Linear weight [out][in]) B_T=1: B stored [K][N]
// forward (x @ W^T)       : A_T=0, B_T=0   (model.py:95-96,174-177,326 under autocast bf16)
// dgrad   (dY @ W)        : A_T=0, B_T=1
// wgrad   (dY^T @ X)      : A_T=1, B_T=1   (split-K over tokens, fp32 atomics into the grad arena)
//
// Structure: 256 threads = 4 waves (2x2), 128x128 block tile, BK=64, v_mfma_f32_16x16x32_bf16,
// register-staged global->LDS double buffer (next tile's loads issued before the MFMAs, written
// after them, one barrier per K-tile). LDS images:
//   k-contiguous operand : [rows][64] bf16 (128-B rows), 16-B chunk c stored at c ^ (row & 7)
//                          -> fragment reads are conflict-free ds_read_b128;
//   m-contiguous operand : [64 k][128] bf16 (256-B rows), chunk c stored at c ^ 2*((k&3)|((k>>3&1)<<2))
//                          -> fragments by two conflict-free ds_read_b64_tr_b16 (hardware transpose).
// Epilogue: accumulators -> LDS (fp32, padded rows) -> row-contiguous 16-B chunks -> fused op -> HBM.
#include "common.h"
#include "gemm_epilogue.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int kThreads = 256;
constexpr int kStageBytes = (BM + BN) * BK * 2;           // 32 KiB
constexpr int kEpiLd = BN + 4;                            // fp32 epilogue row stride (floats)
constexpr int kLdsBytes = (2 * kStageBytes > BM * kEpiLd * 4) ? 2 * kStageBytes : BM * kEpiLd * 4;

__device__ __forceinline__ int kc_off(int row, int chunk) { return row * 128 + 16 * (chunk ^ (row & 7)); }
__device__ __forceinline__ int mc_swz(int k) { return 2 * ((k & 3) | (((k >> 3) & 1) << 2)); }
__device__ __forceinline__ int mc_off(int k, int chunk) { return k * 256 + 16 * ((chunk ^ mc_swz(k)) & 15); }

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ bf16x8 read_frag_kc(const char* base, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(base + kc_off(row, chunk));
}

// tr read of the m-contiguous image: lane (g=l>>4, q=(l&15)>>2, p=l&3) gives A[m0+(l&15)][k0+8g+j]
__device__ __forceinline__ bf16x8 read_frag_mc(const char* base, int k0, int m0, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int k1 = k0 + 8 * g + q;
  const int chunk = (m0 >> 3) + (p >> 1);
  const int off1 = mc_off(k1, chunk) + 8 * (p & 1);
  const int off2 = mc_off(k1 + 4, chunk) + 8 * (p & 1);
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + off1));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + off2));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, r);
}

// Tile loader: 4 x 16-B chunks per thread per operand per K-tile.
template <bool TRANS, int ROWS>
struct Loader {
  // TRANS=0: tile is [ROWS][BK] from src[row*ld + k]; TRANS=1: tile is [BK][ROWS] from src[k*ld + row]
  __device__ __forceinline__ static void load(u32x4* r, const bf16* src, int ld, int row0, int k0, int rmax) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = threadIdx.x + kThreads * i;
      const bf16* p;
      if constexpr (!TRANS) {
        p = src + (size_t)min(row0 + id / 8, rmax) * ld + k0 + 8 * (id % 8);
      } else {  // partial last tile (extent % 128 == 64): clamp the 8-column chunk into the row (rmax+1 is a
                // multiple of 64); the clamped columns only feed outputs the epilogue discards
        p = src + (size_t)(k0 + id / (ROWS / 8)) * ld + min(row0 + 8 * (id % (ROWS / 8)), rmax - 7);
      }
      r[i] = *reinterpret_cast<const u32x4*>(p);
    }
  }
  __device__ __forceinline__ static void store(char* base, const u32x4* r) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = threadIdx.x + kThreads * i;
      int off;
      if constexpr (!TRANS) {
        off = kc_off(id / 8, id % 8);
      } else {
        off = mc_off(id / (ROWS / 8), id % (ROWS / 8));
      }
      *reinterpret_cast<u32x4*>(base + off) = r[i];
    }
  }
};

template <bool A_T, bool B_T, int EPI>
__global__ __launch_bounds__(kThreads, 2) void gemm_kernel(GemmParams P) {
  __shared__ __attribute__((aligned(16))) char smem[kLdsBytes];
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;

  // tile scheduling: XCD-contiguous ranges, grouped-M ordering for L2 reuse
  const int tiles_m = (P.M + BM - 1) / BM, tiles_n = (P.N + BN - 1) / BN;
  const int ntiles = tiles_m * tiles_n;
  const int pid = xcd_remap(blockIdx.x, ntiles);
  constexpr int GM = 8;
  const int group = pid / (GM * tiles_n);
  const int first_m = group * GM;
  const int gsz = min(tiles_m - first_m, GM);
  const int tm = first_m + (pid % (GM * tiles_n)) % gsz;
  const int tn = (pid % (GM * tiles_n)) / gsz;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = blockIdx.z * P.k_per_split;
  const int nk = P.k_per_split / BK;

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 ra[4], rb[4];
  using LA = Loader<A_T, BM>;
  using LB = Loader<B_T, BN>;
  LA::load(ra, P.A, P.lda, m0, kbeg, P.M - 1);
  LB::load(rb, P.B, P.ldb, n0, kbeg, P.N - 1);
  LA::store(smem, ra);
  LB::store(smem + BM * BK * 2, rb);
  __syncthreads();

  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    const char* As = smem + cur * kStageBytes;
    const char* Bs = As + BM * BK * 2;
    if (kt + 1 < nk) {
      LA::load(ra, P.A, P.lda, m0, kbeg + (kt + 1) * BK, P.M - 1);
      LB::load(rb, P.B, P.ldb, n0, kbeg + (kt + 1) * BK, P.N - 1);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        if constexpr (!A_T) af[f] = read_frag_kc(As, wm * 64 + 16 * f + (lane & 15), 4 * kk + (lane >> 4));
        else af[f] = read_frag_mc(As, 32 * kk, wm * 64 + 16 * f, lane);
        if constexpr (!B_T) bfr[f] = read_frag_kc(Bs, wn * 64 + 16 * f + (lane & 15), 4 * kk + (lane >> 4));
        else bfr[f] = read_frag_mc(Bs, 32 * kk, wn * 64 + 16 * f, lane);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) {
      char* nxt = smem + (cur ^ 1) * kStageBytes;
      LA::store(nxt, ra);
      LB::store(nxt + BM * BK * 2, rb);
    }
    __syncthreads();
  }

  // ---- epilogue: accumulators -> LDS fp32 [BM][kEpiLd] ----
  float* ep = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * 64 + 16 * i + 4 * (lane >> 4) + r;
        const int col = wn * 64 + 16 * j + (lane & 15);
        ep[row * kEpiLd + col] = acc[i][j][r];
      }
  __syncthreads();

  float alpha = P.alpha;
  if (P.alpha_dev) alpha *= P.alpha_dev[0];

  if constexpr (EPI == EPI_ATOMIC) {
    float* C = reinterpret_cast<float*>(P.C);
#pragma unroll 4
    for (int it = 0; it < (BM * BN) / kThreads; ++it) {
      const int id = threadIdx.x + kThreads * it;
      const int row = id / BN, col = id % BN;
      if (m0 + row >= P.M || n0 + col >= P.N) continue;
      atomicAdd(C + (size_t)(m0 + row) * P.ldc + n0 + col, alpha * ep[row * kEpiLd + col]);
    }
    return;
  } else {
#pragma unroll 2
    for (int it = 0; it < (BM * BN) / (4 * kThreads); ++it) {
      const int id = threadIdx.x + kThreads * it;
      const int row = id / (BN / 4), c4 = 4 * (id % (BN / 4));
      const int gm = m0 + row, gn = n0 + c4;
      if (gm >= P.M || gn >= P.N) continue;
      f32x4 v = *reinterpret_cast<const f32x4*>(ep + row * kEpiLd + c4);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] *= alpha;
      if (P.bias && EPI != EPI_GELU_BWD) {
        f32x4 b = *reinterpret_cast<const f32x4*>(P.bias + gn);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += b[j];
      }
      epilogue_store<EPI>(P, gm, gn, v);
    }
  }
}

template <bool A_T, bool B_T, int EPI>
int launch(const gpt2mi::GemmPlan& plan, const GemmParams& P, hipStream_t s) {
  gemm_kernel<A_T, B_T, EPI><<<dim3(plan.grid, 1, plan.splits), kThreads, 0, s>>>(P);
  return gpt2mi::check_launch("gemm");
}

}  // namespace

namespace gpt2mi {
// Any M, N multiple of 64 (a half-width last tile), K a multiple of 64 * splits; split-K with the atomic epilogue
int gemm128_launch(const GemmPlan& plan, const GemmParams& P, hipStream_t s) {
  switch ((plan.a_t ? 32 : plan.b_t ? 16 : 0) + plan.epi) {
    case 0 * 16 + EPI_BF16: return launch<false, false, EPI_BF16>(plan, P, s);
    case 0 * 16 + EPI_F32: return launch<false, false, EPI_F32>(plan, P, s);
    case 0 * 16 + EPI_RESID: return launch<false, false, EPI_RESID>(plan, P, s);
    case 0 * 16 + EPI_GELU: return launch<false, false, EPI_GELU>(plan, P, s);
    case 0 * 16 + EPI_GELU_BWD: return launch<false, false, EPI_GELU_BWD>(plan, P, s);
    case 1 * 16 + EPI_BF16: return launch<false, true, EPI_BF16>(plan, P, s);
    case 1 * 16 + EPI_F32: return launch<false, true, EPI_F32>(plan, P, s);
    case 1 * 16 + EPI_GELU_BWD: return launch<false, true, EPI_GELU_BWD>(plan, P, s);
    case 2 * 16 + EPI_F32: return launch<true, true, EPI_F32>(plan, P, s);
    case 2 * 16 + EPI_ATOMIC: return launch<true, true, EPI_ATOMIC>(plan, P, s);
    default: return no_instance("gemm128", plan);
  }
}
}  // namespace gpt2mi
