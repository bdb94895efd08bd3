// Which kernel a bf16 GEMM call runs: one pure function per C ABI entry point (gemm_api.hip), from the arguments the
// choice depends on to a GemmPlan the kernel files' launchers take as decided. Plain C++20: no HIP headers, no globals,
// no allocation, no strings — it compiles on its own with a host compiler (tests/gemm_plan_check.cpp replays
// tests/golden/gemm_plan.json through it).
//
// The kernels, in the order the ladder prefers them:
//   ping-pong 256x256 (gemm_pp.hip): any M, N multiple of 64 in layout 0, full 256-tiles of the transposed operands in
//     layouts 1 / 2 through gpt2mi_gemm (the weight-gradient entries also run partial tiles, bounded: BND), K >= 128;
//     its persistent schedule (one block per CU) for the short-K layout-0 shapes with >= 2 tiles per CU; fuses dbias;
//   2-stage 256x256 (gemm256.hip): full column tiles (layout 2: full row tiles too), any K;
//   128x128 (gemm.hip): everything else, and the only kernel with the atomic split-K epilogue.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "gpt2mi.h"

enum Epi : int {
  EPI_BF16 = 0,      // C_bf16 = alpha*acc (+bias)
  EPI_F32 = 1,       // C_f32 (+)= alpha*acc (+bias)           (accumulate flag)
  EPI_RESID = 2,     // C_f32 = resid_f32 + drop(alpha*acc + bias)          (proj / fc2 + residual)
  EPI_GELU = 3,      // u = acc+bias: C = drop(gelu_tanh(u)), aux = keep/(1-p) * gelu'(u)  (fc1 + NewGELU + drop1)
  EPI_GELU_BWD = 4,  // C = alpha*acc * aux          (fc2 dgrad -> fc1 pre-activation grad: mask and gelu'
                     //                               were folded into aux by the forward epilogue)
  EPI_ATOMIC = 5,    // atomicAdd(C_f32, alpha*acc)            (split-K wgrad into the grad arena)
  EPI_SLAB = 6,      // split-K partial tile -> fp32 slab[split] (summed by splitk_reduce)
  EPI_SLAB16 = 7,    // the same partial tile rounded to a bf16 slab (GPT2MI_SCHED_BF16_SLABS; splitk_reduce16)
};

// Numeric tunables of the choice (A/B builds: -DGPT2MI_AB_BUILD on every GEMM source; guarded in gemm_params.h).
// longest K that takes the persistent schedule by default: the step's K = 768 / 2304 / 3072 shapes (qkv / fc1 dgrad
// and fc2 + residual 2-3 % faster than one tile per block since the persistent kernel reads the next K-tile's B
// fragments in phase 4); the lm_head dgrad (K = 50 432) stays one tile per block
#ifndef GPT2MI_PERSIST_KMAX
#define GPT2MI_PERSIST_KMAX 4096
#endif
#ifndef GPT2MI_PERSIST_GRID
#define GPT2MI_PERSIST_GRID 0  // A/B builds: a fixed persistent grid (a CU-masked stream's CU count), 0 = every CU
#endif
// bf16-slab weight gradients: half-tile map 2 (A contiguous, B interleaved) so that the epilogue takes the wide path
// (8 columns per lane, one 16-B store per row); map 3 (both interleaved, the fp32-slab kernel's) stores 8 B per lane
#ifndef PP_WGRAD16_MAP
#define PP_WGRAD16_MAP 2
#endif

namespace gpt2mi {

enum class GemmFamily : int {
  Refused = 0,         // no kernel takes these arguments (the entry point returns 22)
  PingPong,            // gemm_pp.hip, one tile per block
  PingPongPersistent,  // gemm_pp.hip, one block per CU walking the tiles
  TwoStage256,         // gemm256.hip
  Tile128,             // gemm.hip
};
enum class SlabType : int { None = 0, F32, BF16 };
enum class Reduce : int { None = 0, Plain, Transposed, Grouped };  // the splitk_reduce* launch that follows

struct GemmPlan {
  GemmFamily family;
  // the template instance
  bool a_t, b_t;  // operand stored m-contiguous ([K][M] / [K][N])
  int epi;        // Epi
  int map;        // ping-pong half-tile map: bit 0 = A interleaved, bit 1 = B interleaved
  bool bnd;       // ping-pong: a transposed operand has a partial last tile (bounded DMA)
  bool dyn;       // persistent: tiles from the work queue (GPT2MI_SCHED_SHARED_CUS)
  bool grouped;   // ping-pong: the grouped weight-gradient launch
  int grid;       // blocks in x (the 128x128 kernel: per split, `splits` in z)
  int splits;     // effective split count
  int k_per_split;
  SlabType slab;  // weight gradients: what the splits write into the workspace
  Reduce reduce;
  bool colsum;    // gpt2mi_colsum_bf16 of the stored output follows (dbias given, not fused by this kernel)
};

// sched low byte: the kernel-equivalence tests' and A/B tools' selectors
constexpr int kImplAuto = 0, kImpl128 = 1, kImplTwoStage = 2, kImplOneTile = 6;
constexpr int kSchedFlags = GPT2MI_SCHED_NO_PERSISTENT | GPT2MI_SCHED_SHARED_CUS;
constexpr bool sched_ok(int sched, int flags) {
  const int impl = sched & 0xff;
  return (sched & ~(flags | 0xff)) == 0 &&
         (impl == kImplAuto || impl == kImpl128 || impl == kImplTwoStage || impl == kImplOneTile);
}

constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }
constexpr int tiles256(int M, int N) { return ceil_div(M, 256) * ceil_div(N, 256); }
// the (layout, epilogue) pairs every kernel family has for layouts 0 / 1
constexpr bool fwd_dgrad_epi(int layout, int epi) {
  return layout == 0 ? (epi == EPI_BF16 || epi == EPI_F32 || epi == EPI_RESID || epi == EPI_GELU || epi == EPI_GELU_BWD)
                     : layout == 1 && (epi == EPI_BF16 || epi == EPI_F32 || epi == EPI_GELU_BWD);
}

// One ping-pong launch (one tile per block) over `splits` K ranges; a_t / b_t / epi / k_per_split set by the caller
constexpr GemmPlan pingpong(GemmPlan p, int M, int N, int splits, int map) {
  p.family = GemmFamily::PingPong;
  p.map = map;
  p.bnd = (p.a_t && M % 256 != 0) || (p.b_t && N % 256 != 0);
  p.splits = splits;
  p.grid = tiles256(M, N) * splits;
  return p;
}
constexpr int default_map(bool a_t, bool b_t) { return (a_t ? 1 : 0) | (b_t ? 2 : 0); }

// gpt2mi_gemm. layout: 0 = forward (A[M][K], B[N][K]); 1 = dgrad (A[M][K], B[K][N]); 2 = wgrad (A[K][M], B[K][N]).
constexpr GemmPlan plan_gemm(int layout, int epi, int M, int N, int K, int lda, int ldb, int splits, bool dbias,
                             int sched, int cus) {
  GemmPlan p{};
  if (layout < 0 || layout > 2 || M <= 0 || N <= 0 || M % 64 != 0 || N % 64 != 0 || splits < 1 ||
      K % (64 * splits) != 0 || (splits > 1 && epi != EPI_ATOMIC) || !sched_ok(sched, kSchedFlags) ||
      (dbias && !((epi == EPI_BF16 || epi == EPI_GELU_BWD) && layout <= 1)))
    return p;
  const int impl = sched & 0xff;
  p.a_t = layout == 2;
  p.b_t = layout >= 1;
  p.epi = epi;
  p.splits = splits;
  p.k_per_split = K / splits;
  // full 256-tiles of every transposed operand (layout 0 has none)
  const bool full_t = N % 256 == 0 && (layout <= 1 || M % 256 == 0);
  const bool one_pass = splits == 1 && epi != EPI_ATOMIC;
  if (one_pass && (layout == 0 || full_t) && (impl == kImplAuto || impl == kImplOneTile) && K >= 128) {
    if (layout == 2) {
      if (impl == kImplAuto && (epi == EPI_F32 || epi == EPI_SLAB || epi == EPI_SLAB16))
        return pingpong(p, M, N, 1, epi == EPI_SLAB16 ? PP_WGRAD16_MAP : 3);
    } else if (layout == 1 && (epi == EPI_SLAB || epi == EPI_SLAB16)) {
      return pingpong(p, M, N, 1, 2);
    } else if (fwd_dgrad_epi(layout, epi)) {
      // short-K forward-layout shapes with at least two tiles per CU: the persistent schedule (full tiles and an even
      // K-tile count >= 4 only: its epilogue has no row / column guard, and its K-tile 0 must be a steady-state tile;
      // operands within one 2-GiB buffer descriptor; dbias fused beside the GELU_BWD epilogue only)
      const bool persistent =
          layout == 0 && impl == kImplAuto && !(sched & GPT2MI_SCHED_NO_PERSISTENT) && K <= GPT2MI_PERSIST_KMAX &&
          K >= 256 && K % 128 == 0 && M % 256 == 0 && N % 256 == 0 && tiles256(M, N) >= 2 * cus &&
          epi != EPI_F32 && !(epi == EPI_BF16 && dbias) && (size_t)M * lda * 2 < (1ull << 31) &&
          (size_t)N * ldb * 2 < (1ull << 31);
      if (!persistent) return pingpong(p, M, N, 1, default_map(p.a_t, p.b_t));
      p.family = GemmFamily::PingPongPersistent;
      p.dyn = (sched & GPT2MI_SCHED_SHARED_CUS) != 0;
      const int blocks = GPT2MI_PERSIST_GRID > 0 ? GPT2MI_PERSIST_GRID : cus;
      p.grid = tiles256(M, N) < blocks ? tiles256(M, N) : blocks;
      return p;
    }
  }
  // the other kernels do not fuse the column sums
  p.colsum = dbias;
  if (one_pass && full_t && impl != kImpl128 &&
      (layout == 2 ? (epi == EPI_F32 || epi == EPI_SLAB) : fwd_dgrad_epi(layout, epi))) {
    p.family = GemmFamily::TwoStage256;
    p.grid = ceil_div(M, 256) * (N / 256);
    return p;
  }
  if (layout == 2 ? (epi == EPI_F32 || epi == EPI_ATOMIC) : fwd_dgrad_epi(layout, epi)) {
    p.family = GemmFamily::Tile128;
    p.grid = ceil_div(M, 128) * ceil_div(N, 128);
    return p;
  }
  return GemmPlan{};
}

// Split-K over `K` tokens as the caller asked for `splits` ranges: whole 64-deep K-tiles per split (an even number of
// them for the ping-pong kernel, which walks K-tile pairs), then as many splits as that leaves non-empty
struct SplitK {
  int splits, k_per_split;
};
constexpr SplitK split_k(int K, int splits, bool even_tiles) {
  int tiles_per = ceil_div(K / 64, splits);
  if (even_tiles) tiles_per += tiles_per & 1;
  const int kps = tiles_per * 64;
  return SplitK{ceil_div(K, kps), kps};
}

// gpt2mi_gemm_wgrad: C[M][N] (+)= A^T B, A stored [K][M], B stored [K][N]
constexpr GemmPlan plan_wgrad(int M, int N, int K, int lda, int ldb, int splits, int sched, int cus) {
  GemmPlan p{};
  if (M <= 0 || N <= 0 || K <= 0 || M % 64 != 0 || N % 64 != 0 || K % 64 != 0 || splits < 1 || splits > K / 64 ||
      !sched_ok(sched, kSchedFlags | GPT2MI_SCHED_BF16_SLABS))
    return p;
  const int impl = sched & 0xff;
  // the ping-pong kernel walks K-tile pairs: an even tile count (then every split's count is even too)
  const bool pp = impl == kImplAuto && (K / 64) % 2 == 0;
  // an odd token-tile count with a partial output tile, or the 128x128 kernel asked for: what gpt2mi_gemm picks for
  // the layout-2 fp32 GEMM (accumulates into / writes C, one pass, no slabs)
  if (!pp && (M % 256 != 0 || N % 256 != 0 || impl == kImpl128))
    return plan_gemm(2, EPI_F32, M, N, K, lda, ldb, 1, false,
                     (impl == kImpl128 ? kImpl128 : kImplAuto) | (sched & kSchedFlags), cus);
  const SplitK sk = split_k(K, splits, pp);
  // bf16 slabs on the ping-pong kernel only (the 2-stage fallback writes fp32 ones); one split writes C itself
  const bool slab16 = pp && sk.splits > 1 && (sched & GPT2MI_SCHED_BF16_SLABS);
  p.a_t = p.b_t = true;
  p.epi = sk.splits == 1 ? EPI_F32 : slab16 ? EPI_SLAB16 : EPI_SLAB;
  p.k_per_split = sk.k_per_split;
  if (sk.splits > 1) {
    p.slab = slab16 ? SlabType::BF16 : SlabType::F32;
    p.reduce = Reduce::Plain;
  }
  if (pp) return pingpong(p, M, N, sk.splits, slab16 ? PP_WGRAD16_MAP : 3);
  p.family = GemmFamily::TwoStage256;
  p.splits = sk.splits;
  p.grid = tiles256(M, N) * sk.splits;
  return p;
}

// gpt2mi_gemm_wgrad_kt: the same weight gradient with X given transposed (Bt[N][K]), as C^T[N][M] = Bt . A in layout
// 1 on the ping-pong kernel, always through slabs (one split: an fp32 slab), summed transposed into C
constexpr GemmPlan plan_wgrad_kt(int M, int N, int K, int splits, int sched) {
  GemmPlan p{};
  if (M <= 0 || N <= 0 || K <= 0 || M % 256 != 0 || N % 64 != 0 || K % 128 != 0 || splits < 1 || splits > K / 128 ||
      (sched & ~(kSchedFlags | GPT2MI_SCHED_BF16_SLABS | 0xff)) != 0)
    return p;
  const SplitK sk = split_k(K, splits, true);
  const bool slab16 = sk.splits > 1 && (sched & GPT2MI_SCHED_BF16_SLABS);
  p.b_t = true;
  p.epi = slab16 ? EPI_SLAB16 : EPI_SLAB;
  p.k_per_split = sk.k_per_split;
  p.slab = slab16 ? SlabType::BF16 : SlabType::F32;
  p.reduce = Reduce::Transposed;
  return pingpong(p, N, M, sk.splits, 2);
}

// gpt2mi_gemm_wgrad_grouped: `count` full-tile weight gradients over the same K tokens as one ping-pong launch over
// the (split, problem tile) items into fp32 slabs, and one reduction launch
constexpr int kGroupMax = 4;
constexpr GemmPlan plan_wgrad_grouped(int count, const int* M, const int* N, int K, int splits, int sched) {
  GemmPlan p{};
  if (count < 1 || count > kGroupMax || K <= 0 || K % 128 != 0 || splits < 1 || splits > K / 128 ||
      (sched & ~kSchedFlags) != 0)
    return p;
  int tiles = 0;
  for (int g = 0; g < count; ++g) {
    if (M[g] <= 0 || N[g] <= 0 || M[g] % 256 != 0 || N[g] % 256 != 0) return p;
    tiles += (M[g] / 256) * (N[g] / 256);
  }
  const SplitK sk = split_k(K, splits, true);
  p.family = GemmFamily::PingPong;
  p.a_t = p.b_t = true;
  p.epi = EPI_SLAB;
  p.map = 3;
  p.grouped = true;
  p.grid = tiles * sk.splits;
  p.splits = sk.splits;
  p.k_per_split = sk.k_per_split;
  p.slab = SlabType::F32;
  p.reduce = Reduce::Grouped;
  return p;
}

// gpt2mi_gemm_wgrad_batch: `count` full-tile weight gradients over the same K tokens as one ping-pong launch, one block
// per output tile over all K (plan_wgrad's one-split case for every problem: the EPI_F32 epilogue writes or accumulates
// C itself; no slabs, no reduction). The problem table lives in device memory (gemm_params.h GemmBatch): 4 x 36 problems
// (a 36-block model's four matrices) and room to spare
constexpr int kBatchMax = 256;
constexpr GemmPlan plan_wgrad_batch(int count, const int* M, const int* N, int K, int sched) {
  GemmPlan p{};
  if (count < 1 || count > kBatchMax || K <= 0 || K % 128 != 0 || (sched & ~kSchedFlags) != 0) return p;
  int tiles = 0;
  for (int g = 0; g < count; ++g) {
    if (M[g] <= 0 || N[g] <= 0 || M[g] % 256 != 0 || N[g] % 256 != 0) return p;
    tiles += (M[g] / 256) * (N[g] / 256);
  }
  p.family = GemmFamily::PingPong;
  p.a_t = p.b_t = true;
  p.epi = EPI_F32;
  p.map = 3;
  p.grouped = true;
  p.grid = tiles;
  p.splits = 1;
  p.k_per_split = K;
  return p;
}

}  // namespace gpt2mi
