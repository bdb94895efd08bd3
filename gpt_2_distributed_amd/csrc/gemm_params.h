// Host-visible part of the bf16 GEMMs: the parameter block every kernel takes and the launchers the kernel files
// expose to the C ABI entry points (gemm_api.hip). The epilogue device code is in gemm_epilogue.h; which launcher a
// call gets is decided in gemm_plan.h (Epi, GemmPlan).
#pragma once
#include "common.h"
#include "gemm_plan.h"

GPT2MI_PRODUCT_KNOB(GPT2MI_PERSIST_KMAX, 4096);
GPT2MI_PRODUCT_KNOB(GPT2MI_PERSIST_GRID, 0);
GPT2MI_PRODUCT_KNOB(PP_WGRAD16_MAP, 2);

struct GemmParams {
  const bf16* A;
  const bf16* B;
  void* C;
  const float* bias;
  const float* resid;
  void* aux;  // EPI_GELU: masked GELU derivative out; EPI_GELU_BWD: the same, in (element type = TE)
  const float* alpha_dev;
  float* dbias;  // optional: dbias[n] += sum_m C[m][n] of the stored output (bias grad of the next op)
  int M, N, K, lda, ldb, ldc, ldaux;
  int k_per_split;
  float alpha;
  int accumulate;
  uint64_t seed;
  uint32_t thr;
  float inv_keep;
  int qslot;  // persistent schedule: this launch's work-queue slot (gemm_pp.hip g_pp_queue; set by its launcher)
};

// Grouped weight gradients: kGroupMax problems at most, one launch (gemm_pp.hip gemm_pp_kernel, GRP); prefix[g] =
// output tiles of problems 0 .. g-1 (prefix[count] = tiles)
using gpt2mi::kGroupMax;
struct GemmGroup {
  GemmParams p[kGroupMax];
  int prefix[kGroupMax + 1];
  int count, tiles;
};

// Batched weight gradients (gpt2mi_gemm_wgrad_batch; gemm_pp.hip gemm_pp_kernel, BAT): up to kBatchMax unsplit problems
// in one launch. The table is too large for a kernel argument (kBatchMax x sizeof(GemmParams) against 4 KiB), so it
// lives in device memory: p[count] and prefix[count + 1] (the output tiles of problems 0 .. g-1) in the caller's
// scratch, uploaded stream-ordered ahead of the launch.
using gpt2mi::kBatchMax;
struct GemmBatch {
  const GemmParams* p;
  const int* prefix;
  int count, tiles;
};
constexpr size_t gemm_batch_table_bytes(int count) {
  return (size_t)count * sizeof(GemmParams) + (size_t)(count + 1) * sizeof(int);
}

namespace gpt2mi {
// CUs of the current device rounded down to a multiple of the 8 XCDs (256 when no device answers): plan_gemm's `cus`
int num_cus();
// One launch of the instance a plan names (plan.family is the file's; a plan that names an instance the file does not
// build is a programming error, reported as 22)
inline int no_instance(const char* file, const GemmPlan& plan) {
  set_error("%s: no kernel instance for A_T=%d B_T=%d epilogue %d map %d family %d", file, (int)plan.a_t, (int)plan.b_t,
            plan.epi, plan.map, (int)plan.family);
  return 22;
}
int gemm_pp_launch(const GemmPlan& plan, const GemmParams& P, hipStream_t s);          // gemm_pp.hip
int gemm_pp_launch_grouped(const GemmPlan& plan, const GemmGroup& G, hipStream_t s);   // gemm_pp.hip
int gemm_pp_launch_batch(const GemmPlan& plan, const GemmBatch& G, hipStream_t s);     // gemm_pp.hip
int gemm256_launch(const GemmPlan& plan, const GemmParams& P, hipStream_t s);          // gemm256.hip
int gemm128_launch(const GemmPlan& plan, const GemmParams& P, hipStream_t s);          // gemm.hip
// Split-K slab sums (splitk_reduce.hip), every one in split order (deterministic):
// out[i] (+)= sum_z slab[z][i]
int splitk_reduce(const float* slab, int splits, size_t n, float* out, int accumulate, hipStream_t s);
// the same sums over bf16 slabs (each element widened to fp32, then added in split order)
int splitk_reduce16(const bf16* slab, int splits, size_t n, float* out, int accumulate, hipStream_t s);
// out[c][r] (+)= sum_z slab[z][r][c]: slabs [splits][rows][cols] summed in split order and written transposed
int splitk_reduce_t(const float* slab, int splits, int rows, int cols, float* out, int accumulate, hipStream_t s);
int splitk_reduce16_t(const bf16* slab, int splits, int rows, int cols, float* out, int accumulate, hipStream_t s);
// out_g[i] (+)= sum_z slab_g[z][i] for every problem g of a grouped launch (fp32 slabs)
int splitk_reduce_grouped(const float* const* slab, float* const* out, const size_t* n, int count, int splits,
                          int accumulate, hipStream_t s);
}  // namespace gpt2mi
