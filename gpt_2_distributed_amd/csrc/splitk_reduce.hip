// Split-K reductions: the sums of the partial slabs a split-K weight gradient (gemm_pp.hip / gemm256.hip, EPI_SLAB /
// EPI_SLAB16) wrote into its workspace, in fixed split order (deterministic; no atomics).
#include "common.h"
#include "gemm_epilogue.h"

namespace {

// out[i] (+)= sum_z slab[z][i]   (fixed summation order: deterministic). The slabs' loads go out in groups of 8 before
// their adds (in split order: the same bits as one load per add), so a thread keeps 8 loads in flight instead of one
// (the 27-split proj reduction was latency-bound)
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ slab, int splits, size_t n4,
                                                            float* __restrict__ out, int accumulate) {
  const f32x4* s4 = reinterpret_cast<const f32x4*>(slab);
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    f32x4 s = accumulate ? reinterpret_cast<const f32x4*>(out)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < splits; z += 8) {
      const int nz = min(8, splits - z);  // (uniform)
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (u < nz) v[u] = s4[(size_t)(z + u) * n4 + i];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (u < nz) s += v[u];
    }
    reinterpret_cast<f32x4*>(out)[i] = s;
  }
}

// The same sums for the problems of a grouped weight-gradient launch (gpt2mi_gemm_wgrad_grouped): blockIdx.y is the
// problem, whose slabs / output / length come from the kernel arguments; the same per-element order as above
struct ReduceGroup {
  const float* slab[kGroupMax];
  float* out[kGroupMax];
  size_t n4[kGroupMax];
};
__global__ __launch_bounds__(256) void splitk_reduce_grouped_kernel(ReduceGroup R, int splits, int accumulate) {
  const int g = blockIdx.y;
  const f32x4* s4 = reinterpret_cast<const f32x4*>(R.slab[g]);
  f32x4* o4 = reinterpret_cast<f32x4*>(R.out[g]);
  const size_t n4 = R.n4[g];
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    f32x4 s = accumulate ? o4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < splits; z += 8) {
      const int nz = min(8, splits - z);  // (uniform)
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (u < nz) v[u] = s4[(size_t)(z + u) * n4 + i];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (u < nz) s += v[u];
    }
    o4[i] = s;
  }
}

// bf16 slabs (GPT2MI_SCHED_BF16_SLABS): 8 elements per thread (one 16-B load per slab), each widened to fp32 and added
// in the order above (the old value first when accumulating, then the slabs in split order)
__global__ __launch_bounds__(256) void splitk_reduce16_kernel(const bf16* __restrict__ slab, int splits, size_t n8,
                                                              float* __restrict__ out, int accumulate) {
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    f32x4* o = reinterpret_cast<f32x4*>(out) + 2 * i;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
    if (accumulate) {
      s0 = o[0];
      s1 = o[1];
    }
    for (int z = 0; z < splits; ++z) {
      const bf16x8 v = reinterpret_cast<const bf16x8*>(slab + (size_t)z * n8 * 8)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s0[e] += bf2f(v[e]);
        s1[e] += bf2f(v[4 + e]);
      }
    }
    o[0] = s0;
    o[1] = s1;
  }
}

// 64 x 64 tile of the slabs per block, summed as splitk_reduce sums (the old value first when accumulating, then the
// slabs in split order: the same bits), staged through LDS and written transposed: 16-B loads and stores, 16 lanes per
// 256-B row segment on both sides
template <typename TS>  // slab element: float, or bf16 (GPT2MI_SCHED_BF16_SLABS)
__global__ __launch_bounds__(256) void splitk_reduce_t_kernel(const TS* __restrict__ slab, int splits, int rows,
                                                              int cols, float* __restrict__ out, int accumulate) {
  __shared__ float t[64][65];
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const int q = threadIdx.x & 15, p = threadIdx.x >> 4;  // 16 lanes x 4 floats per 64-float segment, 16 segments / pass
  const size_t plane = (size_t)rows * cols;
  if (accumulate) {  // t[r][c] = out[c][r]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 16 * i + p;
      const f32x4 v = *reinterpret_cast<const f32x4*>(out + (size_t)(c0 + c) * rows + r0 + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) t[4 * q + e][c] = v[e];
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = 16 * i + p;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (accumulate) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = t[r][4 * q + e];
    }
    const TS* src = slab + (size_t)(r0 + r) * cols + c0 + 4 * q;
    for (int z = 0; z < splits; ++z) {
      const f32x4 w = load4<TS>(src + z * plane);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += w[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) t[r][4 * q + e] = v[e];  // (the lane's own elements: read above, by it alone)
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = 16 * i + p;
    const f32x4 v = {t[4 * q][c], t[4 * q + 1][c], t[4 * q + 2][c], t[4 * q + 3][c]};
    *reinterpret_cast<f32x4*>(out + (size_t)(c0 + c) * rows + r0 + 4 * q) = v;
  }
}

}  // namespace

namespace gpt2mi {
int splitk_reduce_t(const float* slab, int splits, int rows, int cols, float* out, int accumulate, hipStream_t s) {
  splitk_reduce_t_kernel<float><<<dim3(cols / 64, rows / 64), 256, 0, s>>>(slab, splits, rows, cols, out, accumulate);
  return check_launch("splitk_reduce_t");
}
int splitk_reduce16_t(const bf16* slab, int splits, int rows, int cols, float* out, int accumulate, hipStream_t s) {
  splitk_reduce_t_kernel<bf16><<<dim3(cols / 64, rows / 64), 256, 0, s>>>(slab, splits, rows, cols, out, accumulate);
  return check_launch("splitk_reduce16_t");
}
int splitk_reduce16(const bf16* slab, int splits, size_t n, float* out, int accumulate, hipStream_t s) {
  splitk_reduce16_kernel<<<2048, 256, 0, s>>>(slab, splits, n / 8, out, accumulate);
  return check_launch("splitk_reduce16");
}
int splitk_reduce_grouped(const float* const* slab, float* const* out, const size_t* n, int count, int splits,
                          int accumulate, hipStream_t s) {
  ReduceGroup R{};
  for (int g = 0; g < count; ++g) {
    R.slab[g] = slab[g];
    R.out[g] = out[g];
    R.n4[g] = n[g] / 4;
  }
  splitk_reduce_grouped_kernel<<<dim3(2048 / count, count), 256, 0, s>>>(R, splits, accumulate);
  return check_launch("splitk_reduce_grouped");
}
int splitk_reduce(const float* slab, int splits, size_t n, float* out, int accumulate, hipStream_t s) {
  splitk_reduce_kernel<<<2048, 256, 0, s>>>(slab, splits, n / 4, out, accumulate);
  return check_launch("splitk_reduce");
}
}  // namespace gpt2mi
