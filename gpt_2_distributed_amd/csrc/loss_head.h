// What the fused loss heads share: the cross entropy (xent_adamw.hip), the policy-gradient head (policy_loss.hip) and
// the distillation head (distill_loss.hip). Each head has a register-resident row kernel (one 1024-thread workgroup
// per row of bf16 logits at GPT-2's vocabulary) and a strided two-pass kernel (256 threads, fp32 logits or any V),
// then one finalize launch for the batch's scalars. Here, once: the 8-wide loads and stores, the packed row and its
// fence, the 1024-thread reductions, the store sweep's frame, the finalize kernel and the host's choice of kernel.
// The per-row rules (what a sweep accumulates, the row's scalars, one element of dlogits) stay in the heads' files.
// Everything is in an unnamed namespace: each file compiles its own copy under its own flags (csrc/Makefile).
#pragma once
#include "common.h"

namespace {

// ---- 8 logits at a time (bf16: one 16-byte access, fp32: two) ------------------------------------------------------
template <typename TL>
__device__ __forceinline__ void load8(const TL* p, float* f) {
  if constexpr (sizeof(TL) == 2) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = bf2f(v[j]);
  } else {
    const f32x4 a = reinterpret_cast<const f32x4*>(p)[0], b = reinterpret_cast<const f32x4*>(p)[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[j] = a[j];
      f[4 + j] = b[j];
    }
  }
}
template <typename TL>
__device__ __forceinline__ void store8(TL* p, const float* f) {
  if constexpr (sizeof(TL) == 2) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(f[j]);
    *reinterpret_cast<bf16x8*>(p) = o;
  } else {
    reinterpret_cast<f32x4*>(p)[0] = f32x4{f[0], f[1], f[2], f[3]};
    reinterpret_cast<f32x4*>(p)[1] = f32x4{f[4], f[5], f[6], f[7]};
  }
}

__device__ __forceinline__ float uniform(float x) {  // a value every lane holds, into an SGPR
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

// A column that holds -inf (the padding as the reductions see it, or a masked logit) has probability 0, and its
// logit or log-probability is floored before it is multiplied by that 0 or enters a difference that is:
// 0 * floor = 0 and 0 * (floor - floor) = 0, where 0 * -inf or 0 * (-inf - -inf) would put a NaN into a good row.
constexpr float kLogFloor = -1e30f;
__device__ __forceinline__ float floored(float x) { return fmaxf(x, kLogFloor); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- the register-resident row --------------------------------------------------------------------------------------
// One row of bf16 logits held packed by a 1024-thread workgroup between the sweeps of a row kernel: NCH chunks of 8
// logits per thread (4 VGPRs a chunk), chunk i of thread tid at column 8 * (tid + 1024 * i), read from HBM once.
template <int NCH>
struct PackedRow {
  bf16x8 raw[NCH];

  __device__ __forceinline__ void load(const bf16* p, int ld, int V, int tid) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = 8 * (tid + 1024 * i);
      raw[i] = c < ld ? *reinterpret_cast<const bf16x8*>(p + c) : bf16x8{};
      if (c + 8 > V) {  // the padding (and the unread tail) never wins the max and has exp(.) = 0
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (c + j >= V) raw[i][j] = (bf16)(-INFINITY);
      }
    }
  }
  // the row stays packed between the phases: without these fences the compiler keeps all 56 unpacked fp32 values
  // live across the reductions (90 VGPRs = one 1024-thread block per CU, whose load and store phases never overlap)
  __device__ __forceinline__ void fence() {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      u32x4 t = __builtin_bit_cast(u32x4, raw[i]);
      asm volatile("" : "+v"(t));
      raw[i] = __builtin_bit_cast(bf16x8, t);
    }
  }
  __device__ __forceinline__ float val(int i, int j) const { return bf2f(raw[i][j]); }
};

// ---- reductions over a 1024-thread workgroup (16 waves) ------------------------------------------------------------
// v[k] = the maximum of v[k] over the workgroup, in every thread; one exchange carries all N. LDS: red[N][16] (a slot
// per wave) and bcast[N]; a caller may write either again once it has passed its next barrier. In both exchanges
// every wave value is formed before the first is stored: with each stored as it is formed, the two-row distillation
// kernel schedules into 103 VGPRs (maxima) or spills (sums).
template <int N>
__device__ __forceinline__ void group_max(float (&v)[N], float (*red)[16], float* bcast, int tid) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_max(v[k]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[k][tid >> 6] = v[k];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      float t = red[k][0];
      for (int w = 1; w < 16; ++w) t = fmaxf(t, red[k][w]);
      bcast[k] = t;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = bcast[k];
}

__device__ __forceinline__ float wave_total(float v) { return wave_sum(v); }
__device__ __forceinline__ double wave_total(double v) { return wave_sum_f64(v); }

// v[k] = the sum of v[k] over the workgroup, in wave 0 only: each wave's butterfly, then the 16 wave sums added by
// wave 0's butterfly: a fixed order, and no 16 N values in one thread. T = double adds across lanes and waves in fp64.
template <typename T, int N>
__device__ __forceinline__ void group_sum_wave0(T (&v)[N], T (*red)[16], int tid) {
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = wave_total(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[k][w] = v[k];
  }
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_total(lane < 16 ? red[k][lane] : (T)0);
  }
}

// ---- the store sweep of a row kernel, from registers -----------------------------------------------------------------
// dlogits of one row in 16-byte stores, nothing at or past ldd: elem(l...) of the column's logit in each of `rows`,
// rounded once; in the label's column elem(l...) - at_label (formed again in fp32 to the end: one rounding); zeros in
// an ignored row, and +0 in the padding [V, ldd), whatever the signs of the coefficients (and in a NaN row).
template <int NCH, typename Elem, typename... Rows>
__device__ __forceinline__ void store_row(bf16* dp, int ldd, int V, int tid, bool ign, int64_t y, float at_label,
                                          Elem elem, const Rows&... rows) {
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c0 = 8 * (tid + 1024 * i);
    if (c0 >= ldd) continue;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(ign ? 0.f : elem(rows.val(i, j)...));
    if (!ign && (uint32_t)(y - c0) < 8u) o[y - c0] = f2bf(elem(rows.val(i, y - c0)...) - at_label);
    if (c0 + 8 > V) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (c0 + j >= V) o[j] = (bf16)0.f;
    }
    *reinterpret_cast<bf16x8*>(dp + c0) = o;
  }
}

// ---- the batch's scalars ------------------------------------------------------------------------------------------------
// NM per-row metric columns of a head (none: the cross entropy), read only when the caller asks for their means.
template <int NM>
struct HeadMetrics {
  const float* col[NM ? NM : 1];
  float* mean;  // [NM] or NULL
};

// One workgroup: loss = sum(loss_rows) / N, inv_count = 1 / N (the dlogits scale for backward; N = labels !=
// ignore_index, NaN / inf at N = 0, as F.cross_entropy), mean[k] = sum(col[k]) / N: ignored rows hold 0 in each
// column. Every thread adds its rows in row order, then the waves' butterflies, then the 16 wave sums in wave order.
template <int NM>
__global__ __launch_bounds__(1024) void head_finalize_kernel(const float* __restrict__ loss_rows,
                                                            const int64_t* __restrict__ labels, int M, int ignore_index,
                                                            float* __restrict__ loss, float* __restrict__ inv_count,
                                                            HeadMetrics<NM> m) {
  constexpr int NQ = 2 + NM;
  const bool means = NM && m.mean;
  float q[NQ] = {};
  // four rows' loads issued together, then added in row order (the same sums as one row per step: 33 us with one
  // dependent load at a time over cfg 2's 65536 rows)
  int i = threadIdx.x;
  for (; i + 3 * 1024 < M; i += 4 * 1024) {
    float l[4], c[4][NM ? NM : 1];
    int64_t y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      l[k] = loss_rows[i + 1024 * k];
      y[k] = labels[i + 1024 * k];
#pragma unroll
      for (int n = 0; n < NM; ++n) c[k][n] = means ? m.col[n][i + 1024 * k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      q[0] += l[k];
      q[1] += (y[k] == ignore_index) ? 0.f : 1.f;
#pragma unroll
      for (int n = 0; n < NM; ++n) q[2 + n] += c[k][n];
    }
  }
  for (; i < M; i += 1024) {
    q[0] += loss_rows[i];
    q[1] += (labels[i] == ignore_index) ? 0.f : 1.f;
#pragma unroll
    for (int n = 0; n < NM; ++n) q[2 + n] += means ? m.col[n][i] : 0.f;
  }
  __shared__ float red[NQ][16];
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    q[k] = wave_sum(q[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = q[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot[NQ];
    for (int k = 0; k < NQ; ++k) {
      tot[k] = 0.f;
      for (int w = 0; w < 16; ++w) tot[k] += red[k][w];
    }
    loss[0] = tot[0] / tot[1];  // NaN when every label is ignored, as F.cross_entropy
    inv_count[0] = 1.f / tot[1];
    if (means)
      for (int k = 0; k < NM; ++k) m.mean[k] = tot[2 + k] / tot[1];
  }
}

// ---- the host's side of one head call ----------------------------------------------------------------------------------
// The logits of a call as the choice of kernel sees them; ldt: the teacher's row stride, in a head that reads one.
struct HeadShape {
  int ld, ldt, ldd, V;
  bool has_teacher, has_dlogits, bf16_logits;
};

// Checks the row strides, launches the head's row kernel (bf16 logits whose widest row is 7 chunks of 8 * 1024: GPT-2's
// vocabulary under autocast, register-resident) or its strided kernel, then the finalize kernel. `head` names the call
// in an error: "<head>_fwd: row strides ...", and the launches "<head>_row", "<head>_fwd", "<head>_finalize". row()
// and strided() launch on `s`.
template <int NM, typename Row, typename Strided>
int head_launch(const char* head, const HeadShape& h, Row row, Strided strided, const float* loss_rows,
                const int64_t* labels, int M, int ignore_index, float* loss, float* inv_count, const HeadMetrics<NM>& m,
                hipStream_t s) {
  const bool ok = h.ld % 8 == 0 && h.ld >= h.V && (!h.has_dlogits || (h.ldd % 8 == 0 && h.ldd >= h.V));
  if (h.has_teacher)
    GPT2MI_REQUIRE(ok && h.ldt % 8 == 0 && h.ldt >= h.V,
                   "%s_fwd: row strides must be multiples of 8 and >= V (ld=%d ldt=%d ldd=%d V=%d)", head, h.ld, h.ldt,
                   h.ldd, h.V);
  GPT2MI_REQUIRE(ok, "%s_fwd: row strides must be multiples of 8 and >= V (ld=%d ldd=%d V=%d)", head, h.ld, h.ldd, h.V);
  const int widest = max(max(h.ld, h.has_teacher ? h.ldt : 0), h.has_dlogits ? h.ldd : 0);
  const bool resident = h.bf16_logits && (widest + 8 * 1024 - 1) / (8 * 1024) == 7;
  if (resident)
    row();
  else
    strided();
  char what[32];
  snprintf(what, sizeof what, "%s_%s", head, resident ? "row" : "fwd");
  int rc = gpt2mi::check_launch(what);
  if (rc) return rc;
  head_finalize_kernel<NM><<<1, 1024, 0, s>>>(loss_rows, labels, M, ignore_index, loss, inv_count, m);
  snprintf(what, sizeof what, "%s_finalize", head);
  return gpt2mi::check_launch(what);
}

}  // namespace
