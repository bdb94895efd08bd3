// Distillation head: the loss rows and dlogits of
//   loss = (1/N) sum_rows ( ce_coef ce + kd_coef kd ),   ce = -log p[y],   kd = tau^2 KL(q || p_tau)  (forward, Hinton)
//                                                                           or tau^2 KL(p_tau || q)  (reverse)
// with p = softmax(s), p_tau = softmax(s / tau), q = softmax(t / tau) over the student logits s and the teacher logits t,
// in one read of both rows and one write, a sibling of the fused cross entropy (csrc/xent_adamw.hip) and of the policy
// head (csrc/policy_loss.hip) with the same outputs for the backward: dlogits unscaled (bf16 or fp32), loss = mean,
// inv_count = 1/N (the alpha of the lm_head backward GEMMs). The rule in plain torch: gpt_2_distributed_amd/distill.py
// (distill_reference). What the heads share (the packed row, the workgroup reductions, the store sweep's frame, the
// finalize kernel and the choice of kernel) is csrc/loss_head.h; here is the rule. Per row, it = 1 / tau:
//   forward:  dlogits_v = ce_coef (p_v - [v = y]) + kd_coef tau (p_tau_v - q_v)
//   reverse:  dlogits_v = ce_coef (p_v - [v = y]) + kd_coef tau p_tau_v (log p_tau_v - log q_v - KL(p_tau || q))
// The row's reductions, m = max s, mt = max t (the maximum of s serves tau = 1 and tau alike):
//   S1 = sum e^(s - m)    St = sum e^((s - m) it)    Q = sum e^((t - mt) it)
//   X  = sum e^((t - mt) it) (t - s)  (forward)   or   sum e^((s - m) it) (s - t)  (reverse)
//   KL(q || p_tau) = it (X / Q - (mt - m)) - log Q + log St      KL(p_tau || q) = it (X / St - (m - mt)) - log St + log Q
// tau == 1 and the direction are compile-time: at tau = 1 St is S1 and p_tau is p, so a sweep pays two exps an element
// (forward) or one (reverse's third sweep), not three. No atomics anywhere: two calls give the same bits.
// kd is a small difference of O(1) terms (at tau = 2 a KL of 0.03 from logs of 5, then times tau^2), so only the
// per-thread partial sums are fp32, where a thread's rounding errors are independent of the others' and average out
// over the workgroup: across lanes and waves the sums are added in fp64, and the one thread that forms the row's
// scalars takes its logs in fp64 (a few hundred instructions a row, beside 50k elements).
#include <math.h>

#include "common.h"
#include "loss_head.h"

namespace {

// What a row's thread 0 reads and writes beside the logits; by value to every kernel.
struct DistillRows {
  const int64_t* labels;
  float tau, inv_tau, ce_coef, kd_coef;
  float *loss_rows, *ce, *kd;  // [M]; ce, kd may be NULL
  int V, ignore_index;
};

// A thread's share of the row's reductions, as the sweeps and the online merge carry it.
struct DistillSums {
  float m, mt, S1, St, Q, X;
};
// The whole row's, summed across the workgroup in fp64.
struct DistillRowSums {
  float m, mt;
  double S1, St, Q, X;
};

// What the third sweep needs of a row, wave-uniform: lse = log sum e^s, lset = log sum e^(s it), lseq = log sum e^(t it),
// and the reverse direction's KL. A bad label makes them NaN, which poisons every element of the row.
struct DistillBcast {
  float lse, lset, lseq, kl;
};

// The row's scalars from its reductions, by one thread; sy = the label's student logit. Stores the per-row outputs. An
// ignored row stores zeros; a label outside [0, V) stores NaN and returns NaN (F.cross_entropy raises on such a label).
template <bool TAU1, bool REV>
__device__ __forceinline__ DistillBcast distill_row_scalars(const DistillRows& a, int row, int64_t y, float sy,
                                                            const DistillRowSums& r) {
  const double tau = TAU1 ? 1.0 : (double)a.tau, m = r.m, mt = r.mt;
  const double logS1 = log(r.S1), logSt = TAU1 ? logS1 : log(r.St), logQ = log(r.Q);
  const double KL = REV ? (r.X / (TAU1 ? r.S1 : r.St) - (m - mt)) / tau - logSt + logQ
                        : (r.X / r.Q - (mt - m)) / tau - logQ + logSt;
  DistillBcast b{(float)(m + logS1), (float)(m / tau + logSt), (float)(mt / tau + logQ), (float)KL};
  float loss = 0.f, ce = 0.f, kd = 0.f;
  if (y != a.ignore_index) {
    if (y < 0 || y >= a.V) {
      loss = ce = kd = b.lse = b.lset = b.lseq = b.kl = __builtin_nanf("");
    } else {
      const double ce64 = logS1 - ((double)sy - m), kd64 = tau * tau * KL;
      ce = (float)ce64;
      kd = (float)kd64;
      loss = (float)((double)a.ce_coef * ce64 + (double)a.kd_coef * kd64);
    }
  }
  a.loss_rows[row] = loss;
  if (a.ce) a.ce[row] = ce;
  if (a.kd) a.kd[row] = kd;
  return b;
}

// The element coefficients of the third sweep, wave-uniform: formed once from the broadcast scalars.
struct DistillCoef {
  float lse, lset, lseq, it;
  float c0, c1, c2;  // forward: c0 p + c1 p_tau - c1 q (tau = 1: c0 p - c1 q); reverse: c0 p + c1 p_tau (lp_tau - lq - c2)
};

template <bool TAU1, bool REV>
__device__ __forceinline__ DistillCoef distill_coef(const DistillRows& a, const DistillBcast& b) {
  const float kt = TAU1 ? a.kd_coef : a.kd_coef * a.tau;
  if (REV) return {b.lse, b.lset, b.lseq, TAU1 ? 1.f : a.inv_tau, a.ce_coef, kt, b.kl};
  return {b.lse, b.lset, b.lseq, TAU1 ? 1.f : a.inv_tau, TAU1 ? a.ce_coef + kt : a.ce_coef, kt, 0.f};
}

// One element of dlogits in fp32, without the label's -ce_coef.
template <bool TAU1, bool REV>
__device__ __forceinline__ float distill_grad(float s, float t, const DistillCoef& k) {
  if constexpr (REV) {
    if constexpr (TAU1) {
      const float lp = s - k.lse, lq = t - k.lseq;
      return __expf(lp) * fmaf(k.c1, floored(lp) - floored(lq) - k.c2, k.c0);
    } else {
      const float lp = fmaf(s, k.it, -k.lset), lq = fmaf(t, k.it, -k.lseq);
      return fmaf(k.c0, __expf(s - k.lse), k.c1 * __expf(lp) * (floored(lp) - floored(lq) - k.c2));
    }
  } else {
    if constexpr (TAU1) {
      return fmaf(k.c0, __expf(s - k.lse), -k.c1 * __expf(t - k.lseq));
    } else {
      const float d = __expf(fmaf(s, k.it, -k.lset)) - __expf(fmaf(t, k.it, -k.lseq));
      return fmaf(k.c0, __expf(s - k.lse), k.c1 * d);
    }
  }
}

// One element's share of the sums, ds = s - m and dt = t - mt (-inf in the padding: every e is 0 there).
template <bool TAU1, bool REV>
__device__ __forceinline__ void distill_accumulate(float s, float t, float ds, float dt, float it, float& S1, float& St,
                                                   float& Q, float& X) {
  const float e1 = __expf(ds);
  const float eq = __expf(TAU1 ? dt : dt * it);
  S1 += e1;
  Q += eq;
  float et = e1;
  if constexpr (!TAU1) {
    et = __expf(ds * it);
    St += et;
  }
  const float diff = floored(t) - floored(s);
  X = REV ? fmaf(et, -diff, X) : fmaf(eq, diff, X);
}

// --- the register-resident two-row kernel (bf16, GPT-2's vocabulary) ------------------------------------------------
// One 1024-thread workgroup per row; the student row AND the teacher row are held packed in registers (two of
// loss_head.h's PackedRow, 4 VGPRs a chunk of 8: 56 VGPRs at NCH = 7) between three sweeps, each read from HBM exactly once and
// fenced so that the unpacked values of one sweep are dead before the next. One workgroup is 4 waves on each SIMD; 56
// packed registers leave no room for a second one (64 VGPRs a wave), so the kernel asks for 4 waves per SIMD and may
// use 128 VGPRs. Sweep 1: both maxima, one LDS exchange. Sweep 2: S1, (St,) Q and X together from the unpacked values,
// one LDS exchange that carries them all, added by wave 0's butterfly in a fixed order. Thread 0 forms the row's
// scalars, stores the per-row outputs and broadcasts (lse, lset, lseq, KL); they are wave-uniform, so they live in
// SGPRs during sweep 3, which writes dlogits once, every element formed in fp32 and rounded once.
template <int NCH, bool TAU1, bool REV>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4, 4)))
void distill_row_kernel(const bf16* __restrict__ logits, int ld, const bf16* __restrict__ teacher, int ldt,
                        bf16* __restrict__ dlogits, int ldd, DistillRows a) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const int V = a.V;
  const float it = TAU1 ? 1.f : a.inv_tau;
  const bf16* sp = logits + (size_t)row * ld;
  __shared__ float red[2][16];
  __shared__ double red64[4][16];
  __shared__ float s_bcast[4];
  PackedRow<NCH> rs, rt;
  rs.load(sp, ld, V, tid);
  rt.load(teacher + (size_t)row * ldt, ldt, V, tid);
  float mv[2] = {-INFINITY, -INFINITY};  // m, mt
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mv[0] = fmaxf(mv[0], rs.val(i, j));
      mv[1] = fmaxf(mv[1], rt.val(i, j));
    }
  rs.fence();
  rt.fence();
  group_max(mv, red, s_bcast, tid);
  const float mx = uniform(mv[0]), mxt = uniform(mv[1]);
  float S1 = 0.f, St = 0.f, Q = 0.f, X = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float s = rs.val(i, j), t = rt.val(i, j);
      distill_accumulate<TAU1, REV>(s, t, s - mx, t - mxt, it, S1, St, Q, X);
    }
  rs.fence();
  rt.fence();
  constexpr int NS = TAU1 ? 3 : 4;  // at tau = 1 St is S1
  double sums[NS] = {S1, Q, X};
  if constexpr (!TAU1) sums[3] = St;
  group_sum_wave0(sums, red64, tid);  // (s_bcast[0..1] consumed before its barrier: the row's scalars are written after)
  const int64_t y = a.labels[row];
  if (tid == 0) {
    const DistillRowSums r{mx, mxt, sums[0], sums[TAU1 ? 0 : NS - 1], sums[1], sums[2]};
    const float sy = (y >= 0 && y < V) ? bf2f(sp[y]) : 0.f;
    const DistillBcast b = distill_row_scalars<TAU1, REV>(a, row, y, sy, r);
    s_bcast[0] = b.lse;
    s_bcast[1] = b.lset;
    s_bcast[2] = b.lseq;
    s_bcast[3] = b.kl;
  }
  __syncthreads();
  if (!dlogits) return;
  const DistillCoef k = distill_coef<TAU1, REV>(
      a, DistillBcast{uniform(s_bcast[0]), uniform(s_bcast[1]), uniform(s_bcast[2]), uniform(s_bcast[3])});
  store_row<NCH>(
      dlogits + (size_t)row * ldd, ldd, V, tid, y == a.ignore_index, y, a.ce_coef,
      [&](float s, float t) { return distill_grad<TAU1, REV>(s, t, k); }, rs, rt);
}

// --- the strided two-pass kernel (fp32 logits, or any V) ---------------------------------------------------------------
// e^((from - to) it) for a maximum that moves from `from` to `to` >= from; an empty set (from = -inf) scales by 0
// whatever `to` is, so a set of nothing but -inf logits merges cleanly too.
__device__ __forceinline__ float rescale(float from, float to, float it) {
  return (from == -INFINITY) ? 0.f : __expf((from - to) * it);
}

// Two disjoint sets' states merged; an empty set is (-inf, -inf, 0, 0, 0, 0). Each sum rescales by its own factor:
// S1 by e^(dm), St by e^(dm it), Q by e^(dmt it), and X by that of the exponential it carries.
template <bool TAU1, bool REV>
__device__ __forceinline__ void distill_merge(DistillSums& p, const DistillSums& o, float it) {
  const float nm = fmaxf(p.m, o.m), nmt = fmaxf(p.mt, o.mt);
  const float a1 = rescale(p.m, nm, 1.f), b1 = rescale(o.m, nm, 1.f);
  const float at = TAU1 ? a1 : rescale(p.m, nm, it), bt = TAU1 ? b1 : rescale(o.m, nm, it);
  const float aq = rescale(p.mt, nmt, it), bq = rescale(o.mt, nmt, it);
  p.S1 = a1 * p.S1 + b1 * o.S1;
  p.St = at * p.St + bt * o.St;
  p.Q = aq * p.Q + bq * o.Q;
  p.X = REV ? at * p.X + bt * o.X : aq * p.X + bq * o.X;
  p.m = nm;
  p.mt = nmt;
}

// One 256-thread workgroup per row. Pass 1: the state online per thread over 16-byte chunks of both rows, each chunk
// merged into it; then the workgroup's two maxima, every thread's state moved to them by one more merge (a thread
// that saw nothing is the empty set), and the sums added across the lanes and the four waves in fp64 in a fixed order;
// thread 0 forms the row's scalars. Pass 2 reads both rows again and writes dlogits.
template <typename TL, bool TAU1, bool REV>
__global__ __launch_bounds__(256) void distill_fwd_kernel(const TL* __restrict__ logits, int ld,
                                                          const TL* __restrict__ teacher, int ldt,
                                                          TL* __restrict__ dlogits, int ldd, DistillRows a) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const int V = a.V;
  const float it = TAU1 ? 1.f : a.inv_tau;
  const TL* sp = logits + (size_t)row * ld;
  const TL* tp = teacher + (size_t)row * ldt;
  DistillSums r{-INFINITY, -INFINITY, 0.f, 0.f, 0.f, 0.f};
  for (int c = 8 * tid; c < V; c += 8 * 256) {
    float s[8], t[8];
    load8<TL>(sp + c, s);
    load8<TL>(tp + c, t);
    DistillSums ch{-INFINITY, -INFINITY, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // the padding of both rows: -inf before anything is formed from it
      s[j] = (c + j < V) ? s[j] : -INFINITY;
      t[j] = (c + j < V) ? t[j] : -INFINITY;
      ch.m = fmaxf(ch.m, s[j]);
      ch.mt = fmaxf(ch.mt, t[j]);
    }
    // a chunk of nothing but -inf (masked tokens) is measured from 0: every e is 0, none is e^(-inf + inf)
    const float cm = (ch.m == -INFINITY) ? 0.f : ch.m, cmt = (ch.mt == -INFINITY) ? 0.f : ch.mt;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      distill_accumulate<TAU1, REV>(s[j], t[j], s[j] - cm, t[j] - cmt, it, ch.S1, ch.St, ch.Q, ch.X);
    distill_merge<TAU1, REV>(r, ch, it);
  }
  __shared__ float smax[2][4];
  __shared__ double sm[4][4];
  __shared__ float s_bcast[4];
  const float wm = wave_max(r.m), wmt = wave_max(r.mt);
  if ((tid & 63) == 0) {
    smax[0][tid >> 6] = wm;
    smax[1][tid >> 6] = wmt;
  }
  __syncthreads();
  const float gm = fmaxf(fmaxf(smax[0][0], smax[0][1]), fmaxf(smax[0][2], smax[0][3]));
  const float gmt = fmaxf(fmaxf(smax[1][0], smax[1][1]), fmaxf(smax[1][2], smax[1][3]));
  distill_merge<TAU1, REV>(r, DistillSums{gm, gmt, 0.f, 0.f, 0.f, 0.f}, it);
  const double wS1 = wave_sum_f64(r.S1), wSt = wave_sum_f64(r.St), wQ = wave_sum_f64(r.Q), wX = wave_sum_f64(r.X);
  if ((tid & 63) == 0) {
    sm[0][tid >> 6] = wS1;
    sm[1][tid >> 6] = wSt;
    sm[2][tid >> 6] = wQ;
    sm[3][tid >> 6] = wX;
  }
  __syncthreads();
  const int64_t y = a.labels[row];
  if (tid == 0) {
    DistillRowSums R{gm, gmt, sm[0][0], sm[1][0], sm[2][0], sm[3][0]};
    for (int k = 1; k < 4; ++k) {
      R.S1 += sm[0][k];
      R.St += sm[1][k];
      R.Q += sm[2][k];
      R.X += sm[3][k];
    }
    if (TAU1) R.St = R.S1;
    const float sy = (y >= 0 && y < V) ? (float)sp[y] : 0.f;
    const DistillBcast b = distill_row_scalars<TAU1, REV>(a, row, y, sy, R);
    s_bcast[0] = b.lse;
    s_bcast[1] = b.lset;
    s_bcast[2] = b.lseq;
    s_bcast[3] = b.kl;
  }
  __syncthreads();
  if (!dlogits) return;
  const bool ign = (y == a.ignore_index);
  const DistillCoef k = distill_coef<TAU1, REV>(
      a, DistillBcast{uniform(s_bcast[0]), uniform(s_bcast[1]), uniform(s_bcast[2]), uniform(s_bcast[3])});
  TL* dp = dlogits + (size_t)row * ldd;
  for (int c0 = 8 * tid; c0 < ldd; c0 += 8 * 256) {
    float o[8];
    if (c0 < V && !ign) {
      float s[8], t[8];
      load8<TL>(sp + c0, s);
      load8<TL>(tp + c0, t);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool in = c0 + j < V;  // the padding of either row never reaches a product
        const float g = distill_grad<TAU1, REV>(in ? s[j] : -INFINITY, in ? t[j] : -INFINITY, k);
        o[j] = in ? g - ((c0 + j == y) ? a.ce_coef : 0.f) : 0.f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = 0.f;
    }
    store8<TL>(dp + c0, o);
  }
}

template <typename TL, bool TAU1, bool REV>
int distill_launch(const TL* logits, int ld, const TL* teacher, int ldt, TL* dlogits, int ldd, int M,
                   const DistillRows& a, float* loss, float* inv_count, float* metrics, hipStream_t s) {
  auto row = [&] {
    if constexpr (sizeof(TL) == 2)
      distill_row_kernel<7, TAU1, REV><<<M, 1024, 0, s>>>(logits, ld, teacher, ldt, dlogits, ldd, a);
  };
  auto strided = [&] {
    distill_fwd_kernel<TL, TAU1, REV><<<M, 256, 0, s>>>(logits, ld, teacher, ldt, dlogits, ldd, a);
  };
  // metrics = the means over the counted rows of (ce, kd)
  return head_launch<2>("distill", {ld, ldt, ldd, a.V, true, dlogits != nullptr, sizeof(TL) == 2}, row, strided,
                        a.loss_rows, a.labels, M, a.ignore_index, loss, inv_count, {{a.ce, a.kd}, metrics}, s);
}

}  // namespace

template <typename TL>
static int distill_fwd_t(const TL* logits, int ld, const TL* teacher, int ldt, const int64_t* labels, float temperature,
                         float ce_coef, float kd_coef, int reverse, float* loss_rows, float* ce, float* kd, TL* dlogits,
                         int ldd, int M, int V, int ignore_index, float* loss, float* inv_count, float* metrics,
                         void* stream) {
  GPT2MI_REQUIRE(M >= 1 && V >= 1, "distill_fwd: M=%d and V=%d must be >= 1", M, V);
  GPT2MI_REQUIRE(logits && teacher && labels && loss_rows && loss && inv_count,
                 "distill_fwd: logits, teacher, labels, loss_rows, loss and inv_count must not be NULL");
  GPT2MI_REQUIRE(isfinite(temperature) && temperature > 0.f, "distill_fwd: temperature=%g must be finite and > 0",
                 (double)temperature);
  GPT2MI_REQUIRE(isfinite(ce_coef) && isfinite(kd_coef), "distill_fwd: ce_coef=%g and kd_coef=%g must be finite",
                 (double)ce_coef, (double)kd_coef);
  GPT2MI_REQUIRE(reverse == 0 || reverse == 1, "distill_fwd: reverse=%d must be 0 (forward KL) or 1", reverse);
  GPT2MI_REQUIRE(!metrics || (ce && kd), "distill_fwd: metrics are the means of the per-row ce and kd outputs: pass both");
  hipStream_t s = (hipStream_t)stream;
  const DistillRows a{labels, temperature, 1.f / temperature, ce_coef, kd_coef, loss_rows, ce, kd, V, ignore_index};
  auto launch = temperature == 1.f ? (reverse ? distill_launch<TL, true, true> : distill_launch<TL, true, false>)
                                   : (reverse ? distill_launch<TL, false, true> : distill_launch<TL, false, false>);
  return launch(logits, ld, teacher, ldt, dlogits, ldd, M, a, loss, inv_count, metrics, s);
}

GPT2MI_EXPORT int gpt2mi_distill_fwd(const uint16_t* logits, int ld, const uint16_t* teacher, int ldt,
                                     const int64_t* labels, float temperature, float ce_coef, float kd_coef, int reverse,
                                     float* loss_rows, float* ce, float* kd, uint16_t* dlogits, int ldd, int M, int V,
                                     int ignore_index, float* loss, float* inv_count, float* metrics, void* stream) {
  return distill_fwd_t<bf16>((const bf16*)logits, ld, (const bf16*)teacher, ldt, labels, temperature, ce_coef, kd_coef,
                             reverse, loss_rows, ce, kd, (bf16*)dlogits, ldd, M, V, ignore_index, loss, inv_count,
                             metrics, stream);
}

GPT2MI_EXPORT int gpt2mi_distill_fwd_f32(const float* logits, int ld, const float* teacher, int ldt,
                                         const int64_t* labels, float temperature, float ce_coef, float kd_coef,
                                         int reverse, float* loss_rows, float* ce, float* kd, float* dlogits, int ldd,
                                         int M, int V, int ignore_index, float* loss, float* inv_count, float* metrics,
                                         void* stream) {
  return distill_fwd_t<float>(logits, ld, teacher, ldt, labels, temperature, ce_coef, kd_coef, reverse, loss_rows, ce,
                              kd, dlogits, ldd, M, V, ignore_index, loss, inv_count, metrics, stream);
}
