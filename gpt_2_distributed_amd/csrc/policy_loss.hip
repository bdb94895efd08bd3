// Policy-gradient head (PPO-clip / GRPO / REINFORCE): the loss rows and dlogits of
//   loss = -(1/N) sum_rows ( min(r A, clamp(r, 1 - clip_low, 1 + clip_high) A) - kl_coef k3 + entropy_coef H )
// in one pass over the logits, a sibling of the fused cross entropy (csrc/xent_adamw.hip) with the same outputs for the
// backward: dlogits unscaled (bf16 or fp32), loss = mean, inv_count = 1/N (the alpha of the lm_head backward GEMMs).
// The rule in plain torch: gpt_2_distributed_amd/policy.py (policy_reference). Per row with label y:
//   logp = logit[y] - lse            r = exp(logp - old)   (old = NULL: r = 1 exactly)
//   d = ref - logp, k3 = exp(d) - d - 1                     H = -sum_v p_v log p_v = log S - sum_v e_v (l_v - m) / S
//   dlogits_v = c (p_v - [v = y]) + entropy_coef p_v (log p_v + H),
//   c = (r A if the unclipped term is the minimum (ties included), else 0) + kl_coef (exp(d) - 1)
// with e_v = exp(l_v - m), S = sum_v e_v. No atomics anywhere: two calls give the same bits.
#include <math.h>

#include "common.h"

namespace {

// log p of a column that holds -inf (the padding as the reductions see it, or a masked logit) is floored before it is
// multiplied by that column's p = 0: 0 * floor = 0 where 0 * -inf would put a NaN into a good row's entropy
constexpr float kLogFloor = -1e30f;

// What a row's thread 0 reads and writes beside the logits; by value to every kernel.
struct PolicyRows {
  const int64_t* labels;
  const float *adv, *old_lp, *ref_lp;  // [M]; old_lp, ref_lp may be NULL
  float clip_low, clip_high, kl_coef, ent_coef;
  float *loss_rows, *logp, *ratio, *kl, *entropy, *clipped;  // [M]; all but loss_rows may be NULL
  int V, ignore_index;
};

// The row's scalars from its reductions, by one thread: ly = logit[y] - m, S = sum e, T = sum e (l - m). Stores the
// per-row outputs, returns c and H. An ignored row stores zeros; a label outside [0, V) stores NaN and returns c = NaN,
// which poisons the row's dlogits (F.cross_entropy raises on such a label).
__device__ __forceinline__ void policy_row_scalars(const PolicyRows& a, int row, int64_t y, float ly, float S, float T,
                                                   float* c_out, float* H_out) {
  const float logS = logf(S);
  const float H = logS - T / S;
  float loss = 0.f, logp = 0.f, r = 0.f, k3 = 0.f, ent = 0.f, cl = 0.f, c = 0.f;
  if (y != a.ignore_index) {
    if (y < 0 || y >= a.V) {
      loss = logp = r = k3 = ent = cl = c = __builtin_nanf("");
    } else {
      logp = ly - logS;
      ent = H;
      const float A = a.adv[row];
      r = a.old_lp ? expf(logp - a.old_lp[row]) : 1.f;
      const float rc = fminf(fmaxf(r, 1.f - a.clip_low), 1.f + a.clip_high);
      cl = (rc != r) ? 1.f : 0.f;
      const float u = r * A, v = rc * A;
      const bool active = u <= v;  // a tie counts for the unclipped term
      float s = active ? u : v;
      c = active ? u : 0.f;
      if (a.ref_lp) {
        const float d = a.ref_lp[row] - logp, em1 = expm1f(d);
        k3 = em1 - d;
        if (a.kl_coef != 0.f) {
          s -= a.kl_coef * k3;
          c += a.kl_coef * em1;
        }
      }
      loss = -(s + a.ent_coef * H);
    }
  }
  a.loss_rows[row] = loss;
  if (a.logp) a.logp[row] = logp;
  if (a.ratio) a.ratio[row] = r;
  if (a.kl) a.kl[row] = k3;
  if (a.entropy) a.entropy[row] = ent;
  if (a.clipped) a.clipped[row] = cl;
  *c_out = c;
  *H_out = H;
}

__device__ __forceinline__ float uniform(float x) {  // a value every lane holds, into an SGPR
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

// One element of dlogits in fp32: x = l - lse = log p, k0 = c + entropy_coef H.
__device__ __forceinline__ float policy_grad(float x, float k0, float ent_coef) {
  return __expf(x) * fmaf(ent_coef, fmaxf(x, kLogFloor), k0);
}

// --- the register-resident row kernel (bf16, GPT-2's vocabulary) ----------------------------------------------------
// xent_row_kernel's plan: one 1024-thread workgroup per row, the row held packed in registers (NCH chunks of 8 logits
// per thread, 4 VGPRs a chunk) between three sweeps over it, read from HBM once and fenced so that the unpacked values
// of one sweep are dead before the next. Sweep 1: the maximum. Sweep 2: S = sum e and T = sum e (l - m) together, two
// accumulators fed by one exp, reduced by one LDS exchange that carries both. Thread 0 forms the row's scalars and
// broadcasts (lse, c, H); they are wave-uniform, so they live in SGPRs during sweep 3, which writes
// bf16(p (c + entropy_coef (log p + H)) - c [v = y]), every element formed in fp32 and rounded once.
template <int NCH>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8)))
void policy_row_kernel(const bf16* __restrict__ logits, int ld, bf16* __restrict__ dlogits, int ldd, PolicyRows a) {
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V;
  const bf16* lp = logits + (size_t)row * ld;
  __shared__ float red[32];
  __shared__ float s_bcast[3];
  bf16x8 raw[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = 8 * (tid + 1024 * i);
    raw[i] = c < ld ? *reinterpret_cast<const bf16x8*>(lp + c) : bf16x8{};
    if (c + 8 > V) {  // the padding (and the unread tail) never wins the max and has exp(.) = 0
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (c + j >= V) raw[i][j] = (bf16)(-INFINITY);
    }
  }
  auto val = [&](int i, int j) { return bf2f(raw[i][j]); };
  auto fence = [&]() {  // the row stays packed between the sweeps (see xent_row_kernel)
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      u32x4 t = __builtin_bit_cast(u32x4, raw[i]);
      asm volatile("" : "+v"(t));
      raw[i] = __builtin_bit_cast(bf16x8, t);
    }
  };
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, val(i, j));
  fence();
  m = wave_max(m);
  if (lane == 0) red[w] = m;
  __syncthreads();
  if (tid == 0) {
    float t = red[0];
    for (int k = 1; k < 16; ++k) t = fmaxf(t, red[k]);
    s_bcast[0] = t;
  }
  __syncthreads();
  const float mx = uniform(s_bcast[0]);
  float sum = 0.f, tsum = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = val(i, j) - mx, e = __expf(d);  // the padding: d = -inf, e = 0
      sum += e;
      tsum = fmaf(e, fmaxf(d, kLogFloor), tsum);
    }
  fence();
  sum = wave_sum(sum);
  tsum = wave_sum(tsum);
  __syncthreads();  // s_bcast[0] consumed
  if (lane == 0) {
    red[w] = sum;
    red[16 + w] = tsum;
  }
  __syncthreads();
  const int64_t y = a.labels[row];
  if (w == 0) {  // the 16 wave sums of both, added by wave 0's butterfly: a fixed order, and no 32 values in one thread
    const float S = wave_sum(lane < 16 ? red[lane] : 0.f), T = wave_sum(lane < 16 ? red[16 + lane] : 0.f);
    if (lane == 0) {
      const float ly = (y >= 0 && y < V) ? bf2f(lp[y]) - mx : 0.f;
      float c, H;
      policy_row_scalars(a, row, y, ly, S, T, &c, &H);
      s_bcast[0] = mx + logf(S);
      s_bcast[1] = c;
      s_bcast[2] = H;
    }
  }
  __syncthreads();
  if (!dlogits) return;
  const bool ign = (y == a.ignore_index);
  const float lse = uniform(s_bcast[0]), c = uniform(s_bcast[1]);
  const float k0 = fmaf(a.ent_coef, uniform(s_bcast[2]), c);
  bf16* dp = dlogits + (size_t)row * ldd;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c0 = 8 * (tid + 1024 * i);
    if (c0 >= ldd) continue;
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(ign ? 0.f : policy_grad(val(i, j) - lse, k0, a.ent_coef));
    if (!ign && (uint32_t)(y - c0) < 8u)  // the label's column again, in fp32 to the end: one rounding
      o[y - c0] = f2bf(policy_grad(bf2f(raw[i][y - c0]) - lse, k0, a.ent_coef) - c);
    if (c0 + 8 > V) {  // +0 in the padding, whatever the sign of c (and in a NaN row)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (c0 + j >= V) o[j] = (bf16)0.f;
    }
    *reinterpret_cast<bf16x8*>(dp + c0) = o;
  }
}

// --- the strided two-pass kernel (fp32 logits, or any V) ---------------------------------------------------------------
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

// (m, s, t) = (max, sum e^(l - m), sum e^(l - m) (l - m)) of two disjoint sets of logits merged; an empty set is
// (-inf, 0, 0). Moving a set's reference from m to nm: s -> a s, t -> a (t + (m - nm) s), a = e^(m - nm).
__device__ __forceinline__ void mst_merge(float& m, float& s, float& t, float om, float os, float ot) {
  const float nm = fmaxf(m, om);
  const float da = m - nm, db = om - nm;
  const float ea = (m == -INFINITY) ? 0.f : __expf(da), eb = (om == -INFINITY) ? 0.f : __expf(db);
  t = ea * fmaf(fmaxf(da, kLogFloor), s, t) + eb * fmaf(fmaxf(db, kLogFloor), os, ot);
  s = ea * s + eb * os;
  m = nm;
}

// One 256-thread workgroup per row. Pass 1: (m, s, t) online per thread over 16-byte chunks, merged across the wave and
// the four waves; thread 0 forms the row's scalars. Pass 2 reads the row again and writes dlogits.
template <typename TL>
__global__ __launch_bounds__(256) void policy_fwd_kernel(const TL* __restrict__ logits, int ld, TL* __restrict__ dlogits,
                                                         int ldd, PolicyRows a) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const int V = a.V;
  const TL* lp = logits + (size_t)row * ld;
  float m = -INFINITY, s = 0.f, t = 0.f;
  for (int c = 8 * tid; c < V; c += 8 * 256) {
    float f[8];
    load8<TL>(lp + c, f);
    float cm = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = (c + j < V) ? f[j] : -INFINITY;
      cm = fmaxf(cm, f[j]);
    }
    const float nm = fmaxf(m, cm);
    float cs = 0.f, ct = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = f[j] - nm, e = __expf(d);
      cs += e;
      ct = fmaf(e, fmaxf(d, kLogFloor), ct);
    }
    const float dm = m - nm, em = __expf(dm);  // first trip: m = -inf, em = 0, s = t = 0
    t = em * fmaf(fmaxf(dm, kLogFloor), s, t) + ct;
    s = em * s + cs;
    m = nm;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    mst_merge(m, s, t, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64), __shfl_xor(t, o, 64));
  __shared__ float sm[4], ss[4], st[4];
  __shared__ float s_bcast[3];
  if ((tid & 63) == 0) {
    sm[tid >> 6] = m;
    ss[tid >> 6] = s;
    st[tid >> 6] = t;
  }
  __syncthreads();
  const int64_t y = a.labels[row];
  if (tid == 0) {
    float M_ = sm[0], S_ = ss[0], T_ = st[0];
    for (int k = 1; k < 4; ++k) mst_merge(M_, S_, T_, sm[k], ss[k], st[k]);
    const float ly = (y >= 0 && y < V) ? (float)lp[y] - M_ : 0.f;
    float c, H;
    policy_row_scalars(a, row, y, ly, S_, T_, &c, &H);
    s_bcast[0] = M_ + logf(S_);
    s_bcast[1] = c;
    s_bcast[2] = H;
  }
  __syncthreads();
  if (!dlogits) return;
  const bool ign = (y == a.ignore_index);
  const float lse = uniform(s_bcast[0]), c = uniform(s_bcast[1]);
  const float k0 = fmaf(a.ent_coef, uniform(s_bcast[2]), c);
  TL* dp = dlogits + (size_t)row * ldd;
  for (int c0 = 8 * tid; c0 < ldd; c0 += 8 * 256) {
    float o[8];
    if (c0 < V && !ign) {
      float v[8];
      load8<TL>(lp + c0, v);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = (c0 + j < V) ? policy_grad(v[j] - lse, k0, a.ent_coef) - ((c0 + j == y) ? c : 0.f) : 0.f;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = 0.f;
    }
    store8<TL>(dp + c0, o);
  }
}

// --- the batch's scalars ------------------------------------------------------------------------------------------------
// One workgroup; every thread adds its rows in row order, the waves and then the 16 wave sums are added in a fixed
// order. loss = sum(loss_rows) / N, inv_count = 1 / N (N = labels != ignore_index; NaN / inf at N = 0, as the cross
// entropy's), metrics = the means over the counted rows of (ratio, clipped, k3, H): ignored rows hold 0 in each.
__global__ __launch_bounds__(1024) void policy_finalize_kernel(const float* __restrict__ loss_rows,
                                                              const int64_t* __restrict__ labels,
                                                              const float* __restrict__ ratio,
                                                              const float* __restrict__ clipped,
                                                              const float* __restrict__ kl,
                                                              const float* __restrict__ entropy, int M, int ignore_index,
                                                              float* __restrict__ loss, float* __restrict__ inv_count,
                                                              float* __restrict__ metrics) {
  constexpr int NQ = 6;
  float q[NQ] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < M; i += 1024) {
    q[0] += loss_rows[i];
    q[1] += (labels[i] == ignore_index) ? 0.f : 1.f;
    if (metrics) {
      q[2] += ratio[i];
      q[3] += clipped[i];
      q[4] += kl[i];
      q[5] += entropy[i];
    }
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
    loss[0] = tot[0] / tot[1];
    inv_count[0] = 1.f / tot[1];
    if (metrics)
      for (int k = 0; k < 4; ++k) metrics[k] = tot[2 + k] / tot[1];
  }
}

}  // namespace

template <typename TL>
static int policy_fwd_t(const TL* logits, int ld, const int64_t* labels, const float* advantages,
                        const float* old_logprobs, const float* ref_logprobs, float clip_low, float clip_high,
                        float kl_coef, float entropy_coef, float* loss_rows, float* logp, float* ratio, float* kl,
                        float* entropy, float* clipped, TL* dlogits, int ldd, int M, int V, int ignore_index, float* loss,
                        float* inv_count, float* metrics, void* stream) {
  GPT2MI_REQUIRE(M >= 1 && V >= 1, "policy_fwd: M=%d and V=%d must be >= 1", M, V);
  GPT2MI_REQUIRE(logits && labels && advantages && loss_rows && loss && inv_count,
                 "policy_fwd: logits, labels, advantages, loss_rows, loss and inv_count must not be NULL");
  GPT2MI_REQUIRE(ld % 8 == 0 && ld >= V && (dlogits == nullptr || (ldd % 8 == 0 && ldd >= V)),
                 "policy_fwd: row strides must be multiples of 8 and >= V (ld=%d ldd=%d V=%d)", ld, ldd, V);
  GPT2MI_REQUIRE(clip_low >= 0.f && clip_high >= 0.f, "policy_fwd: clip_low=%g and clip_high=%g must be >= 0",
                 (double)clip_low, (double)clip_high);
  GPT2MI_REQUIRE(isfinite(kl_coef) && isfinite(entropy_coef), "policy_fwd: kl_coef=%g and entropy_coef=%g must be finite",
                 (double)kl_coef, (double)entropy_coef);
  GPT2MI_REQUIRE(!metrics || (ratio && kl && entropy && clipped),
                 "policy_fwd: metrics are the means of the per-row ratio, kl, entropy and clipped outputs: pass all four");
  hipStream_t s = (hipStream_t)stream;
  const PolicyRows a{labels,    advantages, old_logprobs, ref_logprobs, clip_low, clip_high, kl_coef, entropy_coef,
                     loss_rows, logp,       ratio,        kl,           entropy,  clipped,   V,       ignore_index};
  const int nch = (max(ld, dlogits ? ldd : 0) + 8 * 1024 - 1) / (8 * 1024);
  int rc;
  if (sizeof(TL) == 2 && nch == 7) {  // GPT-2's vocabulary under autocast: the register-resident row
    if constexpr (sizeof(TL) == 2) policy_row_kernel<7><<<M, 1024, 0, s>>>(logits, ld, dlogits, ldd, a);
    rc = gpt2mi::check_launch("policy_row");
  } else {
    policy_fwd_kernel<TL><<<M, 256, 0, s>>>(logits, ld, dlogits, ldd, a);
    rc = gpt2mi::check_launch("policy_fwd");
  }
  if (rc) return rc;
  policy_finalize_kernel<<<1, 1024, 0, s>>>(loss_rows, labels, ratio, clipped, kl, entropy, M, ignore_index, loss,
                                            inv_count, metrics);
  return gpt2mi::check_launch("policy_finalize");
}

GPT2MI_EXPORT int gpt2mi_policy_fwd(const uint16_t* logits, int ld, const int64_t* labels, const float* advantages,
                                    const float* old_logprobs, const float* ref_logprobs, float clip_low,
                                    float clip_high, float kl_coef, float entropy_coef, float* loss_rows, float* logp,
                                    float* ratio, float* kl, float* entropy, float* clipped, uint16_t* dlogits, int ldd,
                                    int M, int V, int ignore_index, float* loss, float* inv_count, float* metrics,
                                    void* stream) {
  return policy_fwd_t<bf16>((const bf16*)logits, ld, labels, advantages, old_logprobs, ref_logprobs, clip_low, clip_high,
                            kl_coef, entropy_coef, loss_rows, logp, ratio, kl, entropy, clipped, (bf16*)dlogits, ldd, M,
                            V, ignore_index, loss, inv_count, metrics, stream);
}

GPT2MI_EXPORT int gpt2mi_policy_fwd_f32(const float* logits, int ld, const int64_t* labels, const float* advantages,
                                        const float* old_logprobs, const float* ref_logprobs, float clip_low,
                                        float clip_high, float kl_coef, float entropy_coef, float* loss_rows,
                                        float* logp, float* ratio, float* kl, float* entropy, float* clipped,
                                        float* dlogits, int ldd, int M, int V, int ignore_index, float* loss,
                                        float* inv_count, float* metrics, void* stream) {
  return policy_fwd_t<float>(logits, ld, labels, advantages, old_logprobs, ref_logprobs, clip_low, clip_high, kl_coef,
                             entropy_coef, loss_rows, logp, ratio, kl, entropy, clipped, dlogits, ldd, M, V,
                             ignore_index, loss, inv_count, metrics, stream);
}
