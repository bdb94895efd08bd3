// Policy-gradient head (PPO-clip / GRPO / REINFORCE): the loss rows and dlogits of
//   loss = -(1/N) sum_rows ( min(r A, clamp(r, 1 - clip_low, 1 + clip_high) A) - kl_coef k3 + entropy_coef H )
// in one pass over the logits, a sibling of the fused cross entropy (csrc/xent_adamw.hip) with the same outputs for the
// backward: dlogits unscaled (bf16 or fp32), loss = mean, inv_count = 1/N (the alpha of the lm_head backward GEMMs).
// What the heads share (the packed row, the workgroup reductions, the store sweep's frame, the finalize kernel and the
// choice of kernel) is csrc/loss_head.h; here is the rule.
// The rule in plain torch: gpt_2_distributed_amd/policy.py (policy_reference). Per row with label y:
//   logp = logit[y] - lse            r = exp(logp - old)   (old = NULL: r = 1 exactly)
//   d = ref - logp, k3 = exp(d) - d - 1                     H = -sum_v p_v log p_v = log S - sum_v e_v (l_v - m) / S
//   dlogits_v = c (p_v - [v = y]) + entropy_coef p_v (log p_v + H),
//   c = (r A if the unclipped term is the minimum (ties included), else 0) + kl_coef (exp(d) - 1)
// with e_v = exp(l_v - m), S = sum_v e_v. No atomics anywhere: two calls give the same bits.
#include <math.h>

#include "common.h"
#include "loss_head.h"

namespace {

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

// One element of dlogits in fp32: x = l - lse = log p, k0 = c + entropy_coef H.
__device__ __forceinline__ float policy_grad(float x, float k0, float ent_coef) {
  return __expf(x) * fmaf(ent_coef, floored(x), k0);
}

// --- the register-resident row kernel (bf16, GPT-2's vocabulary) ----------------------------------------------------
// One 1024-thread workgroup per row, the row held packed in registers (loss_head.h's PackedRow) between three sweeps
// over it, read from HBM once and fenced so that the unpacked values of one sweep are dead before the next (61 VGPRs:
// two workgroups per CU). Sweep 1: the maximum. Sweep 2: S = sum e and T = sum e (l - m) together, two
// accumulators fed by one exp, reduced by one LDS exchange that carries both. Thread 0 forms the row's scalars and
// broadcasts (lse, c, H); they are wave-uniform, so they live in SGPRs during sweep 3, which writes
// bf16(p (c + entropy_coef (log p + H)) - c [v = y]), every element formed in fp32 and rounded once.
template <int NCH>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8)))
void policy_row_kernel(const bf16* __restrict__ logits, int ld, bf16* __restrict__ dlogits, int ldd, PolicyRows a) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const int V = a.V;
  const bf16* lp = logits + (size_t)row * ld;
  __shared__ float red[2][16];
  __shared__ float s_bcast[3];
  PackedRow<NCH> r;
  r.load(lp, ld, V, tid);
  float mv[1] = {-INFINITY};
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) mv[0] = fmaxf(mv[0], r.val(i, j));
  r.fence();
  group_max(mv, red, s_bcast, tid);
  const float mx = uniform(mv[0]);
  float st[2] = {0.f, 0.f};  // S, T
#pragma unroll
  for (int i = 0; i < NCH; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float d = r.val(i, j) - mx, e = __expf(d);  // the padding: d = -inf, e = 0
      st[0] += e;
      st[1] = fmaf(e, floored(d), st[1]);
    }
  r.fence();
  __syncthreads();  // not needed for red or s_bcast: without it the kernel takes 64 VGPRs and spills 364 bytes a lane
  group_sum_wave0(st, red, tid);
  const int64_t y = a.labels[row];
  if (tid == 0) {
    const float ly = (y >= 0 && y < V) ? bf2f(lp[y]) - mx : 0.f;
    float c, H;
    policy_row_scalars(a, row, y, ly, st[0], st[1], &c, &H);
    s_bcast[0] = mx + logf(st[0]);
    s_bcast[1] = c;
    s_bcast[2] = H;
  }
  __syncthreads();
  if (!dlogits) return;
  const float lse = uniform(s_bcast[0]), c = uniform(s_bcast[1]);
  const float k0 = fmaf(a.ent_coef, uniform(s_bcast[2]), c);
  store_row<NCH>(
      dlogits + (size_t)row * ldd, ldd, V, tid, y == a.ignore_index, y, c,
      [&](float l) { return policy_grad(l - lse, k0, a.ent_coef); }, r);
}

// --- the strided two-pass kernel (fp32 logits, or any V) ---------------------------------------------------------------

// (m, s, t) = (max, sum e^(l - m), sum e^(l - m) (l - m)) of two disjoint sets of logits merged; an empty set is
// (-inf, 0, 0). Moving a set's reference from m to nm: s -> a s, t -> a (t + (m - nm) s), a = e^(m - nm).
__device__ __forceinline__ void mst_merge(float& m, float& s, float& t, float om, float os, float ot) {
  const float nm = fmaxf(m, om);
  const float da = m - nm, db = om - nm;
  const float ea = (m == -INFINITY) ? 0.f : __expf(da), eb = (om == -INFINITY) ? 0.f : __expf(db);
  t = ea * fmaf(floored(da), s, t) + eb * fmaf(floored(db), os, ot);
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
      ct = fmaf(e, floored(d), ct);
    }
    const float dm = m - nm, em = __expf(dm);  // first trip: m = -inf, em = 0, s = t = 0
    t = em * fmaf(floored(dm), s, t) + ct;
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
  GPT2MI_REQUIRE(clip_low >= 0.f && clip_high >= 0.f, "policy_fwd: clip_low=%g and clip_high=%g must be >= 0",
                 (double)clip_low, (double)clip_high);
  GPT2MI_REQUIRE(isfinite(kl_coef) && isfinite(entropy_coef), "policy_fwd: kl_coef=%g and entropy_coef=%g must be finite",
                 (double)kl_coef, (double)entropy_coef);
  GPT2MI_REQUIRE(!metrics || (ratio && kl && entropy && clipped),
                 "policy_fwd: metrics are the means of the per-row ratio, kl, entropy and clipped outputs: pass all four");
  hipStream_t s = (hipStream_t)stream;
  const PolicyRows a{labels,    advantages, old_logprobs, ref_logprobs, clip_low, clip_high, kl_coef, entropy_coef,
                     loss_rows, logp,       ratio,        kl,           entropy,  clipped,   V,       ignore_index};
  auto row = [&] {
    if constexpr (sizeof(TL) == 2) policy_row_kernel<7><<<M, 1024, 0, s>>>(logits, ld, dlogits, ldd, a);
  };
  auto strided = [&] { policy_fwd_kernel<TL><<<M, 256, 0, s>>>(logits, ld, dlogits, ldd, a); };
  // metrics = the means over the counted rows of (ratio, clipped, k3, H)
  return head_launch<4>("policy", {ld, 0, ldd, V, false, dlogits != nullptr, sizeof(TL) == 2}, row, strided, loss_rows,
                        labels, M, ignore_index, loss, inv_count, {{ratio, clipped, kl, entropy}, metrics}, s);
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
