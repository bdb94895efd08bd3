// The body of the sampling kernels (csrc/sample.hip has the description) and the by-value structs of their arguments.
// Three translation units instantiate it: sample.hip the plain and the penalised kernels, sample_lp.hip the LP ones,
// sample_con.hip the constrained ones. All of it sits in an unnamed namespace: each unit has its own copy and its own
// kernels.
#ifndef GPT2MI_SAMPLE_ROW_H
#define GPT2MI_SAMPLE_ROW_H
#include <limits.h>
#include <math.h>

#include "common.h"
#include "gpt2mi.h"

namespace {

constexpr int SM_THREADS = 1024, SM_WAVES = SM_THREADS / 64, SM_NE = GPT2MI_SAMPLE_MAX_V / SM_THREADS;
static_assert(SM_NE * SM_THREADS == GPT2MI_SAMPLE_MAX_V && SM_NE % 10 == 0, "the row capacity is a whole number of chunks");

// float <-> a uint32 that orders as the float does (-inf = 0x007FFFFF ... +inf = 0xFF800000)
__device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float keyf(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}
// One rounded fp32 operation each, the result pinned in a register: the compiler contracts x - f * c into an fma
// otherwise, and the bits would not be apply_penalties'.
__device__ __forceinline__ float pinned(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// tid behind an empty asm, for a phase outside sample_row (see tid_here there)
__device__ __forceinline__ int tid_pinned() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// The row of a 1024-thread workgroup: thread t's x[i] is logit i * 1024 + t of `row`, NaN for an index >= V (no
// comparison is true for it, fmaxf drops it; the padding columns of the buffer are not read). The one load of
// sample_row and of the beam search's top-W kernel (csrc/beam.hip), so that they hold the same registers.
// Chunk i of the row is read through a raw buffer over its own valid part, [i * 1024, min(V, (i + 1) * 1024)): the
// hardware drops the lanes past it (they get 0; a chunk with nothing valid reads nothing), the descriptor is scalar
// work and the 50 loads share one offset register, so they are all in flight together (50 clamped 64-bit addresses
// would take 100 registers).
__device__ __forceinline__ float load_chunk(const float* row, int V, int i, uint32_t voff) {
  const int n = min(max(V - i * SM_THREADS, 0), SM_THREADS);
  return __builtin_bit_cast(
      float, __builtin_amdgcn_raw_buffer_load_b32(
                 __builtin_amdgcn_make_buffer_rsrc((void*)(row + min(i * SM_THREADS, V - 1)), 0, 4 * n, 0x00020000), voff,
                 0, 0));
}
__device__ __forceinline__ void load_row(float (&x)[SM_NE], const float* row, int V) {
  const uint32_t voff = 4u * threadIdx.x;
#pragma unroll
  for (int i = 0; i < SM_NE; ++i) x[i] = load_chunk(row, V, i, voff);
  const int t = tid_pinned();
#pragma unroll
  for (int i = 0; i < SM_NE; ++i) x[i] = i * SM_THREADS + t < V ? x[i] : __builtin_nanf("");
}

// The LP prologue, shared by the four LP kernels: the raw row's lse, and its top_n alternatives straight to global memory
// (top_id / top_lp: the row's top_n slots). x is read only; `red` / `par` are sample_row's reduction rows and their
// parity, used by its protocol (one barrier a reduction, the two rows alternately).
//   M    one block max over the per-thread maxima (fmaxf drops the NaN of indices >= V);
//   S    sum of exp(x - M): per thread over its registers in index order, wave_sum, the 16 waves in order (bsum_f's
//        order), each term exp2((x - M) * log2 e): a subtraction that is exact near the maximum, where the terms weigh,
//        one multiplication and one v_exp_f32 (exp2(0) = 1 exactly: the maximum's own term);
//   lse  M + logf(S) (logf(1) = 0 exactly: a row of one entry has logprob 0.0).
// Top-n: top_n rounds of a block arg-max over the 64-bit key (fkey(x) << 32) | (0xFFFFFFFF - index), each strictly below
// the round before: descending values, equal values by ascending index, -inf last; -0 is keyed as the +0 it equals. A
// thread keeps `mine`, its largest key below the last winner, and scans its 50 registers again only after it won (keys
// are distinct, so that is one thread and the other 15 waves skip the scan): a round costs the others a butterfly, a
// barrier and 16 LDS reads. Nothing here outlives the call but lse: the keys are formed where they are compared, the
// rounds are rolled.
__device__ __forceinline__ float logprob_prologue(const float (&x)[SM_NE], int V, uint32_t (&red)[2][SM_WAVES], int& par,
                                                  int top_n, int32_t* __restrict__ top_id,
                                                  float* __restrict__ top_lp) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __shared__ unsigned long long red64[2][SM_WAVES];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < SM_NE; ++i) m = fmaxf(m, x[i]);
  m = wave_max(m);  // (every lane takes part: not under the lane-0 store)
  par ^= 1;
  if (lane == 0) red[par][w] = __float_as_uint(m);
  __syncthreads();
  float M = -INFINITY;
#pragma unroll
  for (int k = 0; k < SM_WAVES; ++k) M = fmaxf(M, __uint_as_float(red[par][k]));
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < SM_NE; ++i) {
    const float e = __builtin_amdgcn_exp2f((x[i] - M) * 1.4426950408889634f);
    a += x[i] <= M ? e : 0.f;  // (false for the NaN of indices >= V)
  }
  a = wave_sum(a);
  par ^= 1;
  if (lane == 0) red[par][w] = __float_as_uint(a);
  __syncthreads();
  float S = 0.f;
#pragma unroll
  for (int k = 0; k < SM_WAVES; ++k) S += __uint_as_float(red[par][k]);
  const float lse = M + logf(S);

  unsigned long long prev = ~0ull, mine = ~0ull;  // (equal: every thread scans in the first round)
#pragma unroll 1
  for (int r = 0; r < top_n; ++r) {
    if (mine == prev) {
      mine = 0;  // below every key of an index < V (fkey(-inf) > 0)
      const uint32_t t = (uint32_t)tid_pinned();
      uint32_t sign = 0x80000000u;  // fkey's constant behind an empty asm, or the 50 keys, which do not depend on the
      asm volatile("" : "+v"(sign));  // round, are hoisted out of the loop: a second and third array beside the row
#pragma unroll
      for (int i = 0; i < SM_NE; ++i) {
        const uint32_t e = (uint32_t)(i * SM_THREADS) + t, ux = __float_as_uint(x[i]), u = ux == sign ? 0u : ux;  // -0
        const unsigned long long k = ((unsigned long long)(u ^ ((uint32_t)((int32_t)u >> 31) | sign)) << 32) |
                                     (0xFFFFFFFFu - e);
        mine = e < (uint32_t)V && k < prev && k > mine ? k : mine;
      }
    }
    unsigned long long v = mine;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long y = __shfl_xor(v, o, 64);
      v = y > v ? y : v;
    }
    const int p64 = r & 1;  // (the row round r writes was last read in round r - 2, a barrier ago)
    if (lane == 0) red64[p64][w] = v;
    __syncthreads();
    unsigned long long best = 0;
#pragma unroll
    for (int k = 0; k < SM_WAVES; ++k) best = red64[p64][k] > best ? red64[p64][k] : best;
    if (threadIdx.x == 0) {  // (top_n <= V: a round always finds a key)
      top_id[r] = (int32_t)(0xFFFFFFFFu - (uint32_t)best);
      top_lp[r] = keyf((uint32_t)(best >> 32)) - lse;
    }
    prev = best;
  }
  return lse;
}

// The constrained form (CON, gpt2mi.h v24.4): a gpt2mi_constraints as the kernels take it, by value. bias_row[b] < 0:
// row b has no bias row. lmp = fp32(log(min_p)), -inf: off. The stop table is read by thread 0 only.
struct ConRows {
  const float* bias;
  int ld_bias;
  float lmp;
  int min_new, n_stop;
  int bias_row[GPT2MI_DECODE_MAX_B];
  int stop_len[GPT2MI_STOP_MAX_SEQS];
  int32_t stop[GPT2MI_STOP_MAX_SEQS][GPT2MI_STOP_MAX_LEN];
};

// GREEDY (temperature == 0) is a kernel of its own: as one branch of the sampling kernel it kept the row live to the
// end of the other branch, beside the exponentials.
// The kernel's body: row b = blockIdx.x of the buffers, drawn with the key (draw_row, pos) and written to column pos of
// seq_out.
// PEN: `hist` is the row's history (positions [0, pos) are read, [gen_start, pos) count as generated), rp / pp / fp the
// repetition, presence and frequency values, logits_out the row-major [B][V] copy of the penalised row (may be NULL).
// LP: lp_out is where the drawn token's log-probability goes, top_id / top_lp the row's top_n slots (logprob_prologue).
// CON: `con` holds the row's constraints (generation.py apply_constraints, stop_match). After the penalties, in this
// order: the row's bias row is added, one coalesced load and one fp32 add per element in groups of ten (no second row
// array); while pos - gen_start < min_new the eos logit becomes -inf; logits_out takes the row as it stands; after the
// top-p search thr = max(thr, max + lmp) (min-p); thread 0 sets done when the drawn token completes a stop sequence
// that lies in [gen_start, pos] (hist is read for that also when PEN is off).
template <bool GREEDY, bool PEN, bool LP, bool CON = false>
__device__ __forceinline__ void sample_row(const float* __restrict__ logits, int ldl, int V, float temperature,
                                           int top_k, float top_p, uint64_t seed, uint32_t draw_row, int pos,
                                           int64_t eos, uint8_t* __restrict__ done, int64_t* __restrict__ tok_out,
                                           int64_t* __restrict__ seq_out, int ld_seq, float* __restrict__ probs_out,
                                           const int64_t* hist = nullptr, int gen_start = 0, float rp = 1.f,
                                           float pp = 0.f, float fp = 0.f, float* __restrict__ logits_out = nullptr,
                                           float* __restrict__ lp_out = nullptr, int top_n = 0,
                                           int32_t* __restrict__ top_id = nullptr,
                                           float* __restrict__ top_lp = nullptr, const ConRows* con = nullptr) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* lp = logits + (size_t)b * ldl;
  __shared__ uint32_t red[2][SM_WAVES];
  __shared__ float csum[SM_WAVES][SM_NE];  // per chunk, the sum of each wave's 64 kept e
  __shared__ float ctot[SM_NE];
  __shared__ int s_tok;
  int par = 0;
  // tid behind an empty asm: each phase forms its 50 element indices where it uses them. Otherwise they are formed
  // once and stay live through the whole kernel, a second array of 50 registers beside the row.
  auto tid_here = [&]() {
    int t = tid;
    asm volatile("" : "+v"(t));
    return t;
  };
  // block reductions of a per-thread (sum: per-wave for the integer count) value; the result is the same in every thread
  auto put = [&](uint32_t v) {
    par ^= 1;
    if (lane == 0) red[par][w] = v;
    __syncthreads();
  };
  auto bsum_f = [&](float v) {
    put(__float_as_uint(wave_sum(v)));
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < SM_WAVES; ++k) t += __uint_as_float(red[par][k]);
    return t;
  };
  auto bsum_wave_i = [&](int wave_value) {
    put((uint32_t)wave_value);
    int t = 0;
#pragma unroll
    for (int k = 0; k < SM_WAVES; ++k) t += (int)red[par][k];
    return t;
  };
  auto bmax_f = [&](float v) {
    put(__float_as_uint(wave_max(v)));
    float t = -INFINITY;
#pragma unroll
    for (int k = 0; k < SM_WAVES; ++k) t = fmaxf(t, __uint_as_float(red[par][k]));
    return t;
  };
  auto bmax_i = [&](int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    put((uint32_t)v);
    int t = INT_MIN;
#pragma unroll
    for (int k = 0; k < SM_WAVES; ++k) t = max(t, (int)red[par][k]);
    return t;
  };

  // the row. Indices >= V hold NaN: no comparison below is true for them, so they are never counted, kept or chosen
  float x[SM_NE];
  load_row(x, lp, V);
  float lse = 0.f;
  if constexpr (LP) lse = logprob_prologue(x, V, red, par, top_n, top_id, top_lp);
  if constexpr (PEN) {
    __shared__ __attribute__((aligned(16))) uint32_t cnt[GPT2MI_SAMPLE_MAX_V / 2];  // two 16-bit entries a word
    for (int i = tid; i < GPT2MI_SAMPLE_MAX_V / 8; i += SM_THREADS) reinterpret_cast<uint4*>(cnt)[i] = uint4{0, 0, 0, 0};
    __syncthreads();
    for (int j = tid; j < pos; j += SM_THREADS) {  // (pos <= ld_hist and <= the cap: the entry's checks)
      const uint64_t t = (uint64_t)hist[j];
      if (t < (uint64_t)V) {  // the one guard of a history value, before it forms any index (negative: huge unsigned)
        const uint32_t sh = ((uint32_t)t & 1u) * 16u;
        if (j >= gen_start)
          atomicAdd(&cnt[(uint32_t)t >> 1], 1u << sh);  // (at most the cap, 8192 < 2^15: no carry into bit 15)
        else
          atomicOr(&cnt[(uint32_t)t >> 1], 0x8000u << sh);
      }
    }
    __syncthreads();
    const uint16_t* c16 = reinterpret_cast<const uint16_t*>(cnt);
#pragma unroll
    for (int i = 0; i < SM_NE; ++i) {
      const uint32_t e = c16[i * SM_THREADS + tid_here()];
      if (__ballot(e != 0)) {  // (wave-uniform) one of this wave's 64 tokens of chunk i is in the window
        const float c = (float)(e & 0x7FFFu);
        float v = x[i];
        if (rp != 1.f && e != 0) v = pinned(v < 0.f ? v * rp : v / rp);
        if (fp != 0.f && c > 0.f) v = pinned(v - pinned(fp * c));
        if (pp != 0.f && c > 0.f) v = pinned(v - pp);
        x[i] = v;
      }
    }
    if constexpr (!CON) {
      if (logits_out) {
#pragma unroll
        for (int i = 0; i < SM_NE; ++i) {
          const int e = i * SM_THREADS + tid_here();
          if (e < V) logits_out[(size_t)b * V + e] = x[i];
        }
      }
    }
  }
  if constexpr (CON) {
    const int br = con->bias_row[b];
    if (br >= 0) {  // (block-uniform) load_row's chunk loads over the bias row: a lane past V adds 0 to its NaN
      const float* brow = con->bias + (size_t)br * con->ld_bias;
      const uint32_t voff = 4u * threadIdx.x;
#pragma unroll
      for (int g = 0; g < SM_NE; g += 10) {
        float bv[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) bv[j] = load_chunk(brow, V, g + j, voff);
#pragma unroll
        for (int j = 0; j < 10; ++j) x[g + j] = pinned(x[g + j] + bv[j]);
      }
    }
    if (con->min_new > 0 && pos - gen_start < con->min_new) {  // (block-uniform; the entry checked eos >= 0)
      const int at = (int)eos - tid_here();
#pragma unroll
      for (int i = 0; i < SM_NE; ++i) x[i] = at == i * SM_THREADS ? -INFINITY : x[i];
    }
    if (logits_out) {
#pragma unroll
      for (int i = 0; i < SM_NE; ++i) {
        const int e = i * SM_THREADS + tid_here();
        if (e < V) logits_out[(size_t)b * V + e] = x[i];
      }
    }
  }
  if constexpr (!GREEDY) {  // IEEE division: the bits of torch's logits / temperature
#pragma unroll
    for (int i = 0; i < SM_NE; ++i) x[i] = x[i] / temperature;
  }
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < SM_NE; ++i) m = fmaxf(m, x[i]);
  const float mx = bmax_f(m);

  int tok;
  if constexpr (GREEDY) {
    int first = INT_MIN;  // -(lowest index at the maximum): chunks in descending order, so the last hit is the lowest
    const int t = tid_here();
#pragma unroll
    for (int i = SM_NE - 1; i >= 0; --i)
      if (x[i] == mx) first = -(i * SM_THREADS + t);
    first = bmax_i(first);
    tok = first == INT_MIN ? 0 : -first;
    if (probs_out)
      for (int e = tid; e < V; e += SM_THREADS) probs_out[(size_t)b * V + e] = e == tok ? 1.f : 0.f;
  } else {
    // top-k: the largest key T with count(x >= T) >= k
    float thr = -INFINITY;
    if (top_k == 1) {
      thr = mx;
    } else if (top_k > 1 && top_k < V) {
      // (the 1024 per-thread maxima are 1024 tokens: for k <= 1024 the k-th largest value is at least their minimum,
      // which starts the search some 8 probes nearer than -inf does)
      uint32_t lo = fkey(top_k <= SM_THREADS ? -bmax_f(-m) : -INFINITY), hi = fkey(mx);
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1) >> 1);
        const float T = keyf(mid);
        int c = 0;
#pragma unroll
        for (int i = 0; i < SM_NE; ++i) c += __popcll(__ballot(x[i] >= T));
        c = bsum_wave_i(c);
        if (c >= top_k) {
          lo = mid;
          if (c == top_k) break;  // no value lies in [T, k-th value): the same set
        } else {
          hi = mid - 1;
        }
      }
      thr = keyf(lo);
    }

    if (top_p < 1.f) {
      // top-p: the smallest key T with mass(x > T) < top_p * Z; then x >= T keeps exactly the tokens whose strictly
      // larger values weigh less than that. T = key(max) has mass 0, so the search ends and the maximum is kept.
      // A second array for the exponentials would not fit (2 x 50 of a thread's 128 registers spill): a probe forms
      // them again, as one fma and one v_exp_f32 each (relative error about 1e-6, on both sides of the
      // comparison).
      const float l2e = 1.4426950408889634f;
      auto mass_above = [&](float T, bool strict) {
        float a = 0.f, off = -mx * l2e;
        asm volatile("" : "+v"(off));  // (or the 50 exponentials are hoisted out of the search loop: that array)
#pragma unroll
        for (int i = 0; i < SM_NE; ++i) {
          const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(x[i], l2e, off));
          a += (strict ? x[i] > T : x[i] >= T) ? e : 0.f;
        }
        return bsum_f(a);
      };
      const float target = top_p * mass_above(thr, false);
      uint32_t lo = fkey(thr), hi = fkey(mx);
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (mass_above(keyf(mid), true) < target)
          hi = mid;
        else
          lo = mid + 1;
      }
      thr = keyf(lo);
    }
    if constexpr (CON) thr = fmaxf(thr, pinned(mx + con->lmp));  // min-p (lmp = -inf: thr as it was)
    // from here the array holds the kept tokens' e = exp(x - max), 0 elsewhere
    float(&ev)[SM_NE] = x;
#pragma unroll
    for (int i = 0; i < SM_NE; ++i) ev[i] = x[i] >= thr ? expf(x[i] - mx) : 0.f;

    // the CDF in vocabulary order: chunk totals (waves in order), chunks in order, then inside one chunk and wave
    // (ten chunks' butterflies side by side, so that a cross-lane step need not wait for the one before it; the sums
    // and their order are those of wave_sum per chunk)
#pragma unroll
    for (int g = 0; g < SM_NE; g += 10) {
      float r[10];
#pragma unroll
      for (int j = 0; j < 10; ++j) r[j] = ev[g + j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int j = 0; j < 10; ++j) r[j] += __shfl_xor(r[j], o, 64);
#pragma unroll
      for (int j = 0; j < 10; ++j)
        if (lane == 0) csum[w][g + j] = r[j];
    }
    if (tid == 0) s_tok = 0;  // (a row without any mass, all NaN: token 0)
    __syncthreads();
    if (tid < SM_NE) {
      float t = 0.f;
#pragma unroll
      for (int k = 0; k < SM_WAVES; ++k) t += csum[k][tid];
      ctot[tid] = t;
    }
    __syncthreads();
    float Z = 0.f;
#pragma unroll 1  // (rolled: unrolled, the 50 running sums of these scans are all live beside the row)
    for (int i = 0; i < SM_NE; ++i) Z += ctot[i];

    uint64_t h = seed + 0x9E3779B97F4A7C15ull * (1ull + (((uint64_t)draw_row << 32) | (uint32_t)pos));
    h ^= h >> 30;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 27;
    h *= 0x94D049BB133111EBull;
    h ^= h >> 31;
    const float u = (float)(uint32_t)(h >> 40) * 0x1p-24f;  // 24 bits: exact
    const float t = u * Z;

    // Each level takes the first member whose running sum exceeds t. The levels add the same terms in different orders
    // (a chunk total is its 16 wave sums from 0, the wave level adds them onto the chunk's base, a wave sum is a
    // butterfly, the lane level a scan), so for t within rounding of a chunk's or wave's upper boundary the level below
    // may find no crossing; u * Z may also round to Z. The level then takes its LAST member with mass: the token stays
    // in the chunk and wave the level above chose, next to the boundary t is within rounding of.
    int c = -1, ws = -1, with_mass = -1;
    bool cross = true;
    float base = 0.f, run = 0.f;
#pragma unroll 1
    for (int i = 0; i < SM_NE; ++i) {
      const float tot = ctot[i], nr = run + tot;
      if (tot > 0.f) with_mass = i;
      if (c < 0 && nr > t) {
        c = i;
        base = run;
      }
      run = nr;
    }
    if (c < 0) {
      c = with_mass;
      cross = false;
    }
    if (c >= 0) {
      run = base;
      with_mass = -1;
#pragma unroll 1
      for (int k = 0; k < SM_WAVES; ++k) {
        const float tot = csum[k][c], nr = run + tot;
        if (tot > 0.f) with_mass = k;
        if (cross && ws < 0 && nr > t) {
          ws = k;
          base = run;
        }
        run = nr;
      }
      if (ws < 0) {
        ws = with_mass;
        cross = false;
      }
    }
    if (ws == w) {  // (wave-uniform) this wave's 64 tokens of chunk c hold the crossing
      float ec = 0.f;
#pragma unroll
      for (int i = 0; i < SM_NE; ++i) ec = i == c ? ev[i] : ec;
      float inc = ec;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
      }
      const unsigned long long mass = __ballot(ec > 0.f), hit = __ballot(cross && ec > 0.f && base + inc > t);
      if (mass && lane == 0) s_tok = c * SM_THREADS + w * 64 + (hit ? __ffsll(hit) - 1 : 63 - __clzll(mass));
    }
    __syncthreads();
    tok = s_tok;
    // (tests only) the kept distribution, from the registers the CDF was built from; the index behind tid_here in every
    // iteration, or the 50 store addresses are formed at once, beside the row
    if (probs_out) {
#pragma unroll
      for (int i = 0; i < SM_NE; ++i) {
        const int e = i * SM_THREADS + tid_here();
        if (e < V) probs_out[(size_t)b * V + e] = ev[i] / Z;
      }
    }
  }

  if (tid == 0) {
    int64_t t64 = tok;
    [[maybe_unused]] bool was_done = false;
    if (done && eos >= 0) {
      if (done[b]) {
        t64 = eos;
        if constexpr (LP) was_done = true;
      } else if (t64 == eos) {
        done[b] = 1;
      } else if constexpr (CON) {
        // stop sequences: the n - 1 history entries before pos and the token in the register against sequence s, when
        // the match lies in [gen_start, pos] and the row then holds min_new generated tokens; every index formed is in
        // [gen_start, pos), inside the window the entry checked
        const int made = pos - gen_start + 1;
        bool hit = false;
        for (int s = 0; s < con->n_stop; ++s) {
          const int n = con->stop_len[s], first = pos - n + 1;
          if (gen_start < 0 || first < gen_start || made < con->min_new || t64 != con->stop[s][n - 1]) continue;
          bool same = true;
          for (int j = 0; j < n - 1; ++j) same = same && hist[first + j] == (int64_t)con->stop[s][j];
          hit = hit || same;
        }
        if (hit) done[b] = 1;
      }
    }
    tok_out[b] = t64;
    if (seq_out) seq_out[(size_t)b * ld_seq + pos] = t64;
    // the raw logit: the logits buffer is never written, the row in registers is long gone
    if constexpr (LP) *lp_out = was_done ? 0.f : lp[tok] - lse;
  }
}

// Per-row position and draw key: the entry's validated host arrays, by value; two scalar loads.
struct RowKeys {
  int pos[GPT2MI_DECODE_MAX_B];
  uint32_t row_id[GPT2MI_DECODE_MAX_B];
};

// The penalised form: per row, the entry's validated host arrays by value again: which row of hist it reads and where
// its generated part starts.
struct PenRows {
  int hist_row[GPT2MI_DECODE_MAX_B];
  int gen_start[GPT2MI_DECODE_MAX_B];
};

// The LP forms. A gpt2mi_logprobs by value, the column of each row from the entry's validated host array.
struct LpRows {
  float* logprob;
  int32_t* top_id;
  float* top_lp;
  int ld, top_n;
  int col[GPT2MI_DECODE_MAX_B];
  // row b's element of the [B][ld] grid
  __device__ size_t at(int b) const { return (size_t)b * ld + col[b]; }
};

// Host: the structs above from a checked call's row tables (common.h SampleCall), and the launch all the kernels share:
// one workgroup per row, the arguments every kernel begins with, then `tail`, what its family takes behind probs_out.
inline RowKeys row_keys(const gpt2mi::SampleCall& c) {
  RowKeys keys;
  memcpy(keys.pos, c.key_pos, sizeof keys.pos);
  memcpy(keys.row_id, c.key_row, sizeof keys.row_id);
  return keys;
}
inline PenRows pen_rows(const gpt2mi::SampleCall& c) {
  PenRows rows;
  memcpy(rows.hist_row, c.hist_row, sizeof rows.hist_row);
  memcpy(rows.gen_start, c.gen_start, sizeof rows.gen_start);
  return rows;
}
inline LpRows lp_rows(const gpt2mi::SampleCall& c) {  // (lp NULL: a form that does not read it)
  LpRows L = {};
  if (c.lp) {
    L = {c.lp->logprob, c.lp->top_id, c.lp->top_logprob, c.lp->ld, c.lp->top_n, {}};
    memcpy(L.col, c.col, sizeof L.col);
  }
  return L;
}
template <class Kernel, class... Tail>
void launch_rows(const gpt2mi::SampleCall& c, Kernel kernel, const Tail&... tail) {
  kernel<<<c.B, SM_THREADS, 0, (hipStream_t)c.stream>>>(c.logits, c.ldl, c.V, c.temperature, c.top_k, c.top_p, c.seed,
                                                        row_keys(c), c.eos, c.done, c.tok_out, c.seq_out, c.ld_seq,
                                                        c.probs_out, tail...);
}

}  // namespace
#endif  // GPT2MI_SAMPLE_ROW_H
