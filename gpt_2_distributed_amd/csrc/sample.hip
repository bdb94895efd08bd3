// Device-side sampling: temperature, top-k, top-p and the draw of one token per row in one launch. gfx950, wave64.
//
// One 1024-thread workgroup per row holds the whole row in registers (the pattern of xent_row_kernel): thread t owns
// the logits of indices c * 1024 + t for the chunks c < SM_NE, so every load of a wave is 256 contiguous bytes and the
// row leaves HBM / L2 once. Everything after the load works on those registers:
//   max                one block reduction;
//   top-k threshold    bisection on the order-preserving 32-bit key of a float; a probe counts x >= T with a ballot
//                      and a scalar popcount per chunk (no cross-lane traffic) and one block reduction of the 16 wave
//                      counts; it ends early once a probe counts exactly k (then {x >= T} is the top-k set);
//   top-p threshold    bisection on the same key space for the smallest T whose mass above T is < top_p * Z: one
//                      ordered block sum per probe, the exponentials formed again in every probe (below);
//   softmax            e = exp(x - max) for what was kept, in place of x;
//   draw               per-chunk wave sums -> chunk totals -> an ordered prefix over the 50 chunks, the 16 waves of the
//                      chunk that holds u * Z, and a 64-lane scan inside that wave: the inclusive CDF in vocabulary
//                      order, two levels above a wave scan. A level that finds no crossing (the levels round
//                      differently) takes its last member with mass: the token stays beside the boundary.
// Every float sum runs in a fixed order (thread-sequential, xor butterfly, waves in order): no atomics, the same bits
// on every run. A block reduction costs one barrier: the 16 wave values go to one of two LDS rows used alternately,
// so the row a reduction writes was last read two barriers ago.
// Registers: a 1024-thread workgroup leaves a thread 128, the row takes 50, and anything that holds a second array of
// 50 beside it spills; the comments at tid_here, mass_above and the rolled scans say where that had to be prevented.
// Bound: not the 200 KB read but the dependent chain after it (up to 32 + 32 probes of a barrier, an LDS round trip and
// 50 compares or exponentials per thread): DESIGN.md "Decode" has the timings.
//
// Penalties (PEN, v22: kernels of their own, the plain ones are compiled as before): between the load and the temperature
// division the row's history window moves the logits of the tokens in it (gpt2mi.h v22, generation.py apply_penalties).
// A per-thread count array beside the row would spill, so the counts live in LDS: 16 bits per vocabulary index (bit 15:
// seen in the prompt part, bits 0..14: occurrences in the generated part), zeroed, filled from the window with integer
// LDS atomics (thread j takes positions j, j + 1024, ...; integer adds commute, so the table does not depend on their
// order) and read back once per register. A (wave, chunk) pair none of whose 64 tokens occurred skips the arithmetic on
// a ballot, so the divisions are paid for the few pairs that hold a token of the window. The cost does not depend on
// how often a token repeats and grows by one atomic per thread for every 1024 positions.
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

// GREEDY (temperature == 0) is a kernel of its own: as one branch of the sampling kernel it kept the row live to the
// end of the other branch, beside the exponentials.
// The kernel's body: row b = blockIdx.x of the buffers, drawn with the key (draw_row, pos) and written to column pos of
// seq_out.
// PEN: `hist` is the row's history (positions [0, pos) are read, [gen_start, pos) count as generated), rp / pp / fp the
// repetition, presence and frequency values, logits_out the row-major [B][V] copy of the penalised row (may be NULL).
template <bool GREEDY, bool PEN>
__device__ __forceinline__ void sample_row(const float* __restrict__ logits, int ldl, int V, float temperature,
                                           int top_k, float top_p, uint64_t seed, uint32_t draw_row, int pos,
                                           int64_t eos, uint8_t* __restrict__ done, int64_t* __restrict__ tok_out,
                                           int64_t* __restrict__ seq_out, int ld_seq, float* __restrict__ probs_out,
                                           const int64_t* hist = nullptr, int gen_start = 0, float rp = 1.f,
                                           float pp = 0.f, float fp = 0.f, float* __restrict__ logits_out = nullptr) {
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
  // (fmaxf drops them); the padding columns of the buffer are not read.
  float x[SM_NE];
  // Chunk i of the row is read through a raw buffer over its own valid part, [i * 1024, min(V, (i + 1) * 1024)): the
  // hardware drops the lanes past it (they get 0; a chunk with nothing valid reads nothing), the descriptor is scalar
  // work and the 50 loads share one offset register, so they are all in flight together (50 clamped 64-bit addresses
  // would take 100 registers).
  const uint32_t voff = 4u * tid;
  auto chunk_rsrc = [&](const float* row, int i) {
    const int n = min(max(V - i * SM_THREADS, 0), SM_THREADS);
    return __builtin_amdgcn_make_buffer_rsrc((void*)(row + min(i * SM_THREADS, V - 1)), 0, 4 * n, 0x00020000);
  };
#pragma unroll
  for (int i = 0; i < SM_NE; ++i)
    x[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(chunk_rsrc(lp, i), voff, 0, 0));
  {
    const int t = tid_here();
#pragma unroll
    for (int i = 0; i < SM_NE; ++i) x[i] = i * SM_THREADS + t < V ? x[i] : __builtin_nanf("");
  }
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
    if (done && eos >= 0) {
      if (done[b])
        t64 = eos;
      else if (t64 == eos)
        done[b] = 1;
    }
    tok_out[b] = t64;
    if (seq_out) seq_out[(size_t)b * ld_seq + pos] = t64;
  }
}

// Per-row position and draw key: the entry's validated host arrays, by value; two scalar loads.
struct RowKeys {
  int pos[GPT2MI_DECODE_MAX_B];
  uint32_t row_id[GPT2MI_DECODE_MAX_B];
};

template <bool GREEDY>
__global__ __launch_bounds__(SM_THREADS) void sample_kernel(const float* __restrict__ logits, int ldl, int V,
                                                            float temperature, int top_k, float top_p, uint64_t seed,
                                                            RowKeys keys, int64_t eos, uint8_t* __restrict__ done,
                                                            int64_t* __restrict__ tok_out, int64_t* __restrict__ seq_out,
                                                            int ld_seq, float* __restrict__ probs_out) {
  sample_row<GREEDY, false>(logits, ldl, V, temperature, top_k, top_p, seed, keys.row_id[blockIdx.x],
                            keys.pos[blockIdx.x], eos, done, tok_out, seq_out, ld_seq, probs_out);
}

// The penalised form. Per row, the entry's validated host arrays by value again: which row of hist it reads and where
// its generated part starts.
struct PenRows {
  int hist_row[GPT2MI_DECODE_MAX_B];
  int gen_start[GPT2MI_DECODE_MAX_B];
};

template <bool GREEDY>
__global__ __launch_bounds__(SM_THREADS) void penalized_kernel(const float* __restrict__ logits, int ldl, int V,
                                                               float temperature, int top_k, float top_p,
                                                               uint64_t seed, RowKeys keys, int64_t eos,
                                                               uint8_t* __restrict__ done,
                                                               int64_t* __restrict__ tok_out, int64_t* seq_out,
                                                               int ld_seq, float* __restrict__ probs_out,
                                                               const int64_t* hist, int ld_hist, PenRows rows, float rp,
                                                               float pp, float fp, float* __restrict__ logits_out) {
  const int b = blockIdx.x;
  sample_row<GREEDY, true>(logits, ldl, V, temperature, top_k, top_p, seed, keys.row_id[b], keys.pos[b], eos, done,
                           tok_out, seq_out, ld_seq, probs_out, hist + (size_t)rows.hist_row[b] * ld_hist,
                           rows.gen_start[b], rp, pp, fp, logits_out);
}

// gpt2mi_sample_ragged, and gpt2mi_sample with every pos[b] equal and no row_id; `what` is the entry's name in messages.
// `pen` (may be NULL) and logits_out: gpt2mi_sample_penalized's.
int sample_rows(const char* what, const float* logits, int ldl, int B, int V, float temperature, int top_k, float top_p,
                uint64_t seed, const int* pos, const uint32_t* row_id, int64_t eos, uint8_t* done, int64_t* tok_out,
                int64_t* seq_out, int ld_seq, float* probs_out, void* stream, const gpt2mi_penalties* pen = nullptr,
                float* logits_out = nullptr) {
  GPT2MI_REQUIRE(B >= 1 && B <= GPT2MI_DECODE_MAX_B && V >= 1, "%s: B=%d not in [1, %d] or V=%d not positive", what, B,
                 GPT2MI_DECODE_MAX_B, V);
  GPT2MI_REQUIRE(V <= GPT2MI_SAMPLE_MAX_V, "%s: V=%d above the kernel's row capacity %d", what, V, GPT2MI_SAMPLE_MAX_V);
  GPT2MI_REQUIRE(ldl >= V, "%s: ldl=%d < V=%d", what, ldl, V);
  GPT2MI_REQUIRE(temperature >= 0.f, "%s: temperature=%g must be >= 0", what, (double)temperature);  // (NaN fails too)
  GPT2MI_REQUIRE(top_p > 0.f, "%s: top_p=%g must be > 0 (>= 1: off)", what, (double)top_p);
  GPT2MI_REQUIRE(pos != nullptr, "%s: the position array (host, B ints) is NULL", what);
  GPT2MI_REQUIRE(eos >= -1 && eos < V, "%s: eos=%lld not in [-1, V=%d)", what, (long long)eos, V);
  RowKeys keys = {};
  for (int b = 0; b < B; ++b) {
    GPT2MI_REQUIRE(pos[b] >= 0, "%s: pos[%d]=%d is negative", what, b, pos[b]);
    GPT2MI_REQUIRE(!seq_out || ld_seq > pos[b], "%s: ld_seq=%d does not reach pos[%d]=%d", what, ld_seq, b, pos[b]);
    keys.pos[b] = pos[b];
    keys.row_id[b] = row_id ? row_id[b] : (uint32_t)b;
  }
  bool on = false;
  PenRows rows = {};
  if (pen) {
    if (const int rc = gpt2mi::check_penalty_values(what, pen->repetition, pen->presence, pen->frequency, &on)) return rc;
    if (on) {
      GPT2MI_REQUIRE(pen->hist != nullptr, "%s: penalties need the history buffer: hist is NULL", what);
      for (int b = 0; b < B; ++b) {
        const int hr = pen->hist_row ? pen->hist_row[b] : b, gs = pen->gen_start ? pen->gen_start[b] : 0;
        GPT2MI_REQUIRE(pos[b] <= GPT2MI_PENALTY_MAX_HISTORY, "%s: pos[%d]=%d above the history cap %d", what, b, pos[b],
                       GPT2MI_PENALTY_MAX_HISTORY);
        GPT2MI_REQUIRE(pen->ld_hist >= pos[b], "%s: ld_hist=%d < pos[%d]=%d", what, pen->ld_hist, b, pos[b]);
        GPT2MI_REQUIRE(hr >= 0 && hr < pen->hist_rows, "%s: hist_row[%d]=%d not in [0, hist_rows=%d)", what, b, hr,
                       pen->hist_rows);
        GPT2MI_REQUIRE(gs >= 0 && gs <= pos[b], "%s: gen_start[%d]=%d not in [0, pos=%d]", what, b, gs, pos[b]);
        rows.hist_row[b] = hr;
        rows.gen_start[b] = gs;
      }
    }
  }
  GPT2MI_REQUIRE(logits && tok_out, "%s: logits and tok_out must not be NULL", what);
  if (on) {
    if (temperature == 0.f)
      penalized_kernel<true><<<B, SM_THREADS, 0, (hipStream_t)stream>>>(
          logits, ldl, V, temperature, top_k, top_p, seed, keys, eos, done, tok_out, seq_out, ld_seq, probs_out,
          pen->hist, pen->ld_hist, rows, pen->repetition, pen->presence, pen->frequency, logits_out);
    else
      penalized_kernel<false><<<B, SM_THREADS, 0, (hipStream_t)stream>>>(
          logits, ldl, V, temperature, top_k, top_p, seed, keys, eos, done, tok_out, seq_out, ld_seq, probs_out,
          pen->hist, pen->ld_hist, rows, pen->repetition, pen->presence, pen->frequency, logits_out);
    return gpt2mi::check_launch(what);
  }
  if (logits_out) {  // neutral values: the logits themselves
    const hipError_t e = hipMemcpy2DAsync(logits_out, sizeof(float) * V, logits, sizeof(float) * ldl, sizeof(float) * V,
                                          B, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    GPT2MI_REQUIRE(e == hipSuccess, "%s: copying the logits to logits_out: %s", what, hipGetErrorString(e));
  }
  if (temperature == 0.f)
    sample_kernel<true><<<B, SM_THREADS, 0, (hipStream_t)stream>>>(logits, ldl, V, temperature, top_k, top_p, seed, keys,
                                                                   eos, done, tok_out, seq_out, ld_seq, probs_out);
  else
    sample_kernel<false><<<B, SM_THREADS, 0, (hipStream_t)stream>>>(logits, ldl, V, temperature, top_k, top_p, seed,
                                                                    keys, eos, done, tok_out, seq_out, ld_seq, probs_out);
  return gpt2mi::check_launch(what);
}

}  // namespace

namespace gpt2mi {
int check_penalty_values(const char* what, float repetition, float presence, float frequency, bool* on) {
  GPT2MI_REQUIRE(repetition > 0.f && repetition < INFINITY, "%s: repetition=%g must be finite and > 0 (1: off)", what,
                 (double)repetition);  // (NaN fails too)
  GPT2MI_REQUIRE(fabsf(presence) < INFINITY, "%s: presence=%g must be finite (0: off)", what, (double)presence);
  GPT2MI_REQUIRE(fabsf(frequency) < INFINITY, "%s: frequency=%g must be finite (0: off)", what, (double)frequency);
  *on = repetition != 1.f || presence != 0.f || frequency != 0.f;
  return 0;
}
}  // namespace gpt2mi

GPT2MI_EXPORT int gpt2mi_sample_penalized(const float* logits, int ldl, int B, int V, float temperature, int top_k,
                                          float top_p, uint64_t seed, const int* pos, const uint32_t* row_id,
                                          int64_t eos, uint8_t* done, int64_t* tok_out, int64_t* seq_out, int ld_seq,
                                          float* probs_out, const gpt2mi_penalties* pen, float* logits_out,
                                          void* stream) {
  return sample_rows("sample_penalized", logits, ldl, B, V, temperature, top_k, top_p, seed, pos, row_id, eos, done,
                     tok_out, seq_out, ld_seq, probs_out, stream, pen, logits_out);
}

GPT2MI_EXPORT int gpt2mi_sample_ragged(const float* logits, int ldl, int B, int V, float temperature, int top_k,
                                       float top_p, uint64_t seed, const int* pos, const uint32_t* row_id, int64_t eos,
                                       uint8_t* done, int64_t* tok_out, int64_t* seq_out, int ld_seq, float* probs_out,
                                       void* stream) {
  return sample_rows("sample_ragged", logits, ldl, B, V, temperature, top_k, top_p, seed, pos, row_id, eos, done,
                     tok_out, seq_out, ld_seq, probs_out, stream);
}

GPT2MI_EXPORT int gpt2mi_sample(const float* logits, int ldl, int B, int V, float temperature, int top_k, float top_p,
                                uint64_t seed, int pos, int64_t eos, uint8_t* done, int64_t* tok_out, int64_t* seq_out,
                                int ld_seq, float* probs_out, void* stream) {
  GPT2MI_REQUIRE(pos >= 0, "sample: pos=%d is negative", pos);
  GPT2MI_REQUIRE(!seq_out || ld_seq > pos, "sample: ld_seq=%d does not reach pos=%d", ld_seq, pos);
  return sample_rows("sample", logits, ldl, B, V, temperature, top_k, top_p, seed, gpt2mi::SamePos(pos).v, nullptr, eos,
                     done, tok_out, seq_out, ld_seq, probs_out, stream);
}
