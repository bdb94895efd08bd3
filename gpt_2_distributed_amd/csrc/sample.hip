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
//
// Log-probabilities (LP, v24.1: kernels of their own again, in a unit of their own, sample_lp.hip, over the same
// sample_row of sample_row.h): logprob_prologue, between the load and everything that
// changes the row, forms lse = max + log(sum exp(x - max)) of the raw row and writes the top_n alternatives; at the end
// thread 0 loads the drawn token's raw logit and writes l_tok - lse (gpt2mi.h v24.1, generation.py token_logprobs).
//
// Constraints (CON, v24.4: kernels and a unit of their own once more, sample_con.hip): a bias row added after the
// penalties, the eos held back below a minimum length, min-p as one more bound on thr, and stop sequences matched by
// thread 0 against the history and the token it drew (gpt2mi.h v24.4, generation.py apply_constraints / stop_match).
// sample_rows below checks a gpt2mi_constraints and sends only a non-neutral one there.
//
// The host path: every entry (and the token loop of decode.hip) fills one gpt2mi::SampleCall (common.h); sample_rows
// checks it, fills its row tables and launches a kernel of this unit or hands the record to launch_sample_lp /
// launch_sample_con; each kernel family's argument list is written once, in launch_rows (sample_row.h) and its caller.
#include "sample_row.h"

namespace {

template <bool GREEDY>
__global__ __launch_bounds__(SM_THREADS) void sample_kernel(const float* __restrict__ logits, int ldl, int V,
                                                            float temperature, int top_k, float top_p, uint64_t seed,
                                                            RowKeys keys, int64_t eos, uint8_t* __restrict__ done,
                                                            int64_t* __restrict__ tok_out, int64_t* __restrict__ seq_out,
                                                            int ld_seq, float* __restrict__ probs_out) {
  sample_row<GREEDY, false, false>(logits, ldl, V, temperature, top_k, top_p, seed, keys.row_id[blockIdx.x],
                                   keys.pos[blockIdx.x], eos, done, tok_out, seq_out, ld_seq, probs_out);
}

// The penalised form (PenRows: which row of hist a row reads and where its generated part starts).
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
  sample_row<GREEDY, true, false>(logits, ldl, V, temperature, top_k, top_p, seed, keys.row_id[b], keys.pos[b], eos,
                                  done, tok_out, seq_out, ld_seq, probs_out, hist + (size_t)rows.hist_row[b] * ld_hist,
                                  rows.gen_start[b], rp, pp, fp, logits_out);
}

}  // namespace

namespace gpt2mi {
// A call as its entry filled it (common.h SampleCall): gpt2mi_sample_ragged's arguments, and gpt2mi_sample's with every
// pos[b] equal and no row_id; `what` is the entry's name in messages. pen (may be NULL) and logits_out:
// gpt2mi_sample_penalized's; lp (may be NULL): gpt2mi_sample_logprobs'; con (may be NULL): gpt2mi_sample_constrained's,
// and only a non-neutral one leaves the launches below.
int sample_rows(const char* what, SampleCall& c) {
  const int B = c.B, V = c.V;
  const int* pos = c.pos;
  const gpt2mi_penalties* pen = c.pen;
  GPT2MI_REQUIRE(B >= 1 && B <= GPT2MI_DECODE_MAX_B && V >= 1, "%s: B=%d not in [1, %d] or V=%d not positive", what, B,
                 GPT2MI_DECODE_MAX_B, V);
  GPT2MI_REQUIRE(V <= GPT2MI_SAMPLE_MAX_V, "%s: V=%d above the kernel's row capacity %d", what, V, GPT2MI_SAMPLE_MAX_V);
  GPT2MI_REQUIRE(c.ldl >= V, "%s: ldl=%d < V=%d", what, c.ldl, V);
  GPT2MI_REQUIRE(c.temperature >= 0.f, "%s: temperature=%g must be >= 0", what, (double)c.temperature);  // (NaN fails too)
  GPT2MI_REQUIRE(c.top_p > 0.f, "%s: top_p=%g must be > 0 (>= 1: off)", what, (double)c.top_p);
  GPT2MI_REQUIRE(pos != nullptr, "%s: the position array (host, B ints) is NULL", what);
  GPT2MI_REQUIRE(c.eos >= -1 && c.eos < V, "%s: eos=%lld not in [-1, V=%d)", what, (long long)c.eos, V);
  for (int b = 0; b < B; ++b) {
    GPT2MI_REQUIRE(pos[b] >= 0, "%s: pos[%d]=%d is negative", what, b, pos[b]);
    GPT2MI_REQUIRE(!c.seq_out || c.ld_seq > pos[b], "%s: ld_seq=%d does not reach pos[%d]=%d", what, c.ld_seq, b, pos[b]);
    c.key_pos[b] = pos[b];
    c.key_row[b] = c.row_id ? c.row_id[b] : (uint32_t)b;
  }
  c.pen_on = c.con_on = false;
  if (pen) {
    if (const int rc = check_penalty_values(what, pen->repetition, pen->presence, pen->frequency, &c.pen_on)) return rc;
    GPT2MI_REQUIRE(!c.pen_on || pen->hist != nullptr, "%s: penalties need the history buffer: hist is NULL", what);
  }
  if (c.lp) {
    if (const int rc = check_logprobs(what, c.lp, V)) return rc;
    for (int b = 0; b < B; ++b) {
      const int col = c.lp->col ? c.lp->col[b] : pos[b];
      GPT2MI_REQUIRE(col >= 0 && col < c.lp->ld, "%s: logprobs %s[%d]=%d not in [0, ld=%d)", what,
                     c.lp->col ? "col" : "pos", b, col, c.lp->ld);
      c.col[b] = col;
    }
  }
  bool stops = false;  // stop sequences read the history, whatever the penalty values
  if (c.con) {
    if (const int rc = check_constraints(what, c.con, B, V, c.eos, c.done, c.bias_row, &c.con_on)) return rc;
    stops = c.con->n_stop > 0;
    GPT2MI_REQUIRE(!stops || (pen && pen->hist), "%s: stop sequences need the history buffer: hist is NULL", what);
  }
  // the rows of a call that reads the history or gen_start (min_new counts from it): the cap is the penalties' LDS table's
  for (int b = 0; b < B && (c.pen_on || c.con_on); ++b) {
    const bool reads = c.pen_on || stops;
    const int hr = pen && pen->hist_row ? pen->hist_row[b] : b, gs = pen && pen->gen_start ? pen->gen_start[b] : 0;
    GPT2MI_REQUIRE(!c.pen_on || pos[b] <= GPT2MI_PENALTY_MAX_HISTORY, "%s: pos[%d]=%d above the history cap %d", what, b,
                   pos[b], GPT2MI_PENALTY_MAX_HISTORY);
    GPT2MI_REQUIRE(!reads || pen->ld_hist >= pos[b], "%s: ld_hist=%d < pos[%d]=%d", what, pen->ld_hist, b, pos[b]);
    GPT2MI_REQUIRE(!reads || (hr >= 0 && hr < pen->hist_rows), "%s: hist_row[%d]=%d not in [0, hist_rows=%d)", what, b, hr,
                   pen->hist_rows);
    GPT2MI_REQUIRE(gs >= 0 && gs <= pos[b], "%s: gen_start[%d]=%d not in [0, pos=%d]", what, b, gs, pos[b]);
    c.hist_row[b] = reads ? hr : 0;
    c.gen_start[b] = gs;
  }
  GPT2MI_REQUIRE(c.logits && c.tok_out, "%s: logits and tok_out must not be NULL", what);
  const bool greedy = c.temperature == 0.f;
  if (c.con_on) {
    c.lmp = c.con->min_p > 0.f ? (float)log((double)c.con->min_p) : -INFINITY;
    return launch_sample_con(what, c);
  }
  if (c.pen_on) {
    if (c.lp) return launch_sample_lp(what, c);
    launch_rows(c, greedy ? penalized_kernel<true> : penalized_kernel<false>, pen->hist, pen->ld_hist, pen_rows(c),
                pen->repetition, pen->presence, pen->frequency, c.logits_out);
    return check_launch(what);
  }
  if (c.logits_out) {  // neutral values: the logits themselves
    const hipError_t e = hipMemcpy2DAsync(c.logits_out, sizeof(float) * V, c.logits, sizeof(float) * c.ldl,
                                          sizeof(float) * V, B, hipMemcpyDeviceToDevice, (hipStream_t)c.stream);
    GPT2MI_REQUIRE(e == hipSuccess, "%s: copying the logits to logits_out: %s", what, hipGetErrorString(e));
  }
  if (c.lp) return launch_sample_lp(what, c);
  launch_rows(c, greedy ? sample_kernel<true> : sample_kernel<false>);
  return check_launch(what);
}

int check_penalty_values(const char* what, float repetition, float presence, float frequency, bool* on) {
  GPT2MI_REQUIRE(repetition > 0.f && repetition < INFINITY, "%s: repetition=%g must be finite and > 0 (1: off)", what,
                 (double)repetition);  // (NaN fails too)
  GPT2MI_REQUIRE(fabsf(presence) < INFINITY, "%s: presence=%g must be finite (0: off)", what, (double)presence);
  GPT2MI_REQUIRE(fabsf(frequency) < INFINITY, "%s: frequency=%g must be finite (0: off)", what, (double)frequency);
  *on = repetition != 1.f || presence != 0.f || frequency != 0.f;
  return 0;
}
int check_logprobs(const char* what, const gpt2mi_logprobs* lp, int V) {
  GPT2MI_REQUIRE(lp->top_n >= 0 && lp->top_n <= GPT2MI_LOGPROBS_MAX_TOP && lp->top_n <= V,
                 "%s: logprobs top_n=%d not in [0, %d] or above V=%d", what, lp->top_n, GPT2MI_LOGPROBS_MAX_TOP, V);
  GPT2MI_REQUIRE(lp->logprob != nullptr, "%s: logprobs: logprob is NULL", what);
  GPT2MI_REQUIRE(lp->top_n == 0 || (lp->top_id && lp->top_logprob),
                 "%s: logprobs top_n=%d needs top_id and top_logprob: one is NULL", what, lp->top_n);
  return 0;
}
int check_constraints(const char* what, const gpt2mi_constraints* con, int B, int V, int64_t eos, const uint8_t* done,
                      int* bias_row, bool* on) {
  GPT2MI_REQUIRE(con->min_p >= 0.f && con->min_p <= 1.f, "%s: constraints min_p=%g not in [0, 1] (0: off)", what,
                 (double)con->min_p);  // (NaN fails too)
  GPT2MI_REQUIRE(con->min_new >= 0, "%s: constraints min_new=%d is negative (0: off)", what, con->min_new);
  GPT2MI_REQUIRE(con->min_new == 0 || eos >= 0, "%s: constraints min_new=%d needs an eos to hold back (eos=%lld)", what,
                 con->min_new, (long long)eos);
  GPT2MI_REQUIRE(con->n_stop >= 0 && con->n_stop <= GPT2MI_STOP_MAX_SEQS, "%s: constraints n_stop=%d not in [0, %d]", what,
                 con->n_stop, GPT2MI_STOP_MAX_SEQS);
  if (con->n_stop > 0) {
    GPT2MI_REQUIRE(con->stop && con->stop_len, "%s: constraints n_stop=%d needs stop and stop_len: one is NULL", what,
                   con->n_stop);
    for (int s = 0; s < con->n_stop; ++s) {
      GPT2MI_REQUIRE(con->stop_len[s] >= 1 && con->stop_len[s] <= GPT2MI_STOP_MAX_LEN,
                     "%s: constraints stop_len[%d]=%d not in [1, %d]", what, s, con->stop_len[s], GPT2MI_STOP_MAX_LEN);
      for (int j = 0; j < con->stop_len[s]; ++j) {
        const int32_t t = con->stop[s * GPT2MI_STOP_MAX_LEN + j];
        GPT2MI_REQUIRE(t >= 0 && t < V, "%s: constraints stop[%d][%d]=%d not in [0, V=%d)", what, s, j, t, V);
      }
    }
    GPT2MI_REQUIRE(eos >= 0, "%s: stop sequences end a row as eos does: eos=%lld is not a token", what, (long long)eos);
    GPT2MI_REQUIRE(done != nullptr, "%s: stop sequences need the done flags: done is NULL", what);
  }
  bool any_bias = false;
  for (int b = 0; b < B; ++b) bias_row[b] = -1;
  if (con->bias) {
    GPT2MI_REQUIRE(con->ld_bias >= V && con->bias_rows >= 1, "%s: constraints bias with ld_bias=%d < V=%d or bias_rows=%d < 1",
                   what, con->ld_bias, V, con->bias_rows);
    GPT2MI_REQUIRE(con->bias_row || con->bias_rows >= B, "%s: constraints bias_rows=%d < B=%d without a bias_row", what,
                   con->bias_rows, B);
    for (int b = 0; b < B; ++b) {
      const int r = con->bias_row ? con->bias_row[b] : b;
      GPT2MI_REQUIRE(r >= -1 && r < con->bias_rows, "%s: constraints bias_row[%d]=%d not in [-1, bias_rows=%d)", what, b, r,
                     con->bias_rows);
      bias_row[b] = r;
      any_bias = any_bias || r >= 0;
    }
  }
  *on = any_bias || con->min_p > 0.f || con->min_new > 0 || con->n_stop > 0;
  return 0;
}
}  // namespace gpt2mi

// The entries: each fills the call's record with what it takes (the option blocks it lacks stay NULL).
#define SAMPLE_CALL_ARGS                                                                                               \
  .logits = logits, .ldl = ldl, .B = B, .V = V, .temperature = temperature, .top_k = top_k, .top_p = top_p, .seed = seed, \
  .pos = pos, .row_id = row_id, .eos = eos, .done = done, .tok_out = tok_out, .seq_out = seq_out, .ld_seq = ld_seq,    \
  .probs_out = probs_out, .stream = stream

GPT2MI_EXPORT int gpt2mi_sample_constrained(const float* logits, int ldl, int B, int V, float temperature, int top_k,
                                            float top_p, uint64_t seed, const int* pos, const uint32_t* row_id,
                                            int64_t eos, uint8_t* done, int64_t* tok_out, int64_t* seq_out, int ld_seq,
                                            float* probs_out, const gpt2mi_penalties* pen, float* logits_out,
                                            const gpt2mi_logprobs* lp, const gpt2mi_constraints* con, void* stream) {
  gpt2mi::SampleCall c = {SAMPLE_CALL_ARGS, .pen = pen, .logits_out = logits_out, .lp = lp, .con = con};
  return gpt2mi::sample_rows("sample_constrained", c);
}

GPT2MI_EXPORT int gpt2mi_sample_penalized(const float* logits, int ldl, int B, int V, float temperature, int top_k,
                                          float top_p, uint64_t seed, const int* pos, const uint32_t* row_id,
                                          int64_t eos, uint8_t* done, int64_t* tok_out, int64_t* seq_out, int ld_seq,
                                          float* probs_out, const gpt2mi_penalties* pen, float* logits_out,
                                          void* stream) {
  gpt2mi::SampleCall c = {SAMPLE_CALL_ARGS, .pen = pen, .logits_out = logits_out};
  return gpt2mi::sample_rows("sample_penalized", c);
}

GPT2MI_EXPORT int gpt2mi_sample_logprobs(const float* logits, int ldl, int B, int V, float temperature, int top_k,
                                         float top_p, uint64_t seed, const int* pos, const uint32_t* row_id, int64_t eos,
                                         uint8_t* done, int64_t* tok_out, int64_t* seq_out, int ld_seq,
                                         float* probs_out, const gpt2mi_penalties* pen, float* logits_out,
                                         const gpt2mi_logprobs* lp, void* stream) {
  gpt2mi::SampleCall c = {SAMPLE_CALL_ARGS, .pen = pen, .logits_out = logits_out, .lp = lp};
  return gpt2mi::sample_rows("sample_logprobs", c);
}

GPT2MI_EXPORT int gpt2mi_sample_ragged(const float* logits, int ldl, int B, int V, float temperature, int top_k,
                                       float top_p, uint64_t seed, const int* pos, const uint32_t* row_id, int64_t eos,
                                       uint8_t* done, int64_t* tok_out, int64_t* seq_out, int ld_seq, float* probs_out,
                                       void* stream) {
  gpt2mi::SampleCall c = {SAMPLE_CALL_ARGS};
  return gpt2mi::sample_rows("sample_ragged", c);
}

GPT2MI_EXPORT int gpt2mi_sample(const float* logits, int ldl, int B, int V, float temperature, int top_k, float top_p,
                                uint64_t seed, int pos0, int64_t eos, uint8_t* done, int64_t* tok_out, int64_t* seq_out,
                                int ld_seq, float* probs_out, void* stream) {
  GPT2MI_REQUIRE(pos0 >= 0, "sample: pos=%d is negative", pos0);
  GPT2MI_REQUIRE(!seq_out || ld_seq > pos0, "sample: ld_seq=%d does not reach pos=%d", ld_seq, pos0);
  const gpt2mi::SamePos same(pos0);
  const int* pos = same.v;
  const uint32_t* row_id = nullptr;
  gpt2mi::SampleCall c = {SAMPLE_CALL_ARGS};
  return gpt2mi::sample_rows("sample", c);
}
#undef SAMPLE_CALL_ARGS
