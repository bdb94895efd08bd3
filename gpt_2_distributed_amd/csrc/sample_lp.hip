// The LP instantiations of the sampling kernel (csrc/sample.hip, sample_row.h): the four forms of the draw, each with
// the log-probability of the drawn token and the top_n alternatives (gpt2mi.h v24.1). A unit of its own: sample.hip
// keeps the kernels it had, compiled as before; its sample_rows checks the arguments and calls the launch below.
#include "sample_row.h"

namespace {

template <bool GREEDY>
__global__ __launch_bounds__(SM_THREADS) void sample_lp_kernel(const float* __restrict__ logits, int ldl, int V,
                                                               float temperature, int top_k, float top_p, uint64_t seed,
                                                               RowKeys keys, int64_t eos, uint8_t* __restrict__ done,
                                                               int64_t* __restrict__ tok_out,
                                                               int64_t* __restrict__ seq_out, int ld_seq,
                                                               float* __restrict__ probs_out, LpRows L) {
  const int b = blockIdx.x;
  const size_t at = L.at(b);
  sample_row<GREEDY, false, true>(logits, ldl, V, temperature, top_k, top_p, seed, keys.row_id[b], keys.pos[b], eos, done,
                                  tok_out, seq_out, ld_seq, probs_out, nullptr, 0, 1.f, 0.f, 0.f, nullptr, L.logprob + at,
                                  L.top_n, L.top_id + at * L.top_n, L.top_lp + at * L.top_n);
}

template <bool GREEDY>
__global__ __launch_bounds__(SM_THREADS) void penalized_lp_kernel(const float* __restrict__ logits, int ldl, int V,
                                                                  float temperature, int top_k, float top_p,
                                                                  uint64_t seed, RowKeys keys, int64_t eos,
                                                                  uint8_t* __restrict__ done,
                                                                  int64_t* __restrict__ tok_out, int64_t* seq_out,
                                                                  int ld_seq, float* __restrict__ probs_out,
                                                                  const int64_t* hist, int ld_hist, PenRows rows,
                                                                  float rp, float pp, float fp,
                                                                  float* __restrict__ logits_out, LpRows L) {
  const int b = blockIdx.x;
  const size_t at = L.at(b);
  sample_row<GREEDY, true, true>(logits, ldl, V, temperature, top_k, top_p, seed, keys.row_id[b], keys.pos[b], eos, done,
                                 tok_out, seq_out, ld_seq, probs_out, hist + (size_t)rows.hist_row[b] * ld_hist,
                                 rows.gen_start[b], rp, pp, fp, logits_out, L.logprob + at, L.top_n,
                                 L.top_id + at * L.top_n, L.top_lp + at * L.top_n);
}

}  // namespace

namespace gpt2mi {
int launch_sample_lp(const char* what, const float* logits, int ldl, int B, int V, float temperature, int top_k,
                     float top_p, uint64_t seed, const int* pos, const uint32_t* row_id, int64_t eos, uint8_t* done,
                     int64_t* tok_out, int64_t* seq_out, int ld_seq, float* probs_out, const gpt2mi_penalties* pen,
                     const int* hist_row, const int* gen_start, float* logits_out, const gpt2mi_logprobs* lp,
                     const int* col, void* stream) {
  RowKeys keys = {};
  PenRows rows = {};
  LpRows L = {lp->logprob, lp->top_id, lp->top_logprob, lp->ld, lp->top_n, {}};
  for (int b = 0; b < B; ++b) {
    keys.pos[b] = pos[b];
    keys.row_id[b] = row_id[b];
    L.col[b] = col[b];
    if (pen) {
      rows.hist_row[b] = hist_row[b];
      rows.gen_start[b] = gen_start[b];
    }
  }
  const hipStream_t st = (hipStream_t)stream;
  if (pen) {
    if (temperature == 0.f)
      penalized_lp_kernel<true><<<B, SM_THREADS, 0, st>>>(
          logits, ldl, V, temperature, top_k, top_p, seed, keys, eos, done, tok_out, seq_out, ld_seq, probs_out,
          pen->hist, pen->ld_hist, rows, pen->repetition, pen->presence, pen->frequency, logits_out, L);
    else
      penalized_lp_kernel<false><<<B, SM_THREADS, 0, st>>>(
          logits, ldl, V, temperature, top_k, top_p, seed, keys, eos, done, tok_out, seq_out, ld_seq, probs_out,
          pen->hist, pen->ld_hist, rows, pen->repetition, pen->presence, pen->frequency, logits_out, L);
  } else if (temperature == 0.f) {
    sample_lp_kernel<true><<<B, SM_THREADS, 0, st>>>(logits, ldl, V, temperature, top_k, top_p, seed, keys, eos, done,
                                                     tok_out, seq_out, ld_seq, probs_out, L);
  } else {
    sample_lp_kernel<false><<<B, SM_THREADS, 0, st>>>(logits, ldl, V, temperature, top_k, top_p, seed, keys, eos, done,
                                                      tok_out, seq_out, ld_seq, probs_out, L);
  }
  return check_launch(what);
}
}  // namespace gpt2mi
