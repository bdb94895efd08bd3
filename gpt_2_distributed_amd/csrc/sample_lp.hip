// The LP instantiations of the sampling kernel (csrc/sample.hip, sample_row.h): the four forms of the draw, each with
// the log-probability of the drawn token and the top_n alternatives (gpt2mi.h v24.1). A unit of its own: sample.hip
// keeps the kernels it had, compiled as before; its sample_rows checks the call (common.h SampleCall), fills the row
// tables and hands the record to the launch below.
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
int launch_sample_lp(const char* what, const SampleCall& c) {
  const bool greedy = c.temperature == 0.f;
  if (c.pen_on)
    launch_rows(c, greedy ? penalized_lp_kernel<true> : penalized_lp_kernel<false>, c.pen->hist, c.pen->ld_hist,
                pen_rows(c), c.pen->repetition, c.pen->presence, c.pen->frequency, c.logits_out, lp_rows(c));
  else
    launch_rows(c, greedy ? sample_lp_kernel<true> : sample_lp_kernel<false>, lp_rows(c));
  return check_launch(what);
}
}  // namespace gpt2mi
