// The constrained instantiations of the sampling kernel (csrc/sample.hip, sample_row.h): logit bias, min-p, a minimum
// number of new tokens and stop sequences in the launch that draws the token (gpt2mi.h v24.4; generation.py
// apply_constraints, sample_reference's min_p and stop_match are the rule). A unit of its own, as sample_lp.hip is: the
// plain, penalised and LP kernels keep their code, and a call whose constraints are all neutral never gets here:
// sample_rows of sample.hip hands the checked record (common.h SampleCall) to the launch below.
// One kernel per (greedy, penalised, LP) form; all take the same arguments, a form reads what it uses.
#include "sample_row.h"

namespace {

template <bool GREEDY, bool PEN, bool LP>
__global__ __launch_bounds__(SM_THREADS) void constrained_kernel(const float* __restrict__ logits, int ldl, int V,
                                                                 float temperature, int top_k, float top_p,
                                                                 uint64_t seed, RowKeys keys, int64_t eos,
                                                                 uint8_t* __restrict__ done,
                                                                 int64_t* __restrict__ tok_out, int64_t* seq_out,
                                                                 int ld_seq, float* __restrict__ probs_out,
                                                                 const int64_t* hist, int ld_hist, PenRows rows, float rp,
                                                                 float pp, float fp, float* __restrict__ logits_out,
                                                                 LpRows L, ConRows con) {
  const int b = blockIdx.x;
  const size_t at = LP ? L.at(b) : 0;
  // (hist NULL: no penalties and no stop sequences, nothing reads it)
  sample_row<GREEDY, PEN, LP, true>(logits, ldl, V, temperature, top_k, top_p, seed, keys.row_id[b], keys.pos[b], eos,
                                    done, tok_out, seq_out, ld_seq, probs_out,
                                    hist ? hist + (size_t)rows.hist_row[b] * ld_hist : nullptr, rows.gen_start[b], rp, pp,
                                    fp, logits_out, LP ? L.logprob + at : nullptr, L.top_n,
                                    LP ? L.top_id + at * L.top_n : nullptr, LP ? L.top_lp + at * L.top_n : nullptr, &con);
}

}  // namespace

namespace gpt2mi {
int launch_sample_con(const char* what, const SampleCall& c) {
  const gpt2mi_penalties* pen = c.pen;
  const gpt2mi_constraints* con = c.con;
  ConRows C = {};
  C.bias = con->bias;
  C.ld_bias = con->ld_bias;
  C.lmp = c.lmp;
  C.min_new = con->min_new;
  C.n_stop = con->n_stop;
  memcpy(C.bias_row, c.bias_row, sizeof C.bias_row);
  for (int s = 0; s < con->n_stop; ++s) {
    C.stop_len[s] = con->stop_len[s];
    for (int j = 0; j < con->stop_len[s]; ++j) C.stop[s][j] = con->stop[s * GPT2MI_STOP_MAX_LEN + j];
  }
  // the kernel of (greedy, penalised, LP) at index 4 greedy + 2 pen_on + lp
  static constexpr decltype(&constrained_kernel<false, false, false>) forms[8] = {
      constrained_kernel<false, false, false>, constrained_kernel<false, false, true>,
      constrained_kernel<false, true, false>,  constrained_kernel<false, true, true>,
      constrained_kernel<true, false, false>,  constrained_kernel<true, false, true>,
      constrained_kernel<true, true, false>,   constrained_kernel<true, true, true>};
  launch_rows(c, forms[(c.temperature == 0.f ? 4 : 0) | (c.pen_on ? 2 : 0) | (c.lp ? 1 : 0)], pen ? pen->hist : nullptr,
              pen ? pen->ld_hist : 0, pen_rows(c), c.pen_on ? pen->repetition : 1.f, c.pen_on ? pen->presence : 0.f,
              c.pen_on ? pen->frequency : 0.f, c.logits_out, lp_rows(c), C);
  return check_launch(what);
}
}  // namespace gpt2mi
