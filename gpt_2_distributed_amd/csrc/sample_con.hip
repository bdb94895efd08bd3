// The constrained instantiations of the sampling kernel (csrc/sample.hip, sample_row.h): logit bias, min-p, a minimum
// number of new tokens and stop sequences in the launch that draws the token (gpt2mi.h v24.4; generation.py
// apply_constraints, sample_reference's min_p and stop_match are the rule). A unit of its own, as sample_lp.hip is: the
// plain, penalised and LP kernels keep their code, and a call whose constraints are all neutral never gets here.
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
int launch_sample_con(const char* what, const float* logits, int ldl, int B, int V, float temperature, int top_k,
                      float top_p, uint64_t seed, const int* pos, const uint32_t* row_id, int64_t eos, uint8_t* done,
                      int64_t* tok_out, int64_t* seq_out, int ld_seq, float* probs_out, const gpt2mi_penalties* pen,
                      bool pen_on, const int* hist_row, const int* gen_start, float* logits_out,
                      const gpt2mi_logprobs* lp, const int* col, const gpt2mi_constraints* con, const int* bias_row,
                      float lmp, void* stream) {
  RowKeys keys = {};
  PenRows rows = {};
  LpRows L = {};
  if (lp) L = {lp->logprob, lp->top_id, lp->top_logprob, lp->ld, lp->top_n, {}};
  ConRows C = {};
  C.bias = con->bias;
  C.ld_bias = con->ld_bias;
  C.lmp = lmp;
  C.min_new = con->min_new;
  C.n_stop = con->n_stop;
  for (int b = 0; b < B; ++b) {
    keys.pos[b] = pos[b];
    keys.row_id[b] = row_id[b];
    rows.hist_row[b] = hist_row[b];
    rows.gen_start[b] = gen_start[b];
    if (lp) L.col[b] = col[b];
    C.bias_row[b] = bias_row[b];
  }
  for (int s = 0; s < con->n_stop; ++s) {
    C.stop_len[s] = con->stop_len[s];
    for (int j = 0; j < con->stop_len[s]; ++j) C.stop[s][j] = con->stop[s * GPT2MI_STOP_MAX_LEN + j];
  }
  const int64_t* hist = pen ? pen->hist : nullptr;
  const int ld_hist = pen ? pen->ld_hist : 0;
  const float rp = pen_on ? pen->repetition : 1.f, pp = pen_on ? pen->presence : 0.f, fp = pen_on ? pen->frequency : 0.f;
  const hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto kernel) {
    kernel<<<B, SM_THREADS, 0, st>>>(logits, ldl, V, temperature, top_k, top_p, seed, keys, eos, done, tok_out, seq_out,
                                     ld_seq, probs_out, hist, ld_hist, rows, rp, pp, fp, logits_out, L, C);
  };
  const bool greedy = temperature == 0.f;
  switch ((greedy ? 4 : 0) | (pen_on ? 2 : 0) | (lp ? 1 : 0)) {
    case 0: launch(constrained_kernel<false, false, false>); break;
    case 1: launch(constrained_kernel<false, false, true>); break;
    case 2: launch(constrained_kernel<false, true, false>); break;
    case 3: launch(constrained_kernel<false, true, true>); break;
    case 4: launch(constrained_kernel<true, false, false>); break;
    case 5: launch(constrained_kernel<true, false, true>); break;
    case 6: launch(constrained_kernel<true, true, false>); break;
    default: launch(constrained_kernel<true, true, true>); break;
  }
  return check_launch(what);
}
}  // namespace gpt2mi
