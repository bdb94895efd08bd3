// Beam search on the device (gpt2mi.h v24.2; generation.py beam_select is the rule, executable). gfx950, wave64.
//
// The W beams of a prompt sit in W adjacent rows of a decode session, forks of one prefill: their caches hold identical
// bits over the prompt. A token of the loop is four launches in front of the step:
//   top-W     per row, the W most likely tokens and their log-probabilities: logprob_prologue of sample_row.h on the row
//             in registers, the function the LP sampling kernels call, so the values are gpt2mi_sample_logprobs' bits;
//   select    one workgroup per prompt: the at most W * W candidates are ranked by counting, for each, the candidates
//             strictly ahead of it in a total order; the candidate with count c < W becomes beam c;
//   reorder   the rows take the generated suffix of their parents' caches and token rows, in two launches through a
//             staging buffer (a permutation has cycles: no launch reads what another workgroup of it writes). The
//             prompt part never moves, so the share map of the attention stays valid.
// No float atomics and no order that depends on scheduling: two calls give the same bits.
#include <algorithm>

#include "kv_format.h"
#include "sample_row.h"

namespace {

constexpr int BM_MAX_W = GPT2MI_LOGPROBS_MAX_TOP, BM_THREADS = 256;

// sample_row's row load (load_row) and its LP prologue, nothing else: x is the raw row, indices >= V hold NaN.
__global__ __launch_bounds__(SM_THREADS) void beam_topw_kernel(const float* __restrict__ logits, int ldl, int V, int W,
                                                               int32_t* __restrict__ top_id,
                                                               float* __restrict__ top_lp) {
  const int b = blockIdx.x;
  __shared__ uint32_t red[2][SM_WAVES];
  int par = 0;
  float x[SM_NE];
  load_row(x, logits + (size_t)b * ldl, V);
  logprob_prologue(x, V, red, par, W, top_id + (size_t)b * W, top_lp + (size_t)b * W);
}

// Where the loop puts a step's tokens beside tok_out: column col[r] of row r of seq (NULL: nowhere). The columns are the
// entry's checked host values, by value.
struct SeqCol {
  int64_t* seq;
  int ld;
  int col[GPT2MI_DECODE_MAX_B];
};

// One workgroup per prompt group g, rows g W .. g W + W - 1. Candidate c = j W + r is rank r of beam j: a live beam has W
// of them, score cum[j] + top_lp[j][r] (one fp32 add), a finished beam has rank 0 alone, token eos at score cum[j].
// Order: score descending, then c ascending, which is (beam, rank) ascending; float comparisons, so -0 == +0 and equal
// -inf tie like any other value. Each candidate counts the candidates ahead of it; the order is total over the valid
// candidates, so the counts below W are 0 .. W - 1 once each (every beam offers at least one candidate) and each output
// slot has one writer. The group's cum and done are in LDS before the first barrier and nothing is written before the
// second, so cum_out / done_out may be cum / done themselves or other buffers.
__global__ __launch_bounds__(BM_THREADS) void beam_select_kernel(const int32_t* __restrict__ top_id,
                                                                 const float* __restrict__ top_lp, const float* cum,
                                                                 const uint8_t* done, int W, int64_t eos,
                                                                 int64_t* __restrict__ tok_out,
                                                                 int32_t* __restrict__ parent_out, float* cum_out,
                                                                 uint8_t* done_out, SeqCol sc) {
  __shared__ float s_score[BM_MAX_W * BM_MAX_W];
  __shared__ uint8_t s_ok[BM_MAX_W * BM_MAX_W];
  __shared__ float s_cum[BM_MAX_W];
  __shared__ uint8_t s_fin[BM_MAX_W];
  const int tid = threadIdx.x, row0 = blockIdx.x * W, n = W * W;
  if (tid < W) {
    s_cum[tid] = cum[row0 + tid];
    s_fin[tid] = eos >= 0 && done[row0 + tid] != 0;  // (no eos: nothing is ever finished)
  }
  __syncthreads();
  for (int c = tid; c < n; c += BM_THREADS) {
    const int j = c / W, r = c - j * W;
    const bool fin = s_fin[j];
    s_ok[c] = !fin || r == 0;
    s_score[c] = fin ? s_cum[j] : s_cum[j] + top_lp[(size_t)(row0 + j) * W + r];
  }
  __syncthreads();
  for (int c = tid; c < n; c += BM_THREADS) {
    if (!s_ok[c]) continue;
    const float s = s_score[c];
    int ahead = 0;
    for (int o = 0; o < n; ++o) {
      const float t = s_score[o];
      ahead += (s_ok[o] && (t > s || (t == s && o < c))) ? 1 : 0;
    }
    if (ahead >= W) continue;
    const int j = c / W, r = c - j * W, out = row0 + ahead;
    const bool fin = s_fin[j];
    const int64_t tok = fin ? eos : (int64_t)top_id[(size_t)(row0 + j) * W + r];
    tok_out[out] = tok;
    parent_out[out] = row0 + j;
    cum_out[out] = s;
    done_out[out] = (fin || (eos >= 0 && tok == eos)) ? 1 : 0;
    if (sc.seq) sc.seq[(size_t)out * sc.ld + sc.col[out]] = tok;
  }
}

// The window [lo, hi) of each row: the entry's checked host arrays, by value.
struct BeamWin {
  int lo[GPT2MI_DECODE_MAX_B], hi[GPT2MI_DECODE_MAX_B];
};

constexpr int BR_POS = 32;  // positions of a block: 8 lanes each, a lane moves what KV::load gives it of a 64-wide row

// One half of the reorder. Grid (blocks of 32 window positions, 2 L H + 1, R): block (x, y, r) takes positions
// lo[r] + 32 x .. + 31 of row r, y = (layer, K or V, head), or y = 2 L H for the token row. TO_STAGE: what row
// parent[r] holds there goes to row r's slot of the staging tensors; else the slot goes to row r. The first launch reads
// the caches and writes only the staging buffer, the second reads the staging buffer and writes only the caches, and a
// slot has one writer and one reader, row r's: no workgroup reads what another of the same launch writes, whatever
// the permutation. A row with parent == self is skipped in both, and so is a row whose parent lies outside its group
// [g W, g W + W): parent is the one device-side row index of the decode path, and this is its one guard, in front of every
// address formed from it (the doctrine of sample_row's history guard). Nothing outside [lo, hi) of a moved row is
// written. The staging tensors are caches of `win` positions and R streams per layer, so the cache types move the rows:
// 16 bytes per lane with bf16, 8 bytes of codes and the row's scale with fp8.
template <bool TO_STAGE, class KV>
__global__ __launch_bounds__(BR_POS * 8) void beam_reorder_kernel(KV kc, KV vc, KV sk, KV sv, size_t layer_rows, int L,
                                                                  int H, int Tcap, int win, int64_t* seq, int ld_seq,
                                                                  int64_t* stage_seq,
                                                                  const int32_t* __restrict__ parent, int W, int R,
                                                                  BeamWin wn) {
  const int r = blockIdx.z, p = parent[r], g0 = (r / W) * W;
  if (p == r || p < g0 || p >= g0 + W) return;
  const int lo = wn.lo[r], t = lo + blockIdx.x * BR_POS + (threadIdx.x >> 3), dg = threadIdx.x & 7;
  if (t >= wn.hi[r]) return;
  const int y = blockIdx.y;
  if (y == 2 * L * H) {
    if (seq && dg == 0) {
      int64_t* slot = stage_seq + (size_t)r * win + (t - lo);
      if (TO_STAGE)
        *slot = seq[(size_t)p * ld_seq + t];
      else
        seq[(size_t)r * ld_seq + t] = *slot;
    }
    return;
  }
  const int h = y % H, which = (y / H) & 1, l = y / (2 * H);
  const KV cache = (which ? vc : kc).shifted((size_t)l * layer_rows);
  const KV stage = (which ? sv : sk).shifted((size_t)l * R * H * win);
  const KvLane wc((size_t)(TO_STAGE ? p : r) * H + h, Tcap, dg), ws((size_t)r * H + h, win, dg);
  if (TO_STAGE) {
    const typename KV::Row row = cache.load(wc, t);
    stage.store(ws, t - lo, row);
    if (dg == 0) stage.store_once(ws, t - lo, row);
  } else {
    const typename KV::Row row = stage.load(ws, t - lo);
    cache.store(wc, t, row);
    if (dg == 0) cache.store_once(wc, t, row);
  }
}

size_t kv_row_bytes(int kv_format) { return kv_format == GPT2MI_KV_FP8 ? 64 : 128; }

// The staging buffer of R rows of `win` positions: K rows, V rows, with fp8 the K and the V scales, then the tokens.
size_t reorder_bytes(int kv_format, int L, int H, int R, int win) {
  const size_t rows = (size_t)L * R * H * win;
  return 2 * rows * (kv_row_bytes(kv_format) + (kv_format == GPT2MI_KV_FP8 ? sizeof(float) : 0)) +
         (size_t)R * win * sizeof(int64_t);
}

int check_group_shape(const char* what, int G, int W) {
  GPT2MI_REQUIRE(W >= 1 && W <= GPT2MI_LOGPROBS_MAX_TOP, "%s: W=%d not in [1, %d] (GPT2MI_LOGPROBS_MAX_TOP)", what, W,
                 GPT2MI_LOGPROBS_MAX_TOP);
  GPT2MI_REQUIRE(G >= 1 && (long long)G * W <= GPT2MI_DECODE_MAX_B, "%s: G=%d x W=%d rows not in [1, %d]", what, G, W,
                 GPT2MI_DECODE_MAX_B);
  return 0;
}

// gpt2mi_beam_select after its checks; sc: the loop's column of seq.
int select_launch(const char* what, const int32_t* top_id, const float* top_logprob, const float* cum,
                  const uint8_t* done, int G, int W, int64_t eos, int64_t* tok_out, int32_t* parent_out, float* cum_out,
                  uint8_t* done_out, const SeqCol& sc, void* stream) {
  if (const int rc = check_group_shape(what, G, W)) return rc;
  GPT2MI_REQUIRE(eos >= -1, "%s: eos=%lld below -1 (-1: none)", what, (long long)eos);
  GPT2MI_REQUIRE(top_id && top_logprob && cum && done && tok_out && parent_out && cum_out && done_out,
                 "%s: top_id, top_logprob, cum, done, tok_out, parent_out, cum_out and done_out must not be NULL", what);
  beam_select_kernel<<<G, BM_THREADS, 0, (hipStream_t)stream>>>(top_id, top_logprob, cum, done, W, eos, tok_out,
                                                                parent_out, cum_out, done_out, sc);
  return gpt2mi::check_launch(what);
}

struct ReorderArgs {
  void *k, *v;
  float *ks, *vs;
  int kv_format, L;
  size_t layer_rows;
  int B, H, Tcap;
  int64_t* seq;
  int ld_seq;
};

int reorder_launch(const char* what, const ReorderArgs& a, const int32_t* parent, int G, int W, const int* lo,
                   const int* hi, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int rc = check_group_shape(what, G, W)) return rc;
  const int R = G * W;
  GPT2MI_REQUIRE(a.kv_format == GPT2MI_KV_BF16 || a.kv_format == GPT2MI_KV_FP8,
                 "%s: kv_format=%d is neither 0 (bf16) nor 1 (fp8 e4m3)", what, a.kv_format);
  GPT2MI_REQUIRE(a.L >= 1 && a.H >= 1 && a.Tcap >= 1 && a.B >= R, "%s: L=%d, H=%d, Tcap=%d must be positive and B=%d >= G W=%d",
                 what, a.L, a.H, a.Tcap, a.B, R);
  GPT2MI_REQUIRE(2ll * a.L * a.H + 1 <= 65535, "%s: 2 L H + 1 = %lld exceeds a grid dimension (65535)", what,
                 2ll * a.L * a.H + 1);
  GPT2MI_REQUIRE(a.L == 1 || a.layer_rows >= (size_t)a.B * a.H * a.Tcap,
                 "%s: layer_rows=%zu below the B H Tcap = %zu rows of a layer", what, a.layer_rows,
                 (size_t)a.B * a.H * a.Tcap);
  GPT2MI_REQUIRE(lo != nullptr && hi != nullptr, "%s: the window arrays lo and hi (host, G W ints) must not be NULL", what);
  BeamWin wn = {};
  int win = 0;
  for (int r = 0; r < R; ++r) {
    GPT2MI_REQUIRE(lo[r] >= 0 && lo[r] <= hi[r] && hi[r] <= a.Tcap, "%s: window [lo[%d]=%d, hi[%d]=%d) not inside [0, Tcap=%d]",
                   what, r, lo[r], r, hi[r], a.Tcap);
    GPT2MI_REQUIRE(!a.seq || hi[r] <= a.ld_seq, "%s: hi[%d]=%d exceeds ld_seq=%d", what, r, hi[r], a.ld_seq);
    const int g0 = (r / W) * W;
    GPT2MI_REQUIRE(lo[r] == lo[g0] && hi[r] == hi[g0],
                   "%s: window [%d, %d) of row %d differs from its group's [%d, %d) (row %d): a row takes its parent's", what,
                   lo[r], hi[r], r, lo[g0], hi[g0], g0);
    wn.lo[r] = lo[r], wn.hi[r] = hi[r];
    win = std::max(win, hi[r] - lo[r]);
  }
  const size_t need = reorder_bytes(a.kv_format, a.L, a.H, R, win);
  GPT2MI_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu bytes given, %zu needed: gpt2mi_beam_reorder_workspace)",
                 what, workspace_bytes, need);
  GPT2MI_REQUIRE(a.kv_format != GPT2MI_KV_FP8 || (a.ks && a.vs), "%s: kscale and vscale of the fp8 cache must not be NULL",
                 what);
  GPT2MI_REQUIRE(a.k && a.v && parent, "%s: the caches and parent must not be NULL", what);
  if (win == 0) return 0;  // every window is empty: nothing moves
  GPT2MI_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "%s: workspace is NULL or not 16-byte aligned", what);
  const size_t rows = (size_t)a.L * R * a.H * win, rb = kv_row_bytes(a.kv_format);
  char* ws = (char*)workspace;
  char *sk = ws, *sv = ws + rows * rb;
  float* sks = (float*)(ws + 2 * rows * rb);
  float* svs = sks + rows;
  int64_t* sseq = (int64_t*)(ws + 2 * rows * (rb + (a.kv_format == GPT2MI_KV_FP8 ? sizeof(float) : 0)));
  const dim3 grid((win + BR_POS - 1) / BR_POS, 2 * a.L * a.H + 1, R);
  const hipStream_t st = (hipStream_t)stream;
  auto both = [&](auto kc, auto vc, auto stk, auto stv) {
    beam_reorder_kernel<true><<<grid, BR_POS * 8, 0, st>>>(kc, vc, stk, stv, a.layer_rows, a.L, a.H, a.Tcap, win, a.seq,
                                                           a.ld_seq, sseq, parent, W, R, wn);
    if (const int rc = gpt2mi::check_launch(what)) return rc;
    beam_reorder_kernel<false><<<grid, BR_POS * 8, 0, st>>>(kc, vc, stk, stv, a.layer_rows, a.L, a.H, a.Tcap, win, a.seq,
                                                            a.ld_seq, sseq, parent, W, R, wn);
    return gpt2mi::check_launch(what);
  };
  if (a.kv_format == GPT2MI_KV_FP8)
    return both(KvFp8{(uint8_t*)a.k, a.ks}, KvFp8{(uint8_t*)a.v, a.vs}, KvFp8{(uint8_t*)sk, sks}, KvFp8{(uint8_t*)sv, svs});
  return both(KvBf16{(bf16*)a.k}, KvBf16{(bf16*)a.v}, KvBf16{(bf16*)sk}, KvBf16{(bf16*)sv});
}

}  // namespace

GPT2MI_EXPORT int gpt2mi_beam_select(const int32_t* top_id, const float* top_logprob, const float* cum,
                                     const uint8_t* done, int G, int W, int64_t eos, int64_t* tok_out,
                                     int32_t* parent_out, float* cum_out, uint8_t* done_out, void* stream) {
  return select_launch("beam_select", top_id, top_logprob, cum, done, G, W, eos, tok_out, parent_out, cum_out, done_out,
                       SeqCol{}, stream);
}

GPT2MI_EXPORT size_t gpt2mi_beam_reorder_workspace(int kv_format, int L, int H, int R, int window) {
  if ((kv_format != GPT2MI_KV_BF16 && kv_format != GPT2MI_KV_FP8) || L < 1 || H < 1 || R < 1 || window < 0) return 0;
  return reorder_bytes(kv_format, L, H, R, window);
}

GPT2MI_EXPORT int gpt2mi_beam_reorder(void* kcache, void* vcache, float* kscale, float* vscale, int kv_format, int L,
                                      size_t layer_rows, int B, int H, int Tcap, int64_t* seq, int ld_seq,
                                      const int32_t* parent, int G, int W, const int* lo, const int* hi, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  return reorder_launch("beam_reorder", ReorderArgs{kcache, vcache, kscale, vscale, kv_format, L, layer_rows, B, H, Tcap,
                                                    seq, ld_seq},
                        parent, G, W, lo, hi, workspace, workspace_bytes, stream);
}

GPT2MI_EXPORT int gpt2mi_decode_beam_search(const gpt2mi_decode_plan* P, int V, int W, int64_t eos, const int* pos0,
                                            const int* lo, int n, int64_t* tok, int64_t* seq, int ld_seq, float* cum,
                                            uint8_t* done, int32_t* parents, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  const char* what = "decode_beam_search";
  GPT2MI_REQUIRE(P != nullptr, "%s: plan is NULL", what);
  GPT2MI_REQUIRE(P->B >= 1 && P->B <= GPT2MI_DECODE_MAX_B, "%s: B=%d not in [1, %d]", what, P->B, GPT2MI_DECODE_MAX_B);
  GPT2MI_REQUIRE(W >= 1 && P->B % W == 0, "%s: the plan's B=%d rows are not groups of W=%d", what, P->B, W);
  const int R = P->B, G = R / W;
  if (const int rc = check_group_shape(what, G, W)) return rc;
  GPT2MI_REQUIRE(V >= 1 && V <= P->Vp && V <= GPT2MI_SAMPLE_MAX_V, "%s: V=%d not in [1, Vp=%d] or above the row capacity %d",
                 what, V, P->Vp, GPT2MI_SAMPLE_MAX_V);
  GPT2MI_REQUIRE(W <= V, "%s: W=%d above V=%d", what, W, V);
  GPT2MI_REQUIRE(eos >= -1 && eos < V, "%s: eos=%lld not in [-1, V=%d)", what, (long long)eos, V);
  GPT2MI_REQUIRE(n >= 0, "%s: n=%d must be >= 0", what, n);
  GPT2MI_REQUIRE(pos0 != nullptr && lo != nullptr, "%s: pos0 and lo (host, B ints) must not be NULL", what);
  int max_pos = 0, win = 0;
  for (int b = 0; b < R; ++b) {
    const int g0 = (b / W) * W;
    GPT2MI_REQUIRE(pos0[b] >= 1 && pos0[b] < P->Tcap, "%s: pos0[%d]=%d not in [1, Tcap=%d)", what, b, pos0[b], P->Tcap);
    GPT2MI_REQUIRE(lo[b] >= 1 && lo[b] <= pos0[b], "%s: lo[%d]=%d not in [1, pos0=%d]", what, b, lo[b], pos0[b]);
    GPT2MI_REQUIRE(pos0[b] == pos0[g0] && lo[b] == lo[g0],
                   "%s: row %d at (pos0=%d, lo=%d) differs from its group's row %d at (%d, %d): beams have one length", what,
                   b, pos0[b], lo[b], g0, pos0[g0], lo[g0]);
    max_pos = std::max(max_pos, pos0[b]);
    win = std::max(win, pos0[b] + std::max(n, 1) - 1 - lo[b]);
  }
  GPT2MI_REQUIRE((long long)max_pos + n <= P->Tcap, "%s: max pos0=%d + n=%d exceeds the cache length Tcap=%d", what, max_pos,
                 n, P->Tcap);
  GPT2MI_REQUIRE((long long)max_pos + n <= ld_seq, "%s: max pos0=%d + n=%d exceeds ld_seq=%d", what, max_pos, n, ld_seq);
  GPT2MI_REQUIRE(tok && seq && cum && done && P->logits, "%s: tok, seq, cum, done and plan->logits must not be NULL", what);
  if (const int rc = gpt2mi::decode_step_check(what, P, tok, pos0)) return rc;  // the plan, its buffers, the share map
  // the caches of the layers as one tensor: layer l at l * layer_rows rows behind layer 0, in all four tensors
  const gpt2mi_decode_layer* Y = P->layers;
  const bool fp8 = P->kv_format == GPT2MI_KV_FP8;
  const size_t rb = kv_row_bytes(P->kv_format);
  size_t layer_rows = 0;
  if (P->L > 1) {
    const ptrdiff_t d = (const char*)Y[1].kcache - (const char*)Y[0].kcache;
    GPT2MI_REQUIRE(d > 0 && (size_t)d % rb == 0, "%s: layers[1].kcache is not whole rows behind layers[0].kcache", what);
    layer_rows = (size_t)d / rb;
  }
  for (int l = 0; l < P->L; ++l) {
    bool ok = (const char*)Y[l].kcache == (const char*)Y[0].kcache + l * layer_rows * rb &&
              (const char*)Y[l].vcache == (const char*)Y[0].vcache + l * layer_rows * rb;
    if (fp8) ok = ok && Y[l].kscale == Y[0].kscale + l * layer_rows && Y[l].vscale == Y[0].vscale + l * layer_rows;
    GPT2MI_REQUIRE(ok, "%s: the caches of layer %d are not layer_rows=%zu rows behind layer 0's: the reorder takes the "
                   "layers as one tensor [L][B][H][Tcap]", what, l, layer_rows);
  }
  const size_t need = GPT2MI_BEAM_LOOP_BYTES + reorder_bytes(P->kv_format, P->L, P->H, R, win);
  GPT2MI_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu bytes given, %zu needed)", what, workspace_bytes,
                 need);
  GPT2MI_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0, "%s: workspace is NULL or not 16-byte aligned", what);
  char* ws = (char*)workspace;
  int32_t* top_id = (int32_t*)ws;
  float* top_lp = (float*)(ws + sizeof(int32_t) * GPT2MI_DECODE_MAX_B * GPT2MI_LOGPROBS_MAX_TOP);
  int32_t* parent_ws = (int32_t*)(ws + 8 * GPT2MI_DECODE_MAX_B * GPT2MI_LOGPROBS_MAX_TOP);
  const ReorderArgs ra = {Y[0].kcache, Y[0].vcache, Y[0].kscale, Y[0].vscale, P->kv_format, P->L, layer_rows, R, P->H,
                          P->Tcap, seq, ld_seq};
  int pos[GPT2MI_DECODE_MAX_B] = {};
  SeqCol sc = {seq, ld_seq, {}};
  for (int i = 0; i < n; ++i) {
    for (int b = 0; b < R; ++b) pos[b] = sc.col[b] = pos0[b] + i;
    beam_topw_kernel<<<R, SM_THREADS, 0, (hipStream_t)stream>>>(P->logits, P->Vp, V, W, top_id, top_lp);
    if (const int rc = gpt2mi::check_launch(what)) return rc;
    int32_t* parent = parents ? parents + (size_t)i * R : parent_ws;
    // (cum and done in place: select_launch's kernel reads a group's before it writes them)
    if (const int rc = select_launch(what, top_id, top_lp, cum, done, G, W, eos, tok, parent, cum, done, sc, stream))
      return rc;
    // rows take their parents' suffix [lo, pos0 + i): column pos0 + i, which the select just wrote, is not in it
    if (const int rc = reorder_launch(what, ra, parent, G, W, lo, pos, ws + GPT2MI_BEAM_LOOP_BYTES,
                                      workspace_bytes - GPT2MI_BEAM_LOOP_BYTES, stream))
      return rc;
    if (i + 1 < n)
      if (const int rc = gpt2mi::decode_step_as(what, P, tok, pos, stream)) return rc;
  }
  return 0;
}
