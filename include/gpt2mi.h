/*
 * gpt2mi.h — C ABI of libgpt2mi.so, the MI355X (gfx950) kernels of the GPT-2 training step.
 *
 * The reference (dpickem/gpt_2_distributed) has no native code and no FFI: its hot path is the
 * implicit aten/cuBLAS/NCCL work behind model.py + train_gpt2_distributed.py. Each entry below
 * replaces the aten work of the reference site cited next to it; the
 * Python binding is gpt_2_distributed_amd/_lib.py (ctypes), see INTEGRATION.md.
 *
 * Conventions
 *  - Every pointer is a DEVICE pointer allocated by the caller (PyTorch's caching allocator in
 *    the package). Kernels never allocate or free.
 *  - bf16 tensors are passed as uint16_t* (raw bf16 bits). Shapes are row-major with explicit
 *    leading dimensions (in elements).
 *  - `stream` is a hipStream_t passed as void*; all launches are asynchronous on it.
 *  - Return value: 0 on success; otherwise an errno-style (22 = invalid argument) or hipError_t
 *    code, with a message in gpt2mi_last_error() (thread-local).
 *  - Dropout (p > 0) uses a counter-based hash of (seed, element index) so backward regenerates
 *    the forward mask; p = 0 disables it.
 */
#ifndef GPT2MI_H
#define GPT2MI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPT2MI_ABI_VERSION 24
/* Counts additions that move no existing signature or struct: a caller written against (24, m) runs on any (24, >= m). */
#define GPT2MI_ABI_MINOR 6

const char* gpt2mi_last_error(void);
int gpt2mi_abi_version(void); /* returns GPT2MI_ABI_VERSION of the built library */
int gpt2mi_abi_minor(void);   /* returns GPT2MI_ABI_MINOR of the built library (v24.1; absent before) */

/* K1: x[b,t,:] = drop(wte[idx[b,t],:] + wpe[t,:])  — model.py:295-304 (embedding, add, dropout).
 * Rows with t >= T_valid are sequence padding (T rounded up to the attention tile by the engine): x = 0
 * there and neither table is read (wpe may have only T_valid rows). */
int gpt2mi_embed_fwd(const int64_t* idx, const float* wte, const float* wpe, float* x, int B, int T, int T_valid,
                     int C, float p, uint64_t seed, void* stream);
/* embedding_dense_backward of both tables: dwte[idx] += g, dwpe[t] += sum_b g (g = dres masked); rows
 * t >= T_valid are skipped. */
int gpt2mi_embed_bwd(const int64_t* idx, const float* dres, float* dwte, float* dwpe, int B, int T, int T_valid,
                     int C, float p, uint64_t seed, void* stream);
/* v24.6: the two above with positions that restart at every document of a packed row (packing.py doc_positions):
 * x[b,t,:] = drop(wte[idx[b,t],:] + wpe[t - start[b,t],:]) and dwpe[p] += the sum of g[b,t] over the rows with
 * t - start[b,t] == p, formed without floating-point atomics in an order fixed by the inputs. start is the int32 [B, T] doc_start of
 * gpt2mi_doc_bounds; a value outside [0, t] is clamped where it is read. The dropout decision of an element is the
 * one of the entries above. Rows t >= T_valid are padding as above (start is not read there); rows of wpe and dwpe
 * from the longest document's length on are neither read nor written. */
int gpt2mi_embed_fwd_doc(const int64_t* idx, const float* wte, const float* wpe, float* x, const int* start, int B,
                         int T, int T_valid, int C, float p, uint64_t seed, void* stream);
int gpt2mi_embed_bwd_doc(const int64_t* idx, const float* dres, float* dwte, float* dwpe, const int* start, int B,
                         int T, int T_valid, int C, float p, uint64_t seed, void* stream);

/* K2: nn.LayerNorm forward — model.py:204,210,247 (used :215,218,311). y_bf16 and/or y_f32 may be NULL. */
int gpt2mi_layernorm_fwd(const float* x, const float* w, const float* b, uint16_t* y_bf16, float* y_f32,
                         float* mean, float* rstd, int M, int C, float eps, void* stream);
/* native_layer_norm_backward fused with the residual gradient (dres += dx, or = dx if dres_init),
 * dw/db += ; optionally emits out_bf16 = bf16(dres*keep/(1-p_out)) for the residual branch below and
 * dbias_out += colsum(out_bf16) (that branch's bias grad). */
int gpt2mi_layernorm_bwd(const float* x, const float* w, const float* mean, const float* rstd, const uint16_t* dy,
                         float* dres, float* dw, float* db, uint16_t* out_bf16, float* dbias_out, int M, int C,
                         float p_out, uint64_t seed_out, int dres_init, void* stream);

/* Bias grad of an addmm: db[n] += sum_m g[m,n] (g bf16, row stride ld). */
int gpt2mi_colsum_bf16(const uint16_t* g, float* db, int M, int N, int ld, void* stream);

/* K3/K9/K10/K11/K12/K14 GEMMs — model.py:95-96,174-177,326 (nn.Linear under bf16 autocast) and their
 * autograd backward (train_gpt2_distributed.py:412).
 *   C[m,n] = epi(alpha*(alpha_dev?*alpha_dev:1) * sum_k A(m,k) B(n,k))
 * layout 0: A[M][K], B[N][K]   (x @ W^T)        layout 1: A[M][K], B[K][N]   (dY @ W, dgrad)
 * layout 2: A[K][M], B[K][N]   (dY^T @ X, wgrad)
 * epilogue 0 BF16: C bf16 (+bias)            1 F32: C fp32 (+bias), += when accumulate
 *          2 RESID: C fp32 = resid + drop(acc+bias)
 *          3 GELU: u = acc+bias, C = bf16(drop(gelu(u))), aux = bf16(keep/(1-p) * gelu'(u)) (what backward needs)
 *          4 GELU_BWD: C = bf16(acc * aux) (aux from the GELU forward)   5 ATOMIC: C fp32 += acc (split-K)
 * dbias (may be NULL; BF16 / GELU_BWD epilogues of layouts 0/1): dbias[n] += sum_m C[m][n] of the stored
 * output — the bias gradient of the Linear whose output grad C is (fused into the 256x256 epilogue).
 * Requires M, N multiples of 64 and K a multiple of 64*splits. The kernel is chosen by csrc/gemm_plan.h (plan_gemm):
 * the ping-pong 256x256 kernel for layout 0 (any N multiple of 64, K >= 128) and for layouts 1 / 2 with N (and, layout 2,
 * M) multiples of 256; otherwise the 2-stage 256x256 kernel (full tiles, K = 64) or the 128x128 kernel.
 * `sched`: GPT2MI_SCHED_* below. */
int gpt2mi_gemm(int layout, int epilogue, int M, int N, int K, const uint16_t* A, int lda, const uint16_t* B, int ldb,
                void* C, int ldc, const float* bias, const float* resid, uint16_t* aux, int ldaux, float alpha,
                const float* alpha_dev, int accumulate, int splits, float p_drop, uint64_t seed, float* dbias,
                int sched, void* stream);

/* GEMM schedule, chosen per call (v8; v7 had process-global switches):
 *  GPT2MI_SCHED_AUTO: the library picks the kernel (ping-pong 256x256; its persistent schedule for the short-K
 *    forward-layout shapes).
 *  GPT2MI_SCHED_NO_PERSISTENT (flag): never the persistent (one block per CU) schedule (one tile per block).
 *  GPT2MI_SCHED_SHARED_CUS (flag, v11): other kernels (the data-parallel wrappers' RCCL collectives) may hold CUs while
 *    this GEMM runs. The persistent schedule then takes its tiles from per-XCD work queues instead of a static walk:
 *    a block whose CU a collective holds takes fewer tiles instead of making the grid end on its latest block.
 *  low byte (the kernel-equivalence tests and A/B tools only): 0 = auto, 1 = 128x128 kernel, 2 = 2-stage 256x256,
 *    6 = ping-pong one tile per block (forward / dgrad layouts; weight gradients take the 2-stage kernel). Any other
 *    value is refused with 22 (v15 retired the experiment selectors 3, 4, 5, 7 and 8; gpt2mi_gemm_wgrad_kt has one
 *    kernel and ignores the low byte). */
#define GPT2MI_SCHED_AUTO 0
#define GPT2MI_SCHED_NO_PERSISTENT 0x100
#define GPT2MI_SCHED_SHARED_CUS 0x400
/* GPT2MI_SCHED_BF16_SLABS (flag, gpt2mi_gemm_wgrad / gpt2mi_gemm_wgrad_kt only; v10): each split-K partial sum is
 * rounded once to bf16 in its slab, then the slabs are summed in fp32 in split order (still deterministic) — half the
 * slab write and reduce traffic. The reference's autocast weight gradient rounds its whole sum to bf16 once
 * (torch.mm in bf16, cast to the fp32 .grad: train_gpt2_distributed.py:412); this rounds each of `splits` partial
 * sums, an error of the same order. Without the flag the slabs are fp32 (fp32-exact weight gradients). */
#define GPT2MI_SCHED_BF16_SLABS 0x200

/* Weight gradient (train_gpt2_distributed.py:412 autograd wgrad of every nn.Linear):
 * C[M][N] (+)= alpha*(alpha_dev?) * A^T B, A stored [K][M] (dY), B stored [K][N] (X), K = tokens.
 * 256x256 tiles; `splits` K ranges write fp32 (GPT2MI_SCHED_BF16_SLABS: bf16) partial slabs to `workspace`
 * (>= splits*M*N floats), summed into C in a fixed order (deterministic). M, N, K multiples of 64; ldc == N. sched: as gpt2mi_gemm
 * (the low byte 2 selects the 2-stage kernel). When M (N) is not a multiple of 256 (GPT-2 1.5B: 1600, 4800) the
 * partial last tile's reads are bounded by the operand's last element ((K-1)*lda + M, (K-1)*ldb + N; buffer
 * num_records): no slack past the operands is needed (v11; v10 read up to 192 elements past the last row). */
int gpt2mi_gemm_wgrad(int M, int N, int K, const uint16_t* A, int lda, const uint16_t* B, int ldb, float* C, int ldc,
                      int accumulate, float alpha, const float* alpha_dev, float* workspace, size_t workspace_floats,
                      int splits, int sched, void* stream);
/* The same weight gradient with B given transposed, k-contiguous: Bt stored [N][K] (X^T; train_gpt2_distributed.py:412,
 * the tied lm_head's wgrad against the final LayerNorm output transposed once per step). Computes C^T = Bt . A on the
 * ping-pong kernel (one transposed operand instead of two) into split-K slabs (workspace >= splits*M*N floats,
 * required) and sums them, transposed, into C (fixed order: the same bits as gpt2mi_gemm_wgrad). M multiple of 256,
 * N of 64, K of 128; ldc == N. ABI v9. */
int gpt2mi_gemm_wgrad_kt(int M, int N, int K, const uint16_t* A, int lda, const uint16_t* Bt, int ldbt, float* C,
                         int ldc, int accumulate, float alpha, const float* alpha_dev, float* workspace,
                         size_t workspace_floats, int splits, int sched, void* stream);

/* Grouped weight gradients (v13; train_gpt2_distributed.py:412, the autograd wgrads of a GPT2Block's four nn.Linear,
 * model.py:95,96,174,177): for g < count (<= 4), C[g][M[g]][N[g]] (+)= alpha*(alpha_dev?) * A[g]^T B[g] over the same
 * K tokens, as ONE split-K launch and ONE reduction launch. Host arrays of count entries; every M[g], N[g] a multiple of
 * 256, K of 128, ldc == N[g]; workspace >= splits * sum(M[g]*N[g]) floats. Each C[g] gets the bits gpt2mi_gemm_wgrad
 * gives it with the same `splits` and fp32 slabs. sched: GPT2MI_SCHED_AUTO or the CU-sharing flags (no BF16_SLABS). */
int gpt2mi_gemm_wgrad_grouped(int count, const int* M, const int* N, int K, const uint16_t* const* A, const int* lda,
                              const uint16_t* const* B, const int* ldb, float* const* C, int accumulate, float alpha,
                              const float* alpha_dev, float* workspace, size_t workspace_floats, int splits, int sched,
                              void* stream);

/* Batched weight gradients (v24.3; the same autograd wgrads, for every GPT2Block of the model at once): for g < count
 * (<= gpt2mi_gemm_wgrad_batch_max(), at least 4 x 36), C[g][M[g]][N[g]] (+)= alpha*(alpha_dev?) * A[g]^T B[g] over the
 * same K tokens as ONE launch WITHOUT split-K: one block per 256x256 output tile over all K, which writes or accumulates
 * C itself (no slabs, no reduction launch). Host arrays of count entries; every M[g], N[g] a multiple of 256, K of 128,
 * lda / ldb multiples of 8, ldc[g] >= N[g] a multiple of 4. Each C[g] gets the bits gpt2mi_gemm_wgrad gives it with
 * splits = 1. table: device scratch of gpt2mi_gemm_wgrad_batch_scratch(count) bytes, 16-byte aligned, which receives the
 * problem table by an asynchronous copy on `stream` ahead of the launch (no host synchronisation; not capturable into
 * a graph); it must stay untouched until the launch has run. The copy's source is pinned host staging the library keeps
 * for it (8 slots of 34 KB per device, allocated at the first call: the one allocation behind this ABI, host memory
 * only). sched as gpt2mi_gemm_wgrad_grouped. */
int gpt2mi_gemm_wgrad_batch(int count, const int* M, const int* N, int K, const uint16_t* const* A, const int* lda,
                            const uint16_t* const* B, const int* ldb, float* const* C, const int* ldc, int accumulate,
                            float alpha, const float* alpha_dev, void* table, size_t table_bytes, int sched,
                            void* stream);
size_t gpt2mi_gemm_wgrad_batch_scratch(int count); /* 0 for a count outside 1..max */
int gpt2mi_gemm_wgrad_batch_max(void);

/* K4-K8: causal flash attention, head_dim 64 — model.py:124-155. q/k/v read from qkv [B*T, 3C];
 * out [B*T, C] head-merged; lse [B*H, T] (natural log of the 1/sqrt(D)-scaled scores). */
int gpt2mi_attn_fwd(const uint16_t* qkv, uint16_t* out, float* lse, int B, int T, int H, int head_dim, float p_drop,
                    uint64_t seed, void* stream);
/* Backward: delta [B*H, T] workspace (dO.O, formed by the dQ pass); dqkv [B*T, 3C] written in the qkv
 * layout. dqkv_colsum (may be NULL): [B*T/32, 3C] fp32 partial column sums of the stored dqkv, one row
 * per 32 tokens — the qkv bias gradient after gpt2mi_colsum_f32 over its rows (model.py c_attn bias). */
int gpt2mi_attn_bwd(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse, float* delta,
                    uint16_t* dqkv, float* dqkv_colsum, int B, int T, int H, int head_dim, float p_drop,
                    uint64_t seed, void* stream);

/* K13: F.cross_entropy(logits.view(-1,V), labels.view(-1), ignore_index) — model.py:357-359.
 * logits bf16 [M, ld]; writes loss_rows [M], lse [M], loss[0] = mean, inv_count[0] = 1/#valid and, if
 * dlogits != NULL, dlogits = softmax - onehot (bf16 [M, ldd], unscaled, zero in columns >= V). A label
 * outside [0, V) other than ignore_index (F.cross_entropy raises) makes its loss row and dlogits row NaN. */
int gpt2mi_xent_fwd(const uint16_t* logits, int ld, const int64_t* labels, float* loss_rows, float* lse,
                    uint16_t* dlogits, int ldd, int M, int V, int ignore_index, float* loss, float* inv_count,
                    void* stream);

/* K15+K16: fused AdamW over a flat fp32 arena (torch.optim.AdamW(lr, weight_decay, betas, eps), one
 * param group, decoupled decay — train_gpt2_distributed.py:356-362,424) with g *= grad_scale, the
 * clip_grad_norm_(inf) total norm of the scaled grads -> grad_norm[0] (partials: workspace of
 * gpt2mi_norm_partials_size() floats), and the bf16 shadow p_bf16 (may be NULL). */
int gpt2mi_adamw(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, size_t n, float lr, float wd,
                 float b1, float b2, float eps, int step, float grad_scale, float* partials, float* grad_norm,
                 void* stream);
int gpt2mi_grad_norm(const float* g, size_t n, float scale, float* partials, float* out, void* stream);
/* v12: out[0] = sqrt(sum of partials[0..n)) — the norm of several gpt2mi_adamw launches given grad_norm = NULL and
 * consecutive gpt2mi_norm_partials_size()-float slices of one partials buffer (FSDP's AdamW runs once per unit). */
int gpt2mi_norm_finalize(const float* partials, int n, float* out, void* stream);
int gpt2mi_norm_partials_size(void);
/* v16: global-norm gradient clipping with the coefficient kept in device memory (nothing here reads it back).
 * gpt2mi_sumsq_partials: gpt2mi_norm_partials_size() partial sums of (g*scale)^2 over g[0..n), n % 4 == 0; several
 *   ranges fill consecutive slices of one buffer (the pieces of the arena around a DDP bucket, the FSDP units).
 * gpt2mi_clip_coef: over partials[0..n) (n >= 1): norm_out[0] = sqrt(sum), the bits gpt2mi_norm_finalize gives;
 *   sumsq_out[0] (may be NULL) = the fp32 sum, for a cross-rank all-reduce (then call again with n = 1 on it);
 *   coef_out[0] = min(1, max_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s coefficient: NaN for a NaN norm,
 *   0 for an infinite one.
 * gpt2mi_adamw_clipped: gpt2mi_adamw with every gradient scaled by grad_scale * coef_dev[0]. partials and grad_norm
 *   may be NULL (they would see the clipped gradients; the pre-clip norm is gpt2mi_clip_coef's). */
int gpt2mi_sumsq_partials(const float* g, size_t n, float scale, float* partials, void* stream);
int gpt2mi_clip_coef(const float* partials, int n, float max_norm, float* sumsq_out, float* norm_out, float* coef_out,
                     void* stream);
int gpt2mi_adamw_clipped(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, size_t n, float lr, float wd,
                         float b1, float b2, float eps, int step, float grad_scale, const float* coef_dev,
                         float* partials, float* grad_norm, void* stream);

/* ---- fp32 mode: the reference model.py run WITHOUT torch.autocast (plain fp32 module; the CPU
 * trajectory goldens and the north star's "fp32 loss within 1e-4" gate). Same contracts as the bf16
 * entries above with every activation / weight operand fp32 (C and aux of the "BF16", GELU and
 * GELU_BWD epilogues are fp32 too). GEMM products are exact fp32 (v_mfma_f32_16x16x4_f32). ---- */
/* K3/K9-K12/K14 in fp32: N % 4 == 0, K % (16*splits) == 0, leading dims % 4 == 0. */
int gpt2mi_gemm_f32(int layout, int epilogue, int M, int N, int K, const float* A, int lda, const float* B, int ldb,
                    void* C, int ldc, const float* bias, const float* resid, float* aux, int ldaux, float alpha,
                    const float* alpha_dev, int accumulate, int splits, float p_drop, uint64_t seed, float* dbias,
                    void* stream);
/* K4-K8 in fp32 (model.py:124-155 without autocast); same dropout mask as gpt2mi_attn_fwd. */
int gpt2mi_attn_fwd_f32(const float* qkv, float* out, float* lse, int B, int T, int H, int head_dim, float p_drop,
                        uint64_t seed, void* stream);
int gpt2mi_attn_bwd_f32(const float* qkv, const float* out, const float* dout, const float* lse, float* delta,
                        float* dqkv, float* dqkv_colsum /* must be NULL */, int B, int T, int H, int head_dim,
                        float p_drop, uint64_t seed, void* stream);
/* LayerNorm backward with fp32 dy and fp32 branch output (see gpt2mi_layernorm_bwd). */
int gpt2mi_layernorm_bwd_f32(const float* x, const float* w, const float* mean, const float* rstd, const float* dy,
                             float* dres, float* dw, float* db, float* out_f32, float* dbias_out, int M, int C,
                             float p_out, uint64_t seed_out, int dres_init, void* stream);
int gpt2mi_colsum_f32(const float* g, float* db, int M, int N, int ld, void* stream);
/* K13 on fp32 logits (the fp32 lm_head output), fp32 dlogits. */
int gpt2mi_xent_fwd_f32(const float* logits, int ld, const int64_t* labels, float* loss_rows, float* lse,
                        float* dlogits, int ldd, int M, int V, int ignore_index, float* loss, float* inv_count,
                        void* stream);

/* dst[c][r] = src[r][c] for a bf16 [R][C] matrix (R, C multiples of 64): the transposed weight shadow
 * the backward dgrad GEMMs read in the forward (k-contiguous) layout. */
int gpt2mi_transpose_bf16(const uint16_t* src, uint16_t* dst, int R, int C, int ld_src, int ld_dst, void* stream);
/* All weights of a shadow arena in one launch: desc (device, int64 [n][4]) = {element offset, R, C, first
 * tile index} with R, C multiples of 64 and first tiles the prefix sums of (R/64)*(C/64); src + offset is a
 * dense [R][C] matrix, dst + offset receives its [C][R] transpose. */
int gpt2mi_transpose_bf16_batched(const uint16_t* src, uint16_t* dst, const int64_t* desc, int n,
                                  int64_t total_tiles, void* stream);
int gpt2mi_cast_f32_bf16(const float* x, uint16_t* y, size_t n, void* stream);
int gpt2mi_cast_bf16_f32(const uint16_t* x, float* y, size_t n, void* stream);

/* ---- v5: the boundary around the fused step (aux_ops.hip) ---- */
/* Gradient entering through the returned logits (model.py:351: logits are returned and differentiable):
 * dl[b*Tp+t][n] = (init ? 0 : alpha_dev[0]*dl) + g[b*Tv+t][n] for t < Tv, n < V; dl columns [V, ldd) = 0;
 * rows t >= Tv (sequence padding) are zeroed when init, else untouched. dl is the lm_head backward's
 * dlogits (bf16 [B*Tp, ldd]); g the caller's grad of the [B, Tv, V] logits (row stride ldg). */
int gpt2mi_dlogits_accum(uint16_t* dl, int ldd, const uint16_t* g, int ldg, int B, int Tp, int Tv, int V,
                         const float* alpha_dev, int init, void* stream);
int gpt2mi_dlogits_accum_f32(float* dl, int ldd, const float* g, int ldg, int B, int Tp, int Tv, int V,
                             const float* alpha_dev, int init, void* stream);
/* Residual-branch output gradient of a stand-alone sub-module backward (model.py:158,191: resid_drop /
 * drop2 then the branch bias): out = dres*keep/(1-p) (bf16 [M,C]; fp32 for _f32), dbias += colsum(out). */
int gpt2mi_branch_bwd(const float* dres, uint16_t* out, float* dbias, int M, int C, float p, uint64_t seed,
                      void* stream);
int gpt2mi_branch_bwd_f32(const float* dres, float* out, float* dbias, int M, int C, float p, uint64_t seed,
                          void* stream);
/* x *= s (n % 4 == 0): DDP's division of a gradient bucket by the world size before a SUM all-reduce
 * (torch/nn/parallel/distributed.py reducer; train_gpt2_distributed.py:163). */
int gpt2mi_scale_f32(float* x, size_t n, float s, void* stream);
/* FSDP flat units (train_gpt2_distributed.py:146-161, MixedPrecision(param=bf16, reduce=bf16)):
 * unpack a gathered unit into the fp32 parameter view and the bf16 GEMM shadow (either may be NULL);
 * pack a unit's fp32 grads into the zero-padded reduce-scatter input (bf16 or fp32);
 * accumulate the reduce-scattered shard into the fp32 grad shard (= when accumulate == 0). */
int gpt2mi_fsdp_unpack(const void* src, int src_f32, float* dst_f32, uint16_t* dst_bf16, size_t n, void* stream);
int gpt2mi_fsdp_pack(const float* src, void* dst, int dst_f32, size_t n, size_t n_pad, void* stream);
int gpt2mi_fsdp_accum(const void* src, int src_f32, float* dst, size_t n, int accumulate, void* stream);
int gpt2mi_scale_mul(const float* a, const float* b, float* out, void* stream);
int gpt2mi_memset_zero(void* ptr, size_t bytes, void* stream);
/* Zero n element ranges of a float array in one launch; ranges = DEVICE int64 pairs (offset, count).
 * Replaces, for the atomically accumulated slots of the grad arena (LayerNorm params, biases, wpe, ln_f),
 * the full-arena zero of optimizer.zero_grad() (torch/optim/optimizer.py zero_grad via
 * train_gpt2_distributed.py:409-425) when the backward's weight-gradient GEMMs write their slots outright. */
int gpt2mi_zero_ranges(float* base, const int64_t* ranges, int n, void* stream);

/* ---- v14: autoregressive decode (csrc/decode.hip). The reference has no generation loop; these are the nanoGPT /
 * llm.c style `generate` of the model.py forward (model.py:335-351) with a per-layer key/value cache, one token per
 * sequence and step. bf16 operands, fp32 accumulation, head_dim 64, no dropout, no atomics: every reduction runs in
 * a fixed order, so outputs are bitwise reproducible.
 * v20: the entries of this block that take one position `pos` for the whole batch (gpt2mi_attn_decode,
 * gpt2mi_embed_decode, gpt2mi_decode_step) are forwarders: they check pos, then call the per-row implementation of the
 * v19 block below with pos[b] = pos for every row. So they take 1 <= B <= GPT2MI_DECODE_MAX_B like it (before v20
 * gpt2mi_attn_decode took any B * H <= 65535 and gpt2mi_embed_decode any B) and refuse a larger B with 22. ---- */
/* Skinny forward GEMM (nn.Linear at M = batch rows): C[m][n] = epi(sum_k A[m][k] W[n][k] + bias[n]), A bf16 [M][K]
 * (row stride lda), W bf16 [N][K] (row stride ldw: the forward layout of the weight shadow), 1 <= M <= 64, N and K
 * multiples of 64 (N need not be a multiple of 256). epilogue: 0 BF16 (+bias), 1 F32 (+bias), 2 RESID: C fp32 =
 * resid + acc + bias (resid row stride ldc, not aliasing C), 3 GELU: C = bf16(gelu_tanh(acc + bias)) (no aux). bias may
 * be NULL. W streams from HBM once, in 16-column strips; K is split across the waves of a block and, while the
 * strips alone leave CUs idle, across blocks whose fp32 partial sums go through `workspace`
 * (>= gpt2mi_gemm_skinny_workspace(M, N, K) floats; may be NULL when that is 0) and are summed in split order. The
 * split depends on (N, K) only and every output row is formed from its own A row: row m has the same bits at any M. */
int gpt2mi_gemm_skinny(int epilogue, int M, int N, int K, const uint16_t* A, int lda, const uint16_t* W, int ldw,
                       void* C, int ldc, const float* bias, const float* resid, float* workspace,
                       size_t workspace_floats, void* stream);
size_t gpt2mi_gemm_skinny_workspace(int M, int N, int K);
/* Prefill's cache fill: for b < B, t < n copy the K and V columns of row b*T_src + t of qkv [B*T_src, 3C] (C = H*64)
 * to position t0 + t of kcache / vcache, each bf16 [B][H][Tcap][64] (one layer). Rows t >= n of a sequence (tile
 * padding) are not copied; nothing else of the cache is written. */
int gpt2mi_kv_store(const uint16_t* qkv, uint16_t* kcache, uint16_t* vcache, int B, int T_src, int n, int t0, int H,
                    int head_dim, int Tcap, void* stream);
/* Single-query attention over the cache (model.py:124-155 for the newest position): qkv bf16 [B, 3C] of the new
 * token; its k and v are written to position pos of the caches, and out[b, h*64..] = softmax(q.K[0..pos]^T / 8)
 * V[0..pos] (bf16 [B, C]). Keys are split in ranges of 32 across workgroups; the partial (max, sum, acc) go through
 * `workspace` (>= gpt2mi_attn_decode_workspace(B, H, Tcap) floats) and are combined in range order. Cache positions
 * > pos are neither read nor written. A forwarder (v20): gpt2mi_attn_decode_ragged with every pos[b] = pos, after
 * "pos=%d not in [0, Tcap)"; B <= GPT2MI_DECODE_MAX_B. */
int gpt2mi_attn_decode(const uint16_t* qkv, uint16_t* kcache, uint16_t* vcache, uint16_t* out, float* workspace,
                       size_t workspace_floats, int B, int H, int head_dim, int Tcap, int pos, void* stream);
size_t gpt2mi_attn_decode_workspace(int B, int H, int Tcap);
/* K1 for one new token per sequence: x[b,:] = wte[tok[b],:] + wpe[pos,:] (fp32, no dropout). A forwarder (v20):
 * gpt2mi_embed_decode_ragged with every pos[b] = pos >= 0; B <= GPT2MI_DECODE_MAX_B. */
int gpt2mi_embed_decode(const int64_t* tok, const float* wte, const float* wpe, float* x, int B, int C, int pos,
                        void* stream);

/* One decode step as one call (about 10 launches per layer without a Python round trip each). All pointers device
 * memory except `layers` (a host array of L entries). */
typedef struct gpt2mi_decode_layer {
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;             /* fp32 [C] */
  const uint16_t *qkv_w, *proj_w, *fc1_w, *fc2_w;         /* bf16 [3C][C], [C][C], [4C][C], [C][4C] */
  const float *qkv_b, *proj_b, *fc1_b, *fc2_b;            /* fp32 */
  uint16_t *kcache, *vcache;                              /* bf16 [B][H][Tcap][64]; with plan->kv_format = 1 the
                                                             fp8 codes, uint8 [B][H][Tcap][64], behind a cast */
  float *kscale, *vscale;                                 /* v23, appended: fp32 [B][H][Tcap], the scales of an fp8
                                                             cache; not read (may be NULL) with kv_format = 0 */
} gpt2mi_decode_layer;
typedef struct gpt2mi_decode_plan {
  int B, C, H, L, Vp, Tcap;                               /* batch, n_embd, heads, layers, padded vocab, cache length */
  float eps;                                              /* LayerNorm eps */
  const float *wte, *wpe, *lnf_w, *lnf_b;                 /* fp32 tables and the final LayerNorm */
  const uint16_t* wte_bf16;                               /* bf16 [Vp][C]: the tied lm_head */
  const gpt2mi_decode_layer* layers;                      /* host array [L] */
  float *x, *xmid;                                        /* fp32 [B][C] residual stream */
  uint16_t *ln, *qkv, *ao, *h;                            /* bf16 [B][C], [B][3C], [B][C], [B][4C] */
  float *mean, *rstd;                                     /* fp32 [B] */
  float* attn_ws;                                         /* gpt2mi_attn_decode_workspace(B, H, Tcap) floats */
  size_t attn_ws_floats;
  float* gemm_ws;                                         /* the largest gpt2mi_gemm_skinny_workspace of the step */
  size_t gemm_ws_floats;
  float* logits;                                          /* fp32 [B][Vp] */
  int rows;                                               /* v21, appended (no earlier offset moved): the rows the
                                                             scratch buffers above (x .. logits, the workspaces) hold;
                                                             0 means B. Read by gpt2mi_decode_extend only. */
  int kv_format;                                          /* v23, appended: GPT2MI_KV_BF16 (0, what a zeroed field
                                                             meant before) or GPT2MI_KV_FP8 (1): see the v23 block.
                                                             On LP64 it fills the former tail padding behind `rows`:
                                                             sizeof(gpt2mi_decode_plan) did not change */
  const int* share_group;                                 /* v24, appended (no earlier offset moved; the struct grows
                                                             by the two pointers): with share_len the share map of the
                                                             v24 block, HOST arrays of B ints read during the call
                                                             only. Both NULL (what a zeroed field means) is v23's
                                                             behaviour, launch for launch. Read by gpt2mi_decode_step*
                                                             and gpt2mi_decode_generate_ragged / _penalized; ignored by
                                                             gpt2mi_decode_extend */
  const int* share_len;
} gpt2mi_decode_plan;
/* embed -> per layer (LN1, qkv, attention at pos, proj + resid, LN2, fc1 + GELU, fc2 + resid) -> ln_f -> lm_head into
 * plan->logits, for the B tokens `tok` (device int64 [B]) at position pos (model.py:295-351 at one position). A
 * forwarder (v20): gpt2mi_decode_step_ragged with every pos[b] = pos in [0, plan->Tcap). */
int gpt2mi_decode_step(const gpt2mi_decode_plan* plan, const int64_t* tok, int pos, void* stream);

/* ---- v17: device-side sampling (csrc/sample.hip) and the token loop around it. The executable specification of the
 * rule is gpt_2_distributed_amd/generation.py sample_reference + uniform_at (nanoGPT's temperature / top-k rule, as
 * generation.py sample_next, plus nucleus filtering and a counter-based draw).
 * v20: gpt2mi_sample and gpt2mi_decode_generate are forwarders to their v19 per-row forms (one kernel, one loop), so
 * gpt2mi_sample takes 1 <= B <= GPT2MI_DECODE_MAX_B (before v20: any B) and refuses a larger B with 22. ---- */
/* Largest vocabulary gpt2mi_sample takes: one 1024-thread workgroup holds a row in registers, 50 logits per thread. */
#define GPT2MI_SAMPLE_MAX_V 51200
/* One token per row b < B from logits fp32 [B][ldl] (columns V..ldl-1 are padding and are not read). One launch, one
 * workgroup per row; the row is read once.
 *  temperature == 0: the argmax, the lowest index among equal maxima (top_k, top_p, seed ignored; probs_out one-hot).
 *  otherwise x = logits / temperature (IEEE fp32 division), then
 *   top_k (1 <= top_k < V; else off): keep x >= the k-th largest value of the row (ties at it all kept);
 *   top_p (0 < top_p < 1; >= 1 off), on p = softmax of what top-k kept: keep token i iff the total p of the tokens
 *     with a value strictly larger than x_i is < top_p (ties at the threshold all kept, the largest always kept);
 *   draw: u = (h >> 40) * 2^-24 with h = splitmix64's finaliser of seed + 0x9E3779B97F4A7C15 * (1 + (b << 32 | pos));
 *     the token is the first kept index i, in vocabulary order, whose inclusive cumulative p exceeds u * Z (Z = the kept
 *     mass): a pure function of (row, parameters, seed, b, pos), whatever B is.
 *  eos (-1: none) / done (uint8 [B], may be NULL): a row whose done flag is set emits eos; otherwise a row that draws eos
 *   sets its flag.
 *  Writes tok_out[b], seq_out[b*ld_seq + pos] (seq_out may be NULL) and, for tests, probs_out [B][V] (may be NULL): the
 *   kept distribution, p_i / Z, zero where filtered.
 * No float atomics; every float reduction and scan runs in a fixed order: two calls give the same bits.
 * Refused with 22 before any launch: B outside [1, GPT2MI_DECODE_MAX_B], V < 1 or > GPT2MI_SAMPLE_MAX_V, ldl < V,
 * temperature < 0 or NaN, top_p <= 0 or NaN, pos < 0, eos outside [-1, V), ld_seq <= pos with seq_out, NULL logits or
 * tok_out. A forwarder (v20): gpt2mi_sample_ragged with every pos[b] = pos and row_id = NULL (the draw key of row b is
 * b). */
int gpt2mi_sample(const float* logits, int ldl, int B, int V, float temperature, int top_k, float top_p, uint64_t seed,
                  int pos, int64_t eos, uint8_t* done, int64_t* tok_out, int64_t* seq_out, int ld_seq, float* probs_out,
                  void* stream);
/* n tokens per sequence without returning to the caller: for i < n, gpt2mi_sample from plan->logits (V valid columns)
 * at position pos0 + i into tok (device int64 [B]) and seq[:, pos0 + i] (seq may be NULL), then, if i + 1 < n,
 * gpt2mi_decode_step(plan, tok, pos0 + i). On entry plan->logits holds the logits for position pos0 (the prefill's or
 * the previous step's); on return the token of position pos0 + n - 1 is in tok and has not been stepped. A host loop of
 * launches on `stream`: nothing is synchronised or read back. n = 0 launches nothing. pos0 >= 1 (after a prefill) and
 * pos0 + n <= plan->Tcap; pos0 < plan->Tcap also when n = 0. A forwarder (v20): gpt2mi_decode_generate_ragged with every
 * pos0[b] = pos0 and row_id = NULL. */
int gpt2mi_decode_generate(const gpt2mi_decode_plan* plan, int V, float temperature, int top_k, float top_p,
                           uint64_t seed, int64_t eos, int pos0, int n, int64_t* tok, int64_t* seq, int ld_seq,
                           uint8_t* done, void* stream);

/* ---- v18: evaluation (csrc/lm_loss.hip). The loss rows of F.cross_entropy(x @ w[:V].T, labels, ignore_index) without
 * forming the logits: the tied lm_head GEMM (bf16 operands, fp32 accumulation) fused with the cross-entropy reduction,
 * so the semantics are gpt2mi_xent_fwd's on the un-rounded fp32 logits. ----
 *  x bf16 [M][ldx] (K valid columns: the ln_f output), w bf16 [w_rows][ldw] (the tied wte shadow; rows V..w_rows-1 are
 *   padding whose contents do not matter: columns >= V of the logits never contribute, rows >= w_rows are never read).
 *  loss_rows [M] = lse - logit[label], 0 where label == ignore_index, NaN where the label is outside [0, V) otherwise
 *   (the sums are then NaN too); lse [M] = log-sum-exp of the row. Either may be NULL.
 *  loss_sum[0] / count[0] (may be NULL): the sum of loss_rows and the number of labels != ignore_index of THIS call,
 *   written (accumulate = 0) or added to what they hold (accumulate = 1: a running token-weighted total over calls).
 *  loss_mean[0] (may be NULL) = this call's sum / count (NaN when every label is ignored, as gpt2mi_xent_fwd's loss).
 *  workspace: gpt2mi_lm_loss_workspace(M, V) bytes of fp32 (per-split row partials; a function of M and V only).
 * Two launches, no float atomics, every reduction in a fixed order: two calls give the same bits.
 * Refused with 22 before any launch: M or K not a positive multiple of 64, V < 1, w_rows < V, a row stride < K or not
 * a multiple of 8, NULL x / w / labels / workspace. */
int gpt2mi_lm_loss(const uint16_t* x, int ldx, const uint16_t* w, int ldw, int w_rows, const int64_t* labels, int M,
                   int V, int K, int ignore_index, float* loss_rows, float* lse, float* loss_sum, float* count,
                   int accumulate, float* loss_mean, float* workspace, void* stream);
size_t gpt2mi_lm_loss_workspace(int M, int V); /* bytes; 0 for M < 1 or V < 1 */

/* ---- v19: ragged decode (csrc/decode.hip, csrc/sample.hip). The entries above put every sequence of a batch at one
 * position; these take one position per row, so prompts of unequal length share a batch and a finished row can be
 * replaced while the others go on (generation.py DecodeSession.refill, generate_many). Since v20 these are the one
 * implementation of each operation, with one set of kernels: the scalar-position entries above forward to them, and
 * the package calls only these.
 * A position array is `const int* pos`: a HOST array of B ints, 1 <= B <= GPT2MI_DECODE_MAX_B. The entry checks every
 * element before any launch and passes the array to its kernels by value, as a kernel argument: there is no device-side
 * position array, so no position reaches a kernel unchecked, nothing is copied to the device and the caller's array may
 * be reused as soon as the call returns.
 * Refused with 22 before any launch, beside the checks stated at the scalar entry: B outside [1, GPT2MI_DECODE_MAX_B], a
 * NULL position array, a pos[b] outside the range stated at the entry, ld_seq <= pos[b] with a seq_out. ---- */
#define GPT2MI_DECODE_MAX_B 64
/* gpt2mi_attn_decode with row b at pos[b] in [0, Tcap) (model.py:124-155 for the newest position of each row): row b's
 * k and v are written to position pos[b] of its streams and out[b] attends over positions 0..pos[b]. The grid covers
 * max_b pos[b] / 32 + 1 key ranges; a wave whose range starts beyond its row's position exits before any load or
 * store, and the combine merges pos[b] / 32 + 1 ranges of row b in range order. Workspace: size and layout of
 * gpt2mi_attn_decode_workspace(B, H, Tcap). Per row: cache positions != pos[b] are not written, positions > pos[b] are
 * not read; no atomics. The bits of out[b] and of row b's cache depend on row b's inputs and pos[b] only: they are
 * those gpt2mi_attn_decode gives that row at pos = pos[b] (the same kernels). */
int gpt2mi_attn_decode_ragged(const uint16_t* qkv, uint16_t* kcache, uint16_t* vcache, uint16_t* out, float* workspace,
                              size_t workspace_floats, int B, int H, int head_dim, int Tcap, const int* pos,
                              void* stream);
/* K1 for one new token per sequence at its own position: x[b,:] = wte[tok[b],:] + wpe[pos[b],:] (model.py:295-304
 * at one position per row; fp32, no dropout), pos[b] >= 0. */
int gpt2mi_embed_decode_ragged(const int64_t* tok, const float* wte, const float* wpe, float* x, int B, int C,
                               const int* pos, void* stream);
/* gpt2mi_sample with a position and a draw key per row: row b draws u from (seed, row_id[b], pos[b]) in place of
 * (seed, b, pos) and writes seq_out[b*ld_seq + pos[b]]; pos[b] >= 0. row_id is a HOST array of B values and may be NULL
 * (row_id[b] = b): it lets a sequence keep its draw stream whichever row of the batch it occupies. Everything else
 * (filtering, scan, draw, eos / done indexed by b, tok_out[b], probs_out) is as stated at gpt2mi_sample. */
int gpt2mi_sample_ragged(const float* logits, int ldl, int B, int V, float temperature, int top_k, float top_p,
                         uint64_t seed, const int* pos, const uint32_t* row_id, int64_t eos, uint8_t* done,
                         int64_t* tok_out, int64_t* seq_out, int ld_seq, float* probs_out, void* stream);
/* gpt2mi_decode_step with row b at pos[b] in [0, plan->Tcap) (model.py:295-351 at one position per row): the sequence
 * stated there with the embedding and the attention of this block; LayerNorm and the skinny GEMMs do not see positions. */
int gpt2mi_decode_step_ragged(const gpt2mi_decode_plan* plan, const int64_t* tok, const int* pos, void* stream);
/* gpt2mi_decode_generate with row b starting at pos0[b] >= 1: for i < n, gpt2mi_sample_ragged at pos0[b] + i (draw key
 * row_id[b], may be NULL), then, if i + 1 < n, gpt2mi_decode_step_ragged at pos0[b] + i. max_b pos0[b] + n <= Tcap (and
 * <= ld_seq with seq) is checked before the first launch. */
int gpt2mi_decode_generate_ragged(const gpt2mi_decode_plan* plan, int V, float temperature, int top_k, float top_p,
                                  uint64_t seed, int64_t eos, const int* pos0, const uint32_t* row_id, int n,
                                  int64_t* tok, int64_t* seq, int ld_seq, uint8_t* done, void* stream);

/* ---- v21: several rows of one launch in the same sequence (csrc/decode.hip). A step appends one token per sequence;
 * these append a run of tokens to a live sequence in one pass over the weights: a second user turn, a prompt suffix, or
 * a chunk of draft tokens to verify (generation.py DecodeSession.extend, speculate).
 * The row map is two HOST arrays of R ints, 1 <= R <= GPT2MI_DECODE_MAX_B: row r is (sequence seq[r] in [0, B), position
 * pos[r] in [0, Tcap)). seq must not decrease, and where seq[r] == seq[r-1], pos[r] == pos[r-1] + 1: the rows of a
 * sequence are one contiguous run at consecutive positions. A sequence may be absent and a run may start at 0. The entry
 * checks every element before any launch and passes the map (with each run's first position, derived on the host) to
 * the kernel by value, indexed by the block index only: there is no device-side index array. These checks are what
 * make every derived index in range: the qkv row of the run's position t, r - (pos[r] - t) for first <= t <= pos[r],
 * is never below the run's first row, and every cache index (seq[r], h, t <= pos[r]) lies inside [B][H][Tcap].
 * Refused with 22 and a message before any launch: R outside [1, GPT2MI_DECODE_MAX_B], a NULL seq or pos array, seq[r]
 * outside [0, B), a decreasing seq, pos[r] outside [0, Tcap), seq[r] == seq[r-1] with pos[r] != pos[r-1] + 1, a
 * workspace or row capacity too small, a NULL pointer. ---- */
/* Single-query attention for R rows, qkv bf16 [R][3C], caches bf16 [B][H][Tcap][64] (one layer), out bf16 [R][C]:
 * out[r] = softmax(q_r . K[0..pos[r]]^T / 8) V[0..pos[r]] over sequence seq[r], with gpt2mi_attn_decode_ragged's
 * arithmetic lane for lane (one wave per 32 keys, head and row; the in-order combine of pos[r] / 32 + 1 ranges). A key
 * at a position below the run's first comes from the cache; a key at first..pos[r] comes from the qkv row of the run
 * at that position and is never read from the cache (other waves of the launch are writing it). The row at position t
 * writes its k / v to position t of its sequence's streams: one writer per position, nothing above pos[r] read, streams
 * of absent sequences untouched, no atomics. Workspace: size and layout of gpt2mi_attn_decode_workspace(R, H, Tcap),
 * slots indexed by row. out[r] and the caches have the bits that R calls of gpt2mi_attn_decode_ragged, one position at
 * a time, give. */
int gpt2mi_attn_extend(const uint16_t* qkv, uint16_t* kcache, uint16_t* vcache, uint16_t* out, float* workspace,
                       size_t workspace_floats, int R, int B, int H, int head_dim, int Tcap, const int* seq,
                       const int* pos, void* stream);
/* gpt2mi_decode_step_ragged's launch list on R rows: the embedding of tok (device int64 [R]) at pos[r], LayerNorm and
 * the skinny GEMMs at M = R, gpt2mi_attn_extend in place of the attention, and the lm_head of all R rows into
 * plan->logits, fp32 [R][Vp]. plan->B is the number of sequences of the caches; the scratch buffers of the plan hold
 * plan->rows rows (0: B) and R must not exceed that. A row's activations do not depend on the other rows of a launch
 * (gpt2mi_gemm_skinny, LayerNorm), so logits row r and the caches have the bits of feeding the same tokens through
 * gpt2mi_decode_step_ragged one position at a time. */
int gpt2mi_decode_extend(const gpt2mi_decode_plan* plan, int R, const int64_t* tok, const int* seq, const int* pos,
                         void* stream);

/* ---- v22: repetition, presence and frequency penalties in the sampler (csrc/sample.hip, csrc/decode.hip). A token's
 * history moves its logit before everything gpt2mi_sample states (the greedy argmax, the temperature division, top-k,
 * top-p, the draw). The executable specification is gpt_2_distributed_amd/generation.py apply_penalties.
 * Row b's history is hist[hist_row[b]][0 .. pos[b]) (values outside [0, V) are ignored). Per vocabulary index i,
 * seen_i = i occurs in [0, pos[b]) (prompt and generated tokens: HF's scope of repetition_penalty) and c_i = its
 * occurrences in [gen_start[b], pos[b]) (generated tokens: the OpenAI / vLLM scope). In this order, every operation one
 * IEEE fp32 operation rounded to nearest, none contracted:
 *   repetition != 1 and seen_i:  x = x < 0 ? x * repetition : x / repetition   (a logit of exactly 0 is divided)
 *   frequency != 0 and c_i > 0:  x = x - (frequency * float(c_i))
 *   presence != 0 and c_i > 0:   x = x - presence
 * The kernels are instantiations of the sampling kernel of their own: the row is still read once and the logits buffer
 * is not written; the counts live in LDS (16 bits per vocabulary index, integer LDS atomics: no table in global memory,
 * no float atomics, two calls give the same bits). ---- */
/* Longest history window (pos[b]) a penalised draw takes. */
#define GPT2MI_PENALTY_MAX_HISTORY 8192
typedef struct gpt2mi_penalties {
  float repetition, presence, frequency; /* 1, 0, 0: off */
  const int64_t* hist;                   /* device int64 [hist_rows][ld_hist] */
  int ld_hist, hist_rows;
  const int* hist_row;                   /* HOST [B], may be NULL (row b reads hist row b) */
  const int* gen_start;                  /* HOST [B], may be NULL (0) */
} gpt2mi_penalties;
/* gpt2mi_sample_ragged with penalties: row b reads hist[hist_row[b]][0 .. pos[b]) and draws at pos[b]. seq_out may
 * alias hist (a block reads positions < pos[b] of its row and writes position pos[b]). logits_out (fp32 [B][V], may be
 * NULL) receives the penalised logits, before the temperature division. The host arrays travel to the kernel by value.
 * pen == NULL or (1, 0, 0) launches gpt2mi_sample_ragged's kernels (its bits, launches and cost; hist may be NULL, the
 * arrays are not read; a logits_out is then a device-to-device copy of the valid columns queued before the launch).
 * Refused with 22 and a message before any launch, beside gpt2mi_sample_ragged's checks: repetition <= 0 or NaN, a
 * non-finite presence or frequency; and with non-neutral values a NULL hist, ld_hist < pos[b], hist_row[b] outside
 * [0, hist_rows) (hist_rows < B without a hist_row), gen_start[b] outside [0, pos[b]], pos[b] above
 * GPT2MI_PENALTY_MAX_HISTORY. */
int gpt2mi_sample_penalized(const float* logits, int ldl, int B, int V, float temperature, int top_k, float top_p,
                            uint64_t seed, const int* pos, const uint32_t* row_id, int64_t eos, uint8_t* done,
                            int64_t* tok_out, int64_t* seq_out, int ld_seq, float* probs_out,
                            const gpt2mi_penalties* pen, float* logits_out, void* stream);
/* gpt2mi_decode_generate_ragged with penalties and seq as the history: row b must hold its tokens at seq[b][0 .. pos0[b])
 * (the loop appends what it draws), gen_start (HOST [B], may be NULL: 0) is where its generated part starts. seq is
 * required when a value is non-neutral; (1, 0, 0) is gpt2mi_decode_generate_ragged. Refused with 22 before any launch,
 * beside its checks: the value checks above, a NULL seq or gen_start[b] outside [0, pos0[b]] with non-neutral values,
 * max pos0 + n - 1 above GPT2MI_PENALTY_MAX_HISTORY. */
int gpt2mi_decode_generate_penalized(const gpt2mi_decode_plan* plan, int V, float temperature, int top_k, float top_p,
                                     uint64_t seed, int64_t eos, const int* pos0, const uint32_t* row_id, int n,
                                     int64_t* tok, int64_t* seq, int ld_seq, uint8_t* done, void* stream,
                                     float repetition, float presence, float frequency, const int* gen_start);

/* ---- v23: an fp8 key/value cache (csrc/decode.hip). The bf16 cache is 128 bytes per (head, position) and tensor; this
 * one is 64 OCP e4m3 codes and one fp32 scale, 68 bytes. The executable specification of the format is
 * gpt_2_distributed_amd/generation.py kv_quantize / kv_dequantize.
 * One scale per 64-wide row, a power of two 2^e: with amax = max |x| over the row's bf16 values = m 2^k, m in [1, 2),
 * e = max(k - 8 + (m > 1.75), -100), the smallest e with amax <= 448 2^e (amax = 0: e = -100). code = RNE_e4m3fn(x 2^-e)
 * and the value every kernel uses is code 2^e. Scaling is exact and |x 2^-e| <= 448, so no conversion saturates or gives
 * NaN and a row's codes and scale are a pure function of its 64 values. NaN / Inf inputs are outside the contract.
 * Layout per layer: kcache, vcache uint8 [B][H][Tcap][64]; kscale, vscale fp32 [B][H][Tcap].
 * Each entry below is its bf16 sibling with the codes in place of the bf16 tensors and the two scale pointers behind
 * them: the same indexing, the same checks with the same refusals (22 and a message, before any launch), and a NULL
 * scale pointer refused as well. A key of the call itself is quantised and dequantised in registers before use, by the
 * function that gpt2mi_kv_store_fp8 quantises with, so a key has the same bits whether it is read from the cache or
 * from the qkv row: gpt2mi_attn_extend_fp8 has the bits of one gpt2mi_attn_decode_fp8_ragged call per position, and a
 * row's bits depend on its own inputs and position only. Nothing at or above a row's position is read, nothing but the
 * row's own position is written, in the codes or in the scales; no atomics.
 * In a plan, kv_format selects the format for gpt2mi_decode_step*, gpt2mi_decode_extend and gpt2mi_decode_generate*:
 * any other value than the two below is refused with 22 and a message naming it, and so is kv_format = 1 with a NULL
 * layers[l].kscale / .vscale. ---- */
#define GPT2MI_KV_BF16 0
#define GPT2MI_KV_FP8 1
int gpt2mi_kv_store_fp8(const uint16_t* qkv, uint8_t* kcache, uint8_t* vcache, float* kscale, float* vscale, int B,
                        int T_src, int n, int t0, int H, int head_dim, int Tcap, void* stream);
int gpt2mi_attn_decode_fp8_ragged(const uint16_t* qkv, uint8_t* kcache, uint8_t* vcache, float* kscale, float* vscale,
                                  uint16_t* out, float* workspace, size_t workspace_floats, int B, int H, int head_dim,
                                  int Tcap, const int* pos, void* stream);
int gpt2mi_attn_extend_fp8(const uint16_t* qkv, uint8_t* kcache, uint8_t* vcache, float* kscale, float* vscale,
                           uint16_t* out, float* workspace, size_t workspace_floats, int R, int B, int H, int head_dim,
                           int Tcap, const int* seq, const int* pos, void* stream);

/* ---- v24: rows that share a prompt (csrc/decode.hip). Several continuations of one prompt sit in rows whose caches
 * hold identical bits over the prompt (generation.py DecodeSession.fork); the step then reads those keys and values once
 * per group of rows, not once per row.
 * The share map is two HOST arrays of B ints beside the position array, checked with it before any launch:
 * share_group[b] is the lowest row of b's group (b itself for a row alone) and share_len[b] the group's shared length (0
 * for a row alone). The caller guarantees that every member's cache holds the bits of row share_group[b]'s at positions
 * [0, share_len[b]), codes and scales with fp8. Both arrays NULL: no sharing, gpt2mi_attn_decode_ragged's launches.
 * A range of 32 keys is shared when it lies wholly below share_len. One wave loads a shared range from the lowest row's
 * stream once and computes, for each member of a chunk of the group in turn, that member's partial (max, sum, acc) with the
 * operations and the order gpt2mi_attn_decode_ragged uses, into the member's own workspace slot; every row computes its
 * ranges from share_len / 32 upward from its own stream as before, in the same launch; the combine is unchanged. out and
 * the caches therefore have the bits of gpt2mi_attn_decode_ragged on the same inputs, and positions below
 * 32 * (share_len / 32) of a member other than the lowest are not read. When no group has two members and a full shared
 * range, the launches are gpt2mi_attn_decode_ragged's; so are those of a plan entry (not of the two entries below)
 * while fewer than 16 rows are in such groups, where the shared form measured no faster: a launch choice, the same bits.
 * Refused with 22 and a message naming the entry and the index, before any launch, beside gpt2mi_attn_decode_ragged's
 * checks: exactly one of the two arrays NULL; share_group[b] outside [0, b]; share_group[share_group[b]] !=
 * share_group[b]; share_len[b] < 0; share_len[b] > pos[b]; share_len[b] != share_len[share_group[b]]; share_len[b] != 0
 * for a row alone in its group. The generate loops check the map against pos0. ---- */
int gpt2mi_attn_decode_shared(const uint16_t* qkv, uint16_t* kcache, uint16_t* vcache, uint16_t* out, float* workspace,
                              size_t workspace_floats, int B, int H, int head_dim, int Tcap, const int* pos,
                              const int* share_group, const int* share_len, void* stream);
int gpt2mi_attn_decode_shared_fp8(const uint16_t* qkv, uint8_t* kcache, uint8_t* vcache, float* kscale, float* vscale,
                                  uint16_t* out, float* workspace, size_t workspace_floats, int B, int H, int head_dim,
                                  int Tcap, const int* pos, const int* share_group, const int* share_len, void* stream);

/* ---- v24.1: per-token log-probabilities from the sampling kernel (csrc/sample_lp.hip, csrc/decode.hip). The executable
 * specification is gpt_2_distributed_amd/generation.py token_logprobs.
 * Per row of fp32 logits l[0 .. V): M = max l, S = sum exp(l_i - M), lse = M + log(S), logprob(i) = l_i - lse: the RAW
 * model distribution, before penalties, the temperature division and top-k / top-p (the OpenAI convention, vLLM's
 * default). lse is a function of the row's bits and V only (not of the sampler's values, the seed, the position, B or the
 * kernel form): S is summed in a fixed order (per thread over its 50 registers, an xor butterfly, the 16 waves in order),
 * no atomics, so two calls give the same bits. The top_n alternatives are the top_n largest l_i in descending order,
 * equal values by ascending index (-0 and +0 are equal; -inf entries come last, by index); the order compares fp32
 * values and is exact. NaN logits are outside the contract.
 * The kernels are instantiations of the sampling kernel of their own (the others are compiled as before): lse and the
 * alternatives are formed from the registers right after the load, the drawn token's raw logit is one load from the
 * logits buffer at the end. A row whose done flag was set on entry gets eos and logprob 0; its alternatives are written
 * like any row's. ---- */
#define GPT2MI_LOGPROBS_MAX_TOP 20
typedef struct gpt2mi_logprobs {
  float* logprob;     /* device fp32 [B][ld]: row b's value goes to logprob[b*ld + col[b]] */
  int ld;
  int top_n;          /* 0 .. GPT2MI_LOGPROBS_MAX_TOP and <= V; 0: the two arrays below are not read */
  int32_t* top_id;    /* device [B][ld][top_n] */
  float* top_logprob; /* device [B][ld][top_n] */
  const int* col;     /* HOST [B], may be NULL: col[b] = pos[b] */
} gpt2mi_logprobs;
/* gpt2mi_sample_penalized with the log-probabilities of what it draws. lp == NULL is gpt2mi_sample_penalized exactly
 * (launches, bits, refusals); otherwise tok_out, seq_out, done, probs_out and logits_out have the bits of that call.
 * col travels to the kernel by value. Refused with 22 and a message, before any launch, beside the forwarded checks:
 * top_n outside [0, GPT2MI_LOGPROBS_MAX_TOP] or > V, a NULL logprob, top_n > 0 with a NULL top array, col[b] (pos[b]
 * without col) outside [0, ld). */
int gpt2mi_sample_logprobs(const float* logits, int ldl, int B, int V, float temperature, int top_k, float top_p,
                           uint64_t seed, const int* pos, const uint32_t* row_id, int64_t eos, uint8_t* done,
                           int64_t* tok_out, int64_t* seq_out, int ld_seq, float* probs_out,
                           const gpt2mi_penalties* pen, float* logits_out, const gpt2mi_logprobs* lp, void* stream);
/* gpt2mi_decode_generate_penalized likewise (lp == NULL: that entry exactly). Step i writes column pos0[b] + i of row b,
 * as it does in seq, so lp->col must be NULL; refused as well: max pos0 + n > lp->ld. */
int gpt2mi_decode_generate_logprobs(const gpt2mi_decode_plan* plan, int V, float temperature, int top_k, float top_p,
                                    uint64_t seed, int64_t eos, const int* pos0, const uint32_t* row_id, int n,
                                    int64_t* tok, int64_t* seq, int ld_seq, uint8_t* done, void* stream,
                                    float repetition, float presence, float frequency, const int* gen_start,
                                    const gpt2mi_logprobs* lp);

/* ---- v24.2: beam search on the device (csrc/beam.hip). The executable specification of the selection rule is
 * gpt_2_distributed_amd/generation.py beam_select.
 * The W beams of a prompt are W adjacent rows, group g in rows g W .. g W + W - 1, forks of one prefill: their caches
 * hold identical bits over the prompt, so re-parenting the beams moves only the generated suffix of the cache rows.
 * State per row: cum, the fp32 cumulative log-probability, and done. A live beam j offers its W most likely tokens in
 * gpt2mi_sample_logprobs' order (value descending, equal values by ascending index), rank r at score
 * cum[j] + top_logprob[j][r], one IEEE fp32 add; a finished beam offers token eos at score cum[j], rank 0. Candidates are
 * ordered by (score descending, beam ascending, rank ascending), comparing fp32 values (-0 == +0; equal -inf scores tie
 * like any others); NaN is outside the contract. The W first become the new beams, best first, in the group's rows. ---- */
/* One launch, one workgroup per group: top_id (int32) / top_logprob device [G W][W]; cum fp32 / done uint8 device [G W].
 * For new beam row s: tok_out[s] (int64) its token, parent_out[s] (int32) the absolute row it continues, cum_out[s] its
 * score, done_out[s] = its parent's done or tok == eos. eos = -1: no eos; the done flags are then not read and done_out
 * is 0. Each candidate counts the candidates ahead of it and the one with count c < W writes slot c: no float atomics, no
 * order that depends on scheduling. cum_out / done_out may be cum / done or other buffers (a group's inputs are read
 * before anything is written). Nothing but rows [0, G W) of the four outputs is written.
 * Refused with 22 and a message before any launch: W outside [1, GPT2MI_LOGPROBS_MAX_TOP], G W outside
 * [1, GPT2MI_DECODE_MAX_B], eos < -1, a NULL pointer. */
int gpt2mi_beam_select(const int32_t* top_id, const float* top_logprob, const float* cum, const uint8_t* done, int G,
                       int W, int64_t eos, int64_t* tok_out, int32_t* parent_out, float* cum_out, uint8_t* done_out,
                       void* stream);
/* For every row r < G W with parent[r] != r, positions [lo[r], hi[r]) of row r become those of row parent[r]: in kcache
 * and vcache (kv_format 0: bf16 [L][B][H][Tcap][64]; 1: uint8 codes, and kscale / vscale fp32 [L][B][H][Tcap], NULL
 * otherwise), layer l at l * layer_rows rows of 64 behind layer 0 (layer_rows >= B H Tcap; not read for L = 1), and in
 * seq, int64 [>= G W][ld_seq] (may be NULL), over the same columns. parent is a DEVICE int32 [G W] array (the select's
 * output): the kernels treat a value outside row r's group [g W, g W + W) as "no move" before they form any address from
 * it. lo and hi are HOST arrays, checked here and passed by value; the rows of a group must have one window. Two
 * launches: the windows of the moved rows are gathered into the workspace, then written back, so no launch reads a
 * position another workgroup of it writes, whatever cycles the permutation has. Nothing outside the windows of moved
 * rows is written: not position hi, not rows >= G W, not the positions below lo. Every window empty: no launch.
 * workspace: gpt2mi_beam_reorder_workspace(kv_format, L, H, G W, max_r hi[r] - lo[r]) bytes, 16-byte aligned.
 * Refused with 22 and a message before any launch: W or G W as above, a kv_format other than 0 / 1, L, H or Tcap < 1,
 * B < G W, 2 L H + 1 > 65535, layer_rows < B H Tcap with L > 1, a window outside 0 <= lo <= hi <= Tcap (hi > ld_seq with
 * seq) or differing within a group, a workspace too small or misaligned, a NULL cache, scale (fp8), parent, lo or hi. */
size_t gpt2mi_beam_reorder_workspace(int kv_format, int L, int H, int R, int window); /* bytes; 0 for invalid arguments */
int gpt2mi_beam_reorder(void* kcache, void* vcache, float* kscale, float* vscale, int kv_format, int L,
                        size_t layer_rows, int B, int H, int Tcap, int64_t* seq, int ld_seq, const int32_t* parent, int G,
                        int W, const int* lo, const int* hi, void* workspace, size_t workspace_bytes, void* stream);
/* The token loop, on the stream with nothing synchronised or read back: plan->B = G W rows, row b at pos0[b] >= 1 with
 * its logits in plan->logits, its prompt ending at lo[b] in [1, pos0[b]] (HOST arrays; one value per group each). For
 * i < n: the per-row top W of plan->logits (gpt2mi_sample_logprobs' alternatives at top_n = W, bit for bit: the same
 * function on the same registers); gpt2mi_beam_select into tok, cum and done in place, the tokens also to column
 * pos0[b] + i of seq; gpt2mi_beam_reorder with the windows [lo[b], pos0[b] + i); if i + 1 < n, gpt2mi_decode_step_ragged at
 * pos0[b] + i. Finished rows keep being stepped with eos. The plan's share map stays valid throughout: positions below
 * lo are never written. cum (fp32) / done (uint8) device [B] hold the state on entry ({0, -inf, ...} per group and 0 at
 * the first step) and on return; parents (device int32 [n][B], may be NULL) receives each step's parent rows.
 * workspace: GPT2MI_BEAM_LOOP_BYTES + gpt2mi_beam_reorder_workspace(plan->kv_format, L, H, B, max_b pos0[b] + n - 1 - lo[b])
 * bytes, 16-byte aligned. The layers' caches must be equally spaced (one tensor per kind, as the package allocates them).
 * Refused with 22 and a message before any launch: what gpt2mi_decode_step_ragged refuses at pos0, B not a multiple of
 * W, W or B as above, W > V, V outside [1, Vp] or above GPT2MI_SAMPLE_MAX_V, eos outside [-1, V), n < 0, pos0[b] or lo[b]
 * out of range or differing within a group, max pos0 + n > Tcap or > ld_seq, unequally spaced layer caches, a workspace
 * too small or misaligned, a NULL pointer. */
#define GPT2MI_BEAM_LOOP_BYTES (GPT2MI_DECODE_MAX_B * (8 * GPT2MI_LOGPROBS_MAX_TOP + 4))
int gpt2mi_decode_beam_search(const gpt2mi_decode_plan* plan, int V, int W, int64_t eos, const int* pos0, const int* lo,
                              int n, int64_t* tok, int64_t* seq, int ld_seq, float* cum, uint8_t* done, int32_t* parents,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- v24.4: logit bias, min-p, a minimum number of new tokens and stop sequences in the sampler (csrc/sample_con.hip,
 * csrc/decode.hip). The executable specification is gpt_2_distributed_amd/generation.py apply_constraints,
 * sample_reference(min_p=) and stop_match. On a row drawn at pos whose generated part starts at gen_start (pen's, 0
 * without), in this order, every arithmetic step one IEEE fp32 operation rounded to nearest:
 *   1 the raw row: the log-probabilities of v24.1 keep coming from it;
 *   2 the penalties of v22;
 *   3 bias: x_i = x_i + bias[bias_row[b]][i] where the row has a bias row (-inf bans a token; +inf and NaN are outside
 *     the contract);
 *   4 min_new > 0 and pos - gen_start < min_new: x_eos = -inf;
 *   5 logits_out receives the row as it stands; then the temperature division, top-k and top-p as ever;
 *   6 min_p > 0, sampled form only: with lmp = fp32(log(double(min_p))) and mx the row maximum after the division, token
 *     i is kept iff x_i >= fl32(mx + lmp), intersected with what top-k and top-p kept;
 *   7 the draw;
 *   8 stop sequences: a row that was not done and drew t != eos gets its done flag set when for some sequence s of length
 *     n the tokens hist[pos - n + 1 .. pos - 1] followed by t equal s, with pos - n + 1 >= gen_start (the match lies in
 *     the generated part) and pos - gen_start + 1 >= min_new. From then on the row emits eos, as a row that drew eos.
 * A row with no finite value left gives token 0 in both kernel forms.
 * The kernels are instantiations of the sampling kernel of their own (the others are compiled as before): the bias is a
 * streaming add of one coalesced load per element, the stop table travels by value and thread 0 compares at most 15
 * history entries per sequence with it; no float atomics, two calls give the same bits. ---- */
#define GPT2MI_STOP_MAX_SEQS 8
#define GPT2MI_STOP_MAX_LEN 16
typedef struct gpt2mi_constraints {
  const float* bias;   /* device fp32 [bias_rows][ld_bias]; NULL: none */
  int ld_bias, bias_rows;
  const int* bias_row; /* HOST [B]; -1: the row has no bias; NULL: row b reads bias row b */
  float min_p;         /* 0: off; (0, 1] */
  int min_new;         /* 0: off */
  int n_stop;          /* 0 .. GPT2MI_STOP_MAX_SEQS */
  const int32_t* stop; /* HOST [n_stop][GPT2MI_STOP_MAX_LEN] */
  const int* stop_len; /* HOST [n_stop], each 1 .. GPT2MI_STOP_MAX_LEN */
} gpt2mi_constraints;
/* gpt2mi_sample_logprobs under the rule above. pen supplies hist / hist_row / gen_start (its values neutral if unused;
 * NULL: no history, gen_start 0); lp may be NULL. con == NULL, or one with nothing on (no row with a bias row, min_p 0,
 * min_new 0, n_stop 0), is gpt2mi_sample_logprobs exactly, on the same kernels. Refused with 22 and a message naming the
 * entry and the index, before any launch, beside the forwarded checks: min_p outside [0, 1] or NaN; min_new < 0, or
 * min_new > 0 with eos < 0; n_stop outside [0, GPT2MI_STOP_MAX_SEQS]; a stop_len outside [1, GPT2MI_STOP_MAX_LEN]; a stop
 * token outside [0, V); n_stop > 0 with eos < 0, a NULL done, a NULL hist (or stop / stop_len), ld_hist < pos[b] or
 * hist_row[b] outside [0, hist_rows); a bias with ld_bias < V or bias_rows < 1; bias_row[b] outside [-1, bias_rows); a
 * NULL bias_row with bias_rows < B; gen_start[b] outside [0, pos[b]]. */
int gpt2mi_sample_constrained(const float* logits, int ldl, int B, int V, float temperature, int top_k, float top_p,
                              uint64_t seed, const int* pos, const uint32_t* row_id, int64_t eos, uint8_t* done,
                              int64_t* tok_out, int64_t* seq_out, int ld_seq, float* probs_out,
                              const gpt2mi_penalties* pen, float* logits_out, const gpt2mi_logprobs* lp,
                              const gpt2mi_constraints* con, void* stream);
/* gpt2mi_decode_generate_logprobs likewise (con == NULL or neutral: that entry exactly): seq is the history, hist_row
 * the identity, and with n_stop > 0 a NULL seq is refused. */
int gpt2mi_decode_generate_constrained(const gpt2mi_decode_plan* plan, int V, float temperature, int top_k, float top_p,
                                       uint64_t seed, int64_t eos, const int* pos0, const uint32_t* row_id, int n,
                                       int64_t* tok, int64_t* seq, int ld_seq, uint8_t* done, void* stream,
                                       float repetition, float presence, float frequency, const int* gen_start,
                                       const gpt2mi_logprobs* lp, const gpt2mi_constraints* con);

/* ---- v24.5: document masking for packed sequences (csrc/packing.hip, csrc/attention.hip, csrc/fp32.hip). The
 * executable specification is gpt_2_distributed_amd/packing.py: doc_bounds_reference and doc_attention_reference.
 * A row of T tokens is partitioned into documents, contiguous intervals [s, e); doc_start / doc_end are int32 [B, T]
 * with 0 <= doc_start[b,t] <= t < doc_end[b,t] <= T, both constant over [doc_start[b,t], doc_end[b,t]). Query t attends
 * key k iff doc_start[b,t] <= k <= t, which for k <= t is t < doc_end[b,k]; the softmax, its statistics and the dropout
 * decision of a pair are those of the unmasked entries. No row is fully masked (key t is visible to query t). ---- */
/* The bounds of idx int64 [B, T] from its separator tokens. eot_begin = 0: eot is the last token of the document it
 * closes (a document begins at p when idx[p - 1] == eot); 1: eot opens a document (one begins at p when idx[p] == eot).
 * Only positions < T_valid count: start[t] = the last beginning <= t, or 0; end[t] = the first beginning > t, or
 * T_valid; positions >= T_valid (the engine's padding to the attention tile) form one document [T_valid, T). One
 * workgroup per row, any T; no atomics, no host synchronisation. Refused with 22: a NULL pointer, B or T < 1, T_valid
 * outside [1, T], eot_begin outside {0, 1}. */
int gpt2mi_doc_bounds(const int64_t* idx, int B, int T, int T_valid, int64_t eot, int eot_begin, int* start, int* end,
                      void* stream);
/* gpt2mi_attn_fwd / gpt2mi_attn_bwd under the mask: the same contracts (T % 64 == 0, head_dim 64, the same dqkv_colsum
 * partials) and, with one document per row, the same bits. Key tiles (forward, dQ) before the document of a workgroup's
 * first query and query tiles (dK/dV) after the document of its last key are not visited, and a wave skips the tiles
 * that lie wholly in other documents. Bounds outside the contract are clamped where they are read (start into [0, t],
 * end into [t + 1, T]): they may give wrong numbers, never an access out of range. NULL bounds are refused with 22
 * before any launch. */
int gpt2mi_attn_fwd_doc(const uint16_t* qkv, uint16_t* out, float* lse, const int* doc_start, int B, int T, int H,
                        int head_dim, float p_drop, uint64_t seed, void* stream);
int gpt2mi_attn_bwd_doc(const uint16_t* qkv, const uint16_t* out, const uint16_t* dout, const float* lse, float* delta,
                        uint16_t* dqkv, float* dqkv_colsum, const int* doc_start, const int* doc_end, int B, int T,
                        int H, int head_dim, float p_drop, uint64_t seed, void* stream);
/* The fp32 family likewise (dqkv_colsum must be NULL, as in gpt2mi_attn_bwd_f32). */
int gpt2mi_attn_fwd_f32_doc(const float* qkv, float* out, float* lse, const int* doc_start, int B, int T, int H,
                            int head_dim, float p_drop, uint64_t seed, void* stream);
int gpt2mi_attn_bwd_f32_doc(const float* qkv, const float* out, const float* dout, const float* lse, float* delta,
                            float* dqkv, float* dqkv_colsum, const int* doc_start, const int* doc_end, int B, int T,
                            int H, int head_dim, float p_drop, uint64_t seed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GPT2MI_H */
