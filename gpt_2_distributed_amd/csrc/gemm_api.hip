// C ABI of the bf16 GEMMs (gpt2mi.h): every entry point validates its arguments, asks gemm_plan.h which kernel the call
// gets, fills the kernels' parameter block once and launches what the plan says (gemm_pp.hip, gemm256.hip, gemm.hip,
// splitk_reduce.hip).
//
//   C[m,n] (op)= epilogue( alpha * sum_k A(m,k) * B(n,k) )
#include <mutex>

#include "common.h"
#include "gemm_params.h"
#include "gpt2mi.h"

using gpt2mi::GemmFamily;
using gpt2mi::GemmPlan;
using gpt2mi::Reduce;
using gpt2mi::SlabType;

namespace {

int launch(const GemmPlan& plan, const GemmParams& P, hipStream_t s) {
  switch (plan.family) {
    case GemmFamily::PingPong:
    case GemmFamily::PingPongPersistent: return gpt2mi::gemm_pp_launch(plan, P, s);
    case GemmFamily::TwoStage256: return gpt2mi::gemm256_launch(plan, P, s);
    case GemmFamily::Tile128: return gpt2mi::gemm128_launch(plan, P, s);
    default: gpt2mi::set_error("gemm: no kernel for these arguments"); return 22;
  }
}

// the operands, shape and scale of one problem with a dense C[M][N] over the plan's K ranges (the caller sets C and
// whatever else its epilogue reads)
GemmParams gemm_params(const GemmPlan& plan, int M, int N, int K, const uint16_t* A, int lda, const uint16_t* B,
                        int ldb, float alpha, const float* alpha_dev) {
  GemmParams P{};
  P.A = (const bf16*)A;
  P.B = (const bf16*)B;
  P.M = M; P.N = N; P.K = K; P.lda = lda; P.ldb = ldb; P.ldc = N;
  P.k_per_split = plan.k_per_split;
  P.alpha = alpha;
  P.alpha_dev = alpha_dev;
  return P;
}

}  // namespace

// layout: 0 = forward (A[M][K], B[N][K]); 1 = dgrad (A[M][K], B[K][N]); 2 = wgrad (A[K][M], B[K][N]).
GPT2MI_EXPORT int gpt2mi_gemm(int layout, int epilogue, int M, int N, int K, const uint16_t* A, int lda,
                              const uint16_t* B, int ldb, void* C, int ldc, const float* bias, const float* resid,
                              uint16_t* aux, int ldaux, float alpha, const float* alpha_dev, int accumulate,
                              int splits, float p_drop, uint64_t seed, float* dbias, int sched, void* stream) {
  GPT2MI_REQUIRE(dbias == nullptr || ((epilogue == EPI_BF16 || epilogue == EPI_GELU_BWD) && layout <= 1),
                 "gemm: dbias (fused column sum) needs the BF16 or GELU_BWD epilogue of layout 0/1");
  // (64-multiples: C = 1600, GPT-2 1.5B, gives N = 1600 / 4800, a partial last tile of every kernel)
  GPT2MI_REQUIRE(N % 64 == 0 && N > 0 && M % 64 == 0 && M > 0, "gemm: N=%d and M=%d must be multiples of 64", N, M);
  GPT2MI_REQUIRE(splits >= 1 && K % (64 * splits) == 0, "gemm: K=%d must be a multiple of %d*splits(%d)", K, 64,
                 splits);
  GPT2MI_REQUIRE(splits == 1 || epilogue == EPI_ATOMIC, "gemm: split-K needs the atomic epilogue");
  GPT2MI_REQUIRE(layout >= 0 && layout <= 2, "gemm: bad layout %d", layout);
  GPT2MI_REQUIRE(gpt2mi::sched_ok(sched, gpt2mi::kSchedFlags), "gemm: bad sched %#x", sched);
  GPT2MI_REQUIRE(ldc % 4 == 0 && (ldaux % 4 == 0 || aux == nullptr), "gemm: ldc/ldaux must be multiples of 4");
  GPT2MI_REQUIRE(p_drop <= 0.f || (size_t)M * N < (1ull << 33),
                 "gemm: M*N=%zu exceeds the 32-bit dropout pair index", (size_t)M * N);
  const GemmPlan plan =
      gpt2mi::plan_gemm(layout, epilogue, M, N, K, lda, ldb, splits, dbias != nullptr, sched, gpt2mi::num_cus());
  GPT2MI_REQUIRE(plan.family != GemmFamily::Refused, "gemm: unsupported layout %d / epilogue %d combination", layout,
                 epilogue);
  GemmParams P = gemm_params(plan, M, N, K, A, lda, B, ldb, alpha, alpha_dev);
  P.C = C;
  P.ldc = ldc;
  P.bias = bias;
  P.resid = resid;
  P.aux = aux;
  P.ldaux = ldaux;
  P.dbias = plan.colsum ? nullptr : dbias;  // (the ping-pong kernel fuses the column sums)
  P.accumulate = accumulate;
  P.seed = seed;
  P.thr = drop_threshold(p_drop);
  P.inv_keep = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
  const int rc = launch(plan, P, (hipStream_t)stream);
  if (rc || !plan.colsum) return rc;
  return gpt2mi_colsum_bf16((const uint16_t*)C, dbias, M, N, ldc, stream);  // of the output just stored
}

// Weight gradient C[M][N] (+)= alpha * A^T B with A stored [K][M], B stored [K][N] (dW = dY^T X over
// K = tokens), on the 256x256 kernels: `splits` K ranges write partial slabs into `workspace`
// (splits*M*N floats), then one pass sums them in fixed order into C (deterministic; no atomics).
GPT2MI_EXPORT int gpt2mi_gemm_wgrad(int M, int N, int K, const uint16_t* A, int lda, const uint16_t* B, int ldb,
                                    float* C, int ldc, int accumulate, float alpha, const float* alpha_dev,
                                    float* workspace, size_t workspace_floats, int splits, int sched,
                                    void* stream) {
  GPT2MI_REQUIRE(M % 64 == 0 && N % 64 == 0 && K % 64 == 0 && M > 0 && N > 0 && K > 0,
                 "gemm_wgrad: M=%d N=%d K=%d must be multiples of 64", M, N, K);
  GPT2MI_REQUIRE(ldc == N, "gemm_wgrad: C must be dense (ldc == N)");
  GPT2MI_REQUIRE(splits >= 1 && splits <= K / 64, "gemm_wgrad: bad splits %d", splits);
  GPT2MI_REQUIRE(gpt2mi::sched_ok(sched, gpt2mi::kSchedFlags | GPT2MI_SCHED_BF16_SLABS), "gemm_wgrad: bad sched %#x",
                 sched);
  const GemmPlan plan = gpt2mi::plan_wgrad(M, N, K, lda, ldb, splits, sched, gpt2mi::num_cus());
  hipStream_t s = (hipStream_t)stream;
  GemmParams P = gemm_params(plan, M, N, K, A, lda, B, ldb, alpha, alpha_dev);
  if (plan.reduce == Reduce::None) {  // one K range: the kernel accumulates into / writes C itself
    P.C = C;
    P.accumulate = accumulate;
    return launch(plan, P, s);
  }
  GPT2MI_REQUIRE(workspace != nullptr && workspace_floats >= (size_t)plan.splits * M * N,
                 "gemm_wgrad: workspace of %zu floats < splits*M*N = %zu", workspace_floats,
                 (size_t)plan.splits * M * N);
  P.C = workspace;
  const int rc = launch(plan, P, s);
  if (rc) return rc;
  if (plan.slab == SlabType::BF16)
    return gpt2mi::splitk_reduce16((const bf16*)workspace, plan.splits, (size_t)M * N, C, accumulate, s);
  return gpt2mi::splitk_reduce(workspace, plan.splits, (size_t)M * N, C, accumulate, s);
}

// Up to four weight gradients over the same K tokens as ONE split-K launch plus one reduction launch (a GPT2Block's qkv /
// proj / fc1 / fc2 weight gradients, issued together at the end of the block's backward): C_g[M_g][N_g] (+)= alpha *
// A_g^T B_g for g < count, every M_g and N_g a multiple of 256. Each problem's `splits` slabs are summed in split
// order, so each C_g holds the same bits as gpt2mi_gemm_wgrad(M_g, N_g, K, ..., splits) with fp32 slabs.
GPT2MI_EXPORT int gpt2mi_gemm_wgrad_grouped(int count, const int* M, const int* N, int K, const uint16_t* const* A,
                                            const int* lda, const uint16_t* const* B, const int* ldb, float* const* C,
                                            int accumulate, float alpha, const float* alpha_dev, float* workspace,
                                            size_t workspace_floats, int splits, int sched, void* stream) {
  GPT2MI_REQUIRE(count >= 1 && count <= kGroupMax, "gemm_wgrad_grouped: count=%d (1..%d)", count, kGroupMax);
  GPT2MI_REQUIRE(K % 128 == 0 && K > 0, "gemm_wgrad_grouped: K=%d must be a multiple of 128", K);
  GPT2MI_REQUIRE(splits >= 1 && splits <= K / 128, "gemm_wgrad_grouped: bad splits %d", splits);
  GPT2MI_REQUIRE((sched & ~(GPT2MI_SCHED_NO_PERSISTENT | GPT2MI_SCHED_SHARED_CUS)) == 0,
                 "gemm_wgrad_grouped: bad sched %#x (fp32 slabs on the ping-pong kernel only)", sched);
  for (int g = 0; g < count; ++g)
    GPT2MI_REQUIRE(M[g] > 0 && N[g] > 0 && M[g] % 256 == 0 && N[g] % 256 == 0,
                   "gemm_wgrad_grouped: problem %d is %d x %d (multiples of 256 only)", g, M[g], N[g]);
  const GemmPlan plan = gpt2mi::plan_wgrad_grouped(count, M, N, K, splits, sched);
  GemmGroup G{};
  G.count = count;
  size_t off = 0;
  const float* slab[kGroupMax];
  float* out[kGroupMax];
  size_t n[kGroupMax];
  for (int g = 0; g < count; ++g) {
    G.p[g] = gemm_params(plan, M[g], N[g], K, A[g], lda[g], B[g], ldb[g], alpha, alpha_dev);
    G.p[g].C = workspace + off;
    slab[g] = workspace + off;
    out[g] = C[g];
    n[g] = (size_t)M[g] * N[g];
    off += (size_t)plan.splits * n[g];
    G.prefix[g + 1] = G.prefix[g] + (M[g] / 256) * (N[g] / 256);
  }
  G.tiles = G.prefix[count];
  GPT2MI_REQUIRE(workspace != nullptr && workspace_floats >= off,
                 "gemm_wgrad_grouped: workspace of %zu floats < %zu (splits x the problems' outputs)", workspace_floats, off);
  hipStream_t s = (hipStream_t)stream;
  const int rc = gpt2mi::gemm_pp_launch_grouped(plan, G, s);
  if (rc) return rc;
  return gpt2mi::splitk_reduce_grouped(slab, out, n, count, plan.splits, accumulate, s);
}

namespace {

// Pinned staging for the problem tables of gpt2mi_gemm_wgrad_batch: kStageSlots slots per device in rotation, each
// with the event of its last upload. A slot is rewritten only after that copy has run, a wait only a caller more than
// kStageSlots batched launches ahead of the GPU ever meets: the upload is an asynchronous copy from pinned memory on the
// caller's stream, ordered before the launch, and the host waits for nothing the stream has not finished long ago.
constexpr int kStageSlots = 8, kStageDevices = 16;
struct TableStage {
  std::mutex mu;
  char* host = nullptr;  // kStageSlots x kStageBytes
  hipEvent_t done[kStageSlots] = {};
  bool pending[kStageSlots] = {};
  unsigned next = 0;
};
constexpr size_t kStageBytes = (gemm_batch_table_bytes(kBatchMax) + 255) / 256 * 256;
static_assert(sizeof(GemmParams) % alignof(GemmParams) == 0 && alignof(GemmParams) >= alignof(int), "table layout");
TableStage g_stage[kStageDevices];

// table (device) <- the `bytes` that fill(host slot) writes, on stream s
template <typename Fill>
int upload_table(void* table, size_t bytes, hipStream_t s, Fill fill) {
  int dev = 0;
  GPT2MI_REQUIRE(hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kStageDevices,
                 "gemm_wgrad_batch: no current device below %d", kStageDevices);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) != hipSuccess) {  // (a stream the query does not take is not a capturing one)
    (void)hipGetLastError();
    cap = hipStreamCaptureStatusNone;
  }
  GPT2MI_REQUIRE(cap == hipStreamCaptureStatusNone,
                 "gemm_wgrad_batch: the stream is capturing (the table upload waits on events: not capturable)");
  TableStage& st = g_stage[dev];
  std::lock_guard<std::mutex> lock(st.mu);
  if (!st.host) {  // (host is set last: a failed first call is tried again from the event it stopped at)
    for (int i = 0; i < kStageSlots; ++i)
      GPT2MI_REQUIRE(st.done[i] != nullptr || hipEventCreateWithFlags(&st.done[i], hipEventDisableTiming) == hipSuccess,
                     "gemm_wgrad_batch: hipEventCreate failed");
    void* h = nullptr;
    GPT2MI_REQUIRE(hipHostMalloc(&h, kStageSlots * kStageBytes, hipHostMallocDefault) == hipSuccess && h != nullptr,
                   "gemm_wgrad_batch: no pinned staging memory");
    st.host = (char*)h;
  }
  const unsigned slot = st.next++ % kStageSlots;
  if (st.pending[slot])
    GPT2MI_REQUIRE(hipEventSynchronize(st.done[slot]) == hipSuccess, "gemm_wgrad_batch: staging slot wait failed");
  char* h = st.host + slot * kStageBytes;
  fill(h);
  GPT2MI_REQUIRE(hipMemcpyAsync(table, h, bytes, hipMemcpyHostToDevice, s) == hipSuccess,
                 "gemm_wgrad_batch: table upload failed");
  GPT2MI_REQUIRE(hipEventRecord(st.done[slot], s) == hipSuccess, "gemm_wgrad_batch: hipEventRecord failed");
  st.pending[slot] = true;
  return 0;
}

}  // namespace

GPT2MI_EXPORT int gpt2mi_gemm_wgrad_batch_max(void) { return kBatchMax; }
GPT2MI_EXPORT size_t gpt2mi_gemm_wgrad_batch_scratch(int count) {
  return count >= 1 && count <= kBatchMax ? gemm_batch_table_bytes(count) : 0;
}

// `count` full-tile weight gradients over the same K tokens as ONE launch without split-K: every block owns one 256x256
// output tile of one problem, accumulates it in registers over all K tokens and writes (or accumulates into) C once. No
// slabs, no reduction launch: what a step with many same-K weight gradients (every GPT2Block's four, deferred to the end
// of the trunk backward) needs to fill whole rounds of CUs without splitting tiles. Each C_g holds the bits
// gpt2mi_gemm_wgrad(M_g, N_g, K, ..., splits = 1) gives it.
GPT2MI_EXPORT int gpt2mi_gemm_wgrad_batch(int count, const int* M, const int* N, int K, const uint16_t* const* A,
                                          const int* lda, const uint16_t* const* B, const int* ldb, float* const* C,
                                          const int* ldc, int accumulate, float alpha, const float* alpha_dev,
                                          void* table, size_t table_bytes, int sched, void* stream) {
  GPT2MI_REQUIRE(count >= 1 && count <= kBatchMax, "gemm_wgrad_batch: count=%d (1..%d)", count, kBatchMax);
  GPT2MI_REQUIRE(K % 128 == 0 && K > 0, "gemm_wgrad_batch: K=%d must be a multiple of 128", K);
  GPT2MI_REQUIRE((sched & ~(GPT2MI_SCHED_NO_PERSISTENT | GPT2MI_SCHED_SHARED_CUS)) == 0,
                 "gemm_wgrad_batch: bad sched %#x", sched);
  long long tiles = 0;
  for (int g = 0; g < count; ++g) {
    GPT2MI_REQUIRE(M[g] > 0 && N[g] > 0 && M[g] % 256 == 0 && N[g] % 256 == 0,
                   "gemm_wgrad_batch: problem %d is %d x %d (multiples of 256 only)", g, M[g], N[g]);
    GPT2MI_REQUIRE(A[g] && B[g] && C[g] && lda[g] >= M[g] && ldb[g] >= N[g] && ldc[g] >= N[g] && ldc[g] % 4 == 0 &&
                       lda[g] % 8 == 0 && ldb[g] % 8 == 0,
                   "gemm_wgrad_batch: problem %d: null operand or bad lda=%d ldb=%d ldc=%d", g, lda[g], ldb[g], ldc[g]);
    tiles += (long long)(M[g] / 256) * (N[g] / 256);
  }
  GPT2MI_REQUIRE(tiles < (1ll << 30), "gemm_wgrad_batch: %lld tiles", tiles);
  const size_t bytes = gemm_batch_table_bytes(count);
  GPT2MI_REQUIRE(table != nullptr && table_bytes >= bytes && (uintptr_t)table % 16 == 0,
                 "gemm_wgrad_batch: table scratch of %zu bytes < %zu (gpt2mi_gemm_wgrad_batch_scratch), or not 16-B aligned",
                 table_bytes, bytes);
  const GemmPlan plan = gpt2mi::plan_wgrad_batch(count, M, N, K, sched);
  GPT2MI_REQUIRE(plan.family != GemmFamily::Refused, "gemm_wgrad_batch: refused by the planner");
  hipStream_t s = (hipStream_t)stream;
  GemmBatch G{};
  G.p = (const GemmParams*)table;
  G.prefix = (const int*)((const char*)table + (size_t)count * sizeof(GemmParams));
  G.count = count;
  G.tiles = plan.grid;
  const int rc = upload_table(table, bytes, s, [&](char* h) {
    GemmParams* p = (GemmParams*)h;
    int* prefix = (int*)(h + (size_t)count * sizeof(GemmParams));
    prefix[0] = 0;
    for (int g = 0; g < count; ++g) {
      p[g] = gemm_params(plan, M[g], N[g], K, A[g], lda[g], B[g], ldb[g], alpha, alpha_dev);
      p[g].C = C[g];
      p[g].ldc = ldc[g];
      p[g].accumulate = accumulate;
      prefix[g + 1] = prefix[g] + (M[g] / 256) * (N[g] / 256);
    }
  });
  if (rc) return rc;
  return gpt2mi::gemm_pp_launch_batch(plan, G, s);
}

// The same weight gradient with the second operand given TRANSPOSED, k-contiguous: Bt stored [N][K] (X^T, e.g. the
// final LayerNorm's output transposed once per step). Runs the ping-pong kernel in layout 1 on C^T[N][M] = Bt . A
// (k-contiguous A operand, m-contiguous B operand: one transposed fragment stream instead of two; the lm_head wgrad
// split 1.75 -> 1.42 ms, tools/lmwg_ab.py) into split-K slabs, then sums them transposed into C[M][N].
GPT2MI_EXPORT int gpt2mi_gemm_wgrad_kt(int M, int N, int K, const uint16_t* A, int lda, const uint16_t* Bt, int ldbt,
                                       float* C, int ldc, int accumulate, float alpha, const float* alpha_dev,
                                       float* workspace, size_t workspace_floats, int splits, int sched,
                                       void* stream) {
  GPT2MI_REQUIRE(M % 64 == 0 && N % 64 == 0 && K % 128 == 0 && M > 0 && N > 0 && K > 0,
                 "gemm_wgrad_kt: M=%d N=%d must be multiples of 64, K=%d of 128", M, N, K);
  GPT2MI_REQUIRE(M % 256 == 0, "gemm_wgrad_kt: M=%d must be a multiple of 256 (the transposed operand's full tiles)", M);
  GPT2MI_REQUIRE(ldc == N, "gemm_wgrad_kt: C must be dense (ldc == N)");
  GPT2MI_REQUIRE(splits >= 1 && splits <= K / 128, "gemm_wgrad_kt: bad splits %d", splits);
  GPT2MI_REQUIRE((sched & ~(GPT2MI_SCHED_NO_PERSISTENT | GPT2MI_SCHED_SHARED_CUS | GPT2MI_SCHED_BF16_SLABS | 0xff)) == 0,
                 "gemm_wgrad_kt: bad sched %#x", sched);
  GPT2MI_REQUIRE(workspace != nullptr, "gemm_wgrad_kt: needs a workspace (splits*M*N floats)");
  const GemmPlan plan = gpt2mi::plan_wgrad_kt(M, N, K, splits, sched);
  GPT2MI_REQUIRE(workspace_floats >= (size_t)plan.splits * M * N, "gemm_wgrad_kt: workspace of %zu floats < %zu",
                 workspace_floats, (size_t)plan.splits * M * N);
  hipStream_t s = (hipStream_t)stream;
  // C^T[N][M] = Bt[N][K] . A[K][M]
  GemmParams P = gemm_params(plan, N, M, K, Bt, ldbt, A, lda, alpha, alpha_dev);
  P.C = workspace;
  const int rc = launch(plan, P, s);
  if (rc) return rc;
  if (plan.slab == SlabType::BF16)
    return gpt2mi::splitk_reduce16_t((const bf16*)workspace, plan.splits, N, M, C, accumulate, s);
  return gpt2mi::splitk_reduce_t(workspace, plan.splits, N, M, C, accumulate, s);
}
