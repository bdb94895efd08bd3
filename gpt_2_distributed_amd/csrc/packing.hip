// Document bounds of packed rows (gpt_2_distributed_amd/packing.py, doc_bounds_reference is the rule): for every
// position t of a row of tokens the document [start[t], end[t]) that holds it, from the separator tokens of the row.
// The masked attention kernels (attention.hip, fp32.hip) read start in forward / dQ and end in dK/dV.
//
// A document begins at position p ("p is a boundary") when idx[p - 1] is the separator (eot closes a document,
// nanoGPT's data preparation) or when idx[p] is (eot opens one, llm.c's); only positions below T_valid count. Then
//   start[t] = max{boundary p <= t}, or 0          end[t] = min{boundary p > t}, or T_valid          (t < T_valid)
// and the padding [T_valid, T) is one document of its own. Both are scans: a running maximum forward, a running minimum
// backward. One workgroup per row; thread i owns the contiguous chunk [i c, (i + 1) c) of it, c = ceil(T / 256): it
// reduces its chunk, the 256 chunk results are scanned in LDS (Hillis-Steele, 8 steps), and it walks its chunk again
// from the scanned value of its neighbours. No atomics, no host synchronisation, any T.
#include "common.h"

namespace {

constexpr int kBThreads = 256;

template <bool BEGIN>
__device__ __forceinline__ bool is_boundary(const int64_t* __restrict__ row, int p, int T_valid, int64_t eot) {
  if (p >= T_valid) return false;
  return BEGIN ? row[p] == eot : (p > 0 && row[p - 1] == eot);
}

template <bool BEGIN>
__global__ __launch_bounds__(kBThreads) void doc_bounds_kernel(const int64_t* __restrict__ idx, int T, int T_valid,
                                                               int64_t eot, int* __restrict__ start,
                                                               int* __restrict__ end) {
  __shared__ int smax[kBThreads], smin[kBThreads];
  const int64_t* row = idx + (size_t)blockIdx.x * T;
  int* srow = start + (size_t)blockIdx.x * T;
  int* erow = end + (size_t)blockIdx.x * T;
  const int i = threadIdx.x;
  const int c = (T + kBThreads - 1) / kBThreads;
  const int t0 = min(i * c, T), t1 = min(t0 + c, T);
  int last = 0, first = T_valid;  // the chunk's last / first boundary (0 / T_valid: none)
  for (int t = t0; t < t1; ++t)
    if (is_boundary<BEGIN>(row, t, T_valid, eot)) {
      last = t;
      first = min(first, t);
    }
  smax[i] = last;
  smin[i] = first;
  __syncthreads();
  // inclusive scans over the chunks: smax[i] = max of chunks 0..i, smin[i] = min of chunks i..255
  for (int o = 1; o < kBThreads; o <<= 1) {
    const int a = i >= o ? smax[i - o] : 0;
    const int b = i + o < kBThreads ? smin[i + o] : T_valid;
    __syncthreads();
    smax[i] = max(smax[i], a);
    smin[i] = min(smin[i], b);
    __syncthreads();
  }
  int run = i > 0 ? smax[i - 1] : 0;  // the last boundary before the chunk
  for (int t = t0; t < t1; ++t) {
    if (is_boundary<BEGIN>(row, t, T_valid, eot)) run = t;
    srow[t] = t < T_valid ? run : T_valid;
  }
  run = i + 1 < kBThreads ? smin[i + 1] : T_valid;  // the first boundary after the chunk
  for (int t = t1 - 1; t >= t0; --t) {
    erow[t] = t < T_valid ? run : T;
    if (is_boundary<BEGIN>(row, t, T_valid, eot)) run = t;
  }
}

}  // namespace

GPT2MI_EXPORT int gpt2mi_doc_bounds(const int64_t* idx, int B, int T, int T_valid, int64_t eot, int eot_begin,
                                    int* start, int* end, void* stream) {
  GPT2MI_REQUIRE(idx != nullptr && start != nullptr && end != nullptr, "doc_bounds: idx / start / end is NULL");
  GPT2MI_REQUIRE(B > 0 && T > 0, "doc_bounds: B=%d T=%d must be positive", B, T);
  GPT2MI_REQUIRE(T_valid > 0 && T_valid <= T, "doc_bounds: T_valid=%d must be in [1, T=%d]", T_valid, T);
  GPT2MI_REQUIRE(eot_begin == 0 || eot_begin == 1, "doc_bounds: eot_begin=%d must be 0 or 1", eot_begin);
  if (eot_begin)
    doc_bounds_kernel<true><<<B, kBThreads, 0, (hipStream_t)stream>>>(idx, T, T_valid, eot, start, end);
  else
    doc_bounds_kernel<false><<<B, kBThreads, 0, (hipStream_t)stream>>>(idx, T, T_valid, eot, start, end);
  return gpt2mi::check_launch("doc_bounds");
}
