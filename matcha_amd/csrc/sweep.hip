// De novo k-way sweep: the candidates of a region made on the device from their rank, and a streaming selection that
// keeps the best K (score, rank) pairs across chunks without the scores ever leaving the device.
//
// Candidates.  A candidate of size k in the region [lo, lo + n) is a strictly ascending k-tuple of node ids whose adjacent differences
// are all >= min_gap (generate_kmers.py:18, :33 and the sampler's rule with min_gap = min_distance + 1).  With s = min_gap - 1 and
// m = n - (k - 1) s, y_j = x_j - lo - j s maps them, order preserved, onto the plain k-subsets of [0, m): C(m, k) of them, ranked
// lexicographically from 0.
//
//   kway_rows_kernel   one thread per row.  The lexicographic rank r of y equals total - 1 - (colexicographic rank of the mirrored set
//                      z_j = m - 1 - y_j), so the row is read off the combinatorial number system of q = total - 1 - r: for j = k .. 1
//                      the largest c with C(c, j) <= q (z_{k-j} = c, q -= C(c, j)).  c is estimated as (q j!)^(1/j) + (j - 1) / 2 in
//                      float64 and corrected with exact integer binomials, so the result does not depend on the estimate.  64-bit
//                      integers throughout: C(a, j) is built as C(a-j+i, i) = C(a-j+i-1, i-1) (a-j+i) / i with gcd(a-j+i, i) divided out
//                      of both factors first, which keeps every intermediate <= the result (n = 120 000, k = 4 has C > 2^61, where
//                      the plain product passes 2^64).  Rows go through LDS and leave as one contiguous, coalesced run per block.
//                      The same kernel serves a range of ranks (rank0 + i) and a device list of ranks (the winners at the end).
//
// Selection.  The total order is: higher score first (IEEE comparison: -0.0 == +0.0, +inf highest, -inf lowest), then lower rank; NaN
// scores and rows with skip[i] != 0 are never kept.  The state is the K best pairs so far, sorted, padded with sentinels.
//
//   topk_init_kernel   fills the state with sentinels (no memset).
//   topk_keys_kernel   score -> 32-bit key that sorts ascending in the order above (-0.0 folded onto +0.0 in the key only; the stored
//                      score keeps its bits), invalid rows -> the sentinel key; value = the row's index in the chunk.
//   rocPRIM radix sort of (key, index): stable, and the chunk's ranks ascend with the index, so the chunk comes out in the total order.
//   topk_merge_kernel  merge path over the sorted state and the chunk's best min(K, n) rows: output position p finds its split by a
//                      binary search on the composite (key, rank) and takes one element.
//   topk_commit_kernel copies the merged K back into the state.
//   topk_read_kernel   scores, ranks and the number of valid pairs (the first sentinel's position).
//
// No atomics of any kind: every output element has one owner, so the state after a sequence of updates depends only on the multiset of
// (score, rank) pairs seen -- not on how the stream was cut, and not on timing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include <rocprim/device/device_radix_sort.hpp>

#include "kernels.hpp"

namespace matcha {
namespace {

constexpr int kMaxK = MATCHA_MAX_L;            // candidate sizes 2 .. 8
constexpr int kRowsPerBlock = 256;
constexpr uint32_t kSentinel = 0xFFFFFFFFu;    // sorts behind every real key (the worst real key is -inf: 0xFF800000)

__host__ __device__ __forceinline__ uint32_t gcd_small(uint32_t a, uint32_t b) {
  while (b) { const uint32_t t = a % b; a = b; b = t; }
  return a;
}

// r / d for d in 1 .. 8 with constant divisors (a 64-bit division by a variable is a long software routine on the device)
__host__ __device__ __forceinline__ uint64_t div_small(uint64_t r, uint32_t d) {
  switch (d) {
    case 2: return r / 2;
    case 3: return r / 3;
    case 4: return r / 4;
    case 5: return r / 5;
    case 6: return r / 6;
    case 7: return r / 7;
    case 8: return r / 8;
    default: return r;
  }
}
__host__ __device__ __forceinline__ uint32_t div_small32(uint32_t r, uint32_t d) {
  switch (d) {
    case 2: return r / 2;
    case 3: return r / 3;
    case 4: return r / 4;
    case 5: return r / 5;
    case 6: return r / 6;
    case 7: return r / 7;
    case 8: return r / 8;
    default: return r;
  }
}

// C(a, j) for 0 <= j <= 8 and 0 <= a < 2^31; exact whenever the result fits 64 bits: step i holds C(a-j+i, i), which grows with i,
// and i / gcd(a-j+i, i) divides the previous value because it is coprime to the other factor.
__host__ __device__ __forceinline__ uint64_t binom(int64_t a, int j) {
  if (a < j) return 0;
  uint64_t r = 1;
  for (int i = 1; i <= j; ++i) {
    const uint32_t t = (uint32_t)(a - j + i);
    const uint32_t g = gcd_small(t % (uint32_t)i, (uint32_t)i);
    r = div_small(r, (uint32_t)i / g) * div_small32(t, g);
  }
  return r;
}

// C(m, k) on the host, -1 when it does not fit a signed 64-bit integer (the intermediates grow with i, so the first one over decides)
int64_t count_subsets(int64_t m, int k) {
  if (m < k) return 0;
  unsigned __int128 r = 1;
  const unsigned __int128 lim = (unsigned __int128)1 << 63;
  for (int i = 1; i <= k; ++i) {
    r = r * (unsigned __int128)(m - k + i) / (unsigned __int128)i;
    if (r >= lim) return -1;
  }
  return (int64_t)r;
}

bool kway_args_ok(int32_t n, int32_t k, int32_t min_gap) { return n >= 1 && k >= 2 && k <= kMaxK && min_gap >= 1; }

int64_t kway_count(int32_t n, int32_t k, int32_t min_gap) {
  if (!kway_args_ok(n, k, min_gap)) return -1;
  const int64_t m = (int64_t)n - (int64_t)(k - 1) * (min_gap - 1);
  return count_subsets(m, k);
}

// y[0 .. k): the k-subset of [0, m) of lexicographic rank r, 0 <= r < total = C(m, k)
__device__ __forceinline__ void unrank(uint64_t r, uint64_t total, int32_t m, int k, int32_t (&y)[kMaxK]) {
  const double fact[kMaxK + 1] = {1., 1., 2., 6., 24., 120., 720., 5040., 40320.};
  uint64_t q = total - 1 - r;
  int64_t upper = (int64_t)m - 1;                                      // invariant: q < C(upper + 1, j)
#pragma unroll
  for (int s = 0; s < kMaxK; ++s) {
    if (s < k) {
      const int j = k - s;
      int64_t c;
      if (j == 1) {
        c = (int64_t)q;
      } else {
        c = (int64_t)(pow((double)q * fact[j], 1.0 / (double)j) + 0.5 * (double)(j - 1));
        c = c < j - 1 ? j - 1 : c;
        c = c > upper ? upper : c;
        uint64_t b = binom(c, j);
        while (b > q) { --c; b = binom(c, j); }                        // ends at c = j - 1 at the latest: C(j - 1, j) = 0
        while (c < upper) {
          const uint64_t b1 = binom(c + 1, j);
          if (b1 > q) break;
          ++c;
          b = b1;
        }
        q -= b;
      }
      y[s] = (int32_t)((int64_t)m - 1 - c);
      upper = c - 1;
    }
  }
}

__global__ __launch_bounds__(kRowsPerBlock) void kway_rows_kernel(int64_t lo, int32_t m, int32_t k, int32_t slack, uint64_t total, int64_t rank0,
                                                                  const int64_t* __restrict__ ranks, int64_t count, int32_t L,
                                                                  int64_t* __restrict__ x) {
  __shared__ int64_t tile[kRowsPerBlock * kMaxK];
  for (int64_t base = (int64_t)blockIdx.x * kRowsPerBlock; base < count; base += (int64_t)gridDim.x * kRowsPerBlock) {
    const int64_t i = base + threadIdx.x;
    if (i < count) {
      const int64_t r = ranks ? ranks[i] : rank0 + i;
      const bool ok = r >= 0 && (uint64_t)r < total;
      int32_t y[kMaxK] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ok) unrank((uint64_t)r, total, m, k, y);
#pragma unroll
      for (int c = 0; c < kMaxK; ++c)
        if (c < L) tile[threadIdx.x * L + c] = (ok && c < k) ? lo + (int64_t)y[c] + (int64_t)c * slack : 0;
    }
    __syncthreads();
    const int64_t rows = count - base < kRowsPerBlock ? count - base : kRowsPerBlock;
    const int elems = (int)rows * L;
    for (int e = threadIdx.x; e < elems; e += kRowsPerBlock) x[base * L + e] = tile[e];
    __syncthreads();                                                   // the tile is reused by the next run of rows
  }
}

// ---- selection ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t score_key(float s) {
  if (s != s) return kSentinel;
  uint32_t b = __builtin_bit_cast(uint32_t, s);
  if (b == 0x80000000u) b = 0;                                         // -0.0 == +0.0: one key, the rank decides
  const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ~asc;                                                         // ascending key = descending score
}

struct TopkPlan {
  size_t off_key, off_score, off_rank;        // the state: K sorted pairs
  size_t off_tkey, off_tscore, off_trank;     // the merged K before they are committed
  size_t off_ckey, off_cidx, off_skey, off_sidx, off_sort, sort_bytes, total;
};

bool topk_args_ok(int64_t K, int64_t max_chunk) {
  return K >= 1 && K <= ((int64_t)1 << 31) - 1 && max_chunk >= 1 && max_chunk <= ((int64_t)1 << 31) - 1;
}

// The radix sort's scratch is reserved by a bound (two buffers of keys and values plus its histograms and look-back state), not by asking
// rocPRIM: sizing must work where there is no device.  matcha_topk_update checks the bound against what rocPRIM asks for.
TopkPlan make_tplan(int64_t K, int64_t max_chunk) {
  TopkPlan pl;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  pl.off_key = take((size_t)K * 4);
  pl.off_score = take((size_t)K * 4);
  pl.off_rank = take((size_t)K * 8);
  pl.off_tkey = take((size_t)K * 4);
  pl.off_tscore = take((size_t)K * 4);
  pl.off_trank = take((size_t)K * 8);
  pl.off_ckey = take((size_t)max_chunk * 4);
  pl.off_cidx = take((size_t)max_chunk * 4);
  pl.off_skey = take((size_t)max_chunk * 4);
  pl.off_sidx = take((size_t)max_chunk * 4);
  pl.sort_bytes = (size_t)max_chunk * 16 + ((size_t)4 << 20);
  pl.off_sort = take(pl.sort_bytes);
  pl.total = off;
  return pl;
}

struct TopkState {
  uint32_t* key;
  float* score;
  int64_t* rank;
};

TopkState state_at(void* base, size_t off_key, size_t off_score, size_t off_rank) {
  char* w = (char*)base;
  return TopkState{(uint32_t*)(w + off_key), (float*)(w + off_score), (int64_t*)(w + off_rank)};
}

__global__ __launch_bounds__(256) void topk_init_kernel(TopkState st, int64_t K) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= K) return;
  st.key[p] = kSentinel;
  st.score[p] = 0.f;
  st.rank[p] = -1;
}

__global__ __launch_bounds__(256) void topk_keys_kernel(const float* __restrict__ scores, const int32_t* __restrict__ skip, int64_t n,
                                                        uint32_t* __restrict__ key, uint32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool skipped = skip && skip[i] != 0;
  key[i] = skipped ? kSentinel : score_key(scores[i]);
  idx[i] = (uint32_t)i;
}

// (key, rank) of the state before (key, rank) of the chunk?  Equal pairs (the same rank fed twice) go either way: they are the same pair.
__device__ __forceinline__ bool state_first(uint32_t ka, int64_t ra, uint32_t kb, int64_t rb) { return ka < kb || (ka == kb && ra <= rb); }

__global__ __launch_bounds__(256) void topk_merge_kernel(TopkState a, int64_t K, const uint32_t* __restrict__ bkey, const uint32_t* __restrict__ bidx,
                                                         int64_t nb, const float* __restrict__ scores, int64_t rank0, TopkState out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= K) return;
  // ia = how many of the first p merged elements come from the state: the smallest ia whose successor in the state does not precede the
  // chunk element it would displace
  int64_t lo = p > nb ? p - nb : 0, hi = p;                            // p < K, so ia <= p < K
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int64_t jb = p - 1 - mid;                                    // in [0, nb)
    if (state_first(a.key[mid], a.rank[mid], bkey[jb], rank0 + (int64_t)bidx[jb])) lo = mid + 1;
    else hi = mid;
  }
  const int64_t ia = lo, ib = p - lo;
  bool from_a = true;
  if (ib < nb) from_a = state_first(a.key[ia], a.rank[ia], bkey[ib], rank0 + (int64_t)bidx[ib]);
  uint32_t key;
  float score;
  int64_t rank;
  if (from_a) {
    key = a.key[ia]; score = a.score[ia]; rank = a.rank[ia];
  } else {
    key = bkey[ib]; score = scores[bidx[ib]]; rank = rank0 + (int64_t)bidx[ib];
  }
  if (key == kSentinel) { score = 0.f; rank = -1; }
  out.key[p] = key;
  out.score[p] = score;
  out.rank[p] = rank;
}

__global__ __launch_bounds__(256) void topk_commit_kernel(TopkState from, TopkState to, int64_t K) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= K) return;
  to.key[p] = from.key[p];
  to.score[p] = from.score[p];
  to.rank[p] = from.rank[p];
}

__global__ __launch_bounds__(256) void topk_read_kernel(TopkState st, int64_t K, float* __restrict__ scores_out, int64_t* __restrict__ ranks_out,
                                                        int64_t* __restrict__ n_out) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= K) return;
  const bool valid = st.key[p] != kSentinel;
  scores_out[p] = st.score[p];
  ranks_out[p] = st.rank[p];
  // the valid pairs are a prefix: its end has exactly one owner
  if (valid && (p == K - 1 || st.key[p + 1] == kSentinel)) *n_out = p + 1;
  if (!valid && p == 0) *n_out = 0;
}

}  // namespace
}  // namespace matcha

using namespace matcha;

extern "C" int64_t matcha_kway_count(int32_t n, int32_t k, int32_t min_gap) { return kway_count(n, k, min_gap); }

extern "C" int matcha_kway_rows(int64_t lo, int32_t n, int32_t k, int32_t min_gap, int64_t rank0, const int64_t* ranks, int64_t count, int32_t L,
                                int64_t* x, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(kway_args_ok(n, k, min_gap), "matcha_kway_rows: need n >= 1, 2 <= k <= %d, min_gap >= 1 (n=%d k=%d min_gap=%d)", kMaxK, n, k, min_gap);
  MATCHA_CHECK_ARG(L >= k && L <= kMaxK, "matcha_kway_rows: row width L=%d must be in [k, %d]", L, kMaxK);
  MATCHA_CHECK_ARG(lo >= 0 && lo <= ((int64_t)1 << 62), "matcha_kway_rows: lo out of range");
  const int64_t total = kway_count(n, k, min_gap);
  MATCHA_CHECK_ARG(total >= 0, "matcha_kway_rows: C(m, k) does not fit 63 bits (n=%d k=%d min_gap=%d)", n, k, min_gap);
  MATCHA_CHECK_ARG(count >= 0 && count <= ((int64_t)1 << 40), "matcha_kway_rows: count out of range");
  if (!ranks)
    MATCHA_CHECK_ARG(rank0 >= 0 && rank0 <= total && count <= total - rank0,
                     "matcha_kway_rows: ranks [%lld, %lld) outside [0, %lld)", (long long)rank0, (long long)(rank0 + count), (long long)total);
  if (count == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(x, "matcha_kway_rows: null output");
  const int32_t slack = min_gap - 1;
  const int64_t m64 = (int64_t)n - (int64_t)(k - 1) * slack;
  const int32_t m = m64 > 0 ? (int32_t)m64 : 0;
  int64_t blocks = cdiv(count, kRowsPerBlock);
  if (blocks > (1 << 20)) blocks = 1 << 20;
  hipLaunchKernelGGL(kway_rows_kernel, dim3((unsigned)blocks), dim3(kRowsPerBlock), 0, (hipStream_t)stream, lo, m, k, slack, (uint64_t)total, rank0,
                     ranks, count, L, x);
  MATCHA_CHECK_LAUNCH("kway_rows_kernel");
  return MATCHA_OK;
}

extern "C" size_t matcha_topk_bytes(int32_t K, int64_t max_chunk) {
  if (!topk_args_ok(K, max_chunk)) return 0;
  return make_tplan(K, max_chunk).total;
}

#define TOPK_COMMON_ARGS(fn)                                                                                                          \
  MATCHA_CHECK_ARG(state, fn ": null state");                                                                                         \
  MATCHA_CHECK_ARG(topk_args_ok(K, max_chunk), fn ": need 1 <= K < 2^31 and 1 <= max_chunk < 2^31 (K=%d max_chunk=%lld)", K,          \
                   (long long)max_chunk);                                                                                             \
  MATCHA_CHECK_ARG(((uintptr_t)state) % 8 == 0, fn ": state must be 8-byte aligned");                                                 \
  const TopkPlan pl = make_tplan(K, max_chunk);                                                                                       \
  MATCHA_CHECK_ARG(bytes >= pl.total, fn ": state too small (%zu bytes, matcha_topk_bytes says %zu)", bytes, pl.total)

extern "C" int matcha_topk_init(void* state, size_t bytes, int32_t K, int64_t max_chunk, matcha_stream_t stream) {
  TOPK_COMMON_ARGS("matcha_topk_init");
  hipLaunchKernelGGL(topk_init_kernel, dim3((unsigned)cdiv(K, 256)), dim3(256), 0, (hipStream_t)stream,
                     state_at(state, pl.off_key, pl.off_score, pl.off_rank), (int64_t)K);
  MATCHA_CHECK_LAUNCH("topk_init_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_topk_update(void* state, size_t bytes, int32_t K, int64_t max_chunk, const float* scores, const int32_t* skip, int64_t n,
                                  int64_t rank0, matcha_stream_t stream) {
  TOPK_COMMON_ARGS("matcha_topk_update");
  MATCHA_CHECK_ARG(n >= 0 && n <= max_chunk, "matcha_topk_update: n=%lld outside [0, max_chunk=%lld]", (long long)n, (long long)max_chunk);
  MATCHA_CHECK_ARG(rank0 >= 0 && rank0 <= INT64_MAX - n, "matcha_topk_update: rank0 out of range");
  if (n == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(scores, "matcha_topk_update: null scores");
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)state;
  uint32_t* ckey = (uint32_t*)(w + pl.off_ckey);
  uint32_t* cidx = (uint32_t*)(w + pl.off_cidx);
  uint32_t* skey = (uint32_t*)(w + pl.off_skey);
  uint32_t* sidx = (uint32_t*)(w + pl.off_sidx);
  size_t need = 0;
  if (rocprim::radix_sort_pairs(nullptr, need, ckey, skey, cidx, sidx, (size_t)n, 0, 32, st) != hipSuccess || need > pl.sort_bytes) {
    set_error("matcha_topk_update: the radix sort asks for %zu bytes of scratch, %zu are reserved", need, pl.sort_bytes);
    return MATCHA_EHIP;
  }
  hipLaunchKernelGGL(topk_keys_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, scores, skip, n, ckey, cidx);
  MATCHA_CHECK_LAUNCH("topk_keys_kernel");
  size_t tb = pl.sort_bytes;
  if (rocprim::radix_sort_pairs(w + pl.off_sort, tb, ckey, skey, cidx, sidx, (size_t)n, 0, 32, st) != hipSuccess) {
    set_error("matcha_topk_update: radix sort failed");
    return MATCHA_EHIP;
  }
  const TopkState cur = state_at(state, pl.off_key, pl.off_score, pl.off_rank);
  const TopkState tmp = state_at(state, pl.off_tkey, pl.off_tscore, pl.off_trank);
  const int64_t nb = n < K ? n : (int64_t)K;
  const unsigned blocks = (unsigned)cdiv(K, 256);
  hipLaunchKernelGGL(topk_merge_kernel, dim3(blocks), dim3(256), 0, st, cur, (int64_t)K, skey, sidx, nb, scores, rank0, tmp);
  MATCHA_CHECK_LAUNCH("topk_merge_kernel");
  hipLaunchKernelGGL(topk_commit_kernel, dim3(blocks), dim3(256), 0, st, tmp, cur, (int64_t)K);
  MATCHA_CHECK_LAUNCH("topk_commit_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_topk_read(const void* state, size_t bytes, int32_t K, int64_t max_chunk, float* scores_out, int64_t* ranks_out,
                                int64_t* n_out, matcha_stream_t stream) {
  TOPK_COMMON_ARGS("matcha_topk_read");
  MATCHA_CHECK_ARG(scores_out && ranks_out && n_out, "matcha_topk_read: null output");
  hipLaunchKernelGGL(topk_read_kernel, dim3((unsigned)cdiv(K, 256)), dim3(256), 0, (hipStream_t)stream,
                     state_at((void*)state, pl.off_key, pl.off_score, pl.off_rank), (int64_t)K, scores_out, ranks_out, n_out);
  MATCHA_CHECK_LAUNCH("topk_read_kernel");
  return MATCHA_OK;
}

// ==== anchored sweep ================================================================================================
// The best K completions of every anchor.  An anchor row holds s fixed node ids (1 <= s <= k - 1); the free part is a candidate of
// size f = k - s of the partner region [lo, lo + n) under the rule above (f = 1: every node of the region, C_f = n).  With A anchor
// rows the global rank is g = a C_f + r: anchor index a, free rank r.  The row is the k ids sorted ascending (duplicates kept); it is
// valid iff every adjacent difference is >= min_gap, which rejects a free node on or near an anchor and every row of an anchor that
// breaks the rule itself.  Invalid rows keep their place in the rank space and hold real node ids; a flag marks them.
//
//   kway_anchor_rows_kernel  one thread per row: g / C_f once per row (32-bit when both fit), unrank() of the free rank, the anchor's
//                            ids read from the device table, a 19-exchange sorting network over 8 registers (pads = INT64_MAX), the
//                            gap test on unsigned differences.  Rows leave through LDS as in kway_rows_kernel, flags directly.
//
// Segmented selection: one top-K per segment of seg_len consecutive global ranks (the anchored sweep: seg_len = C_f, segment = anchor),
// under exactly the order of the plain selection.  A chunk may cover a fraction of one segment or thousands of them.
//
//   segtopk_init_kernel    sentinels into all A K slots.
//   segtopk_keys_kernel    64-bit key = (segment index within the chunk) << 32 | score key; value = the row's index in the chunk.
//   rocPRIM radix sort of (key, index) over the bits in use: stable, every row stays in its segment's group (sentinel rows last), so
//                          the sorted run of chunk segment t begins at max(0, t seg_len - off0), known by arithmetic.
//   segtopk_merge_kernel   one thread per (touched segment, position p < K): the merge path of topk_merge_kernel between the segment's
//                          state and the best min(K, run length) rows of its run.
//   segtopk_commit_kernel  copies the merged rows of the touched segments (a contiguous range of the state) back.
//   segtopk_read_kernel    scores, ranks and per-segment counts.
//
// No atomics; segments a chunk does not touch are neither read nor written.
namespace matcha {
namespace {

bool anchor_args_ok(int64_t A, int32_t s, int32_t n, int32_t k, int32_t min_gap) {
  return A >= 0 && n >= 1 && k >= 2 && k <= kMaxK && s >= 1 && s <= k - 1 && min_gap >= 1;
}

// C_f = C(n - (f - 1)(min_gap - 1), f) for f >= 1 (f = 1: n), -1 when it does not fit 63 bits
int64_t free_count(int32_t n, int32_t f, int32_t min_gap) {
  return count_subsets((int64_t)n - (int64_t)(f - 1) * (min_gap - 1), f);
}

// A C_f, -1 for invalid arguments or a total >= 2^63; *cf_out = C_f
int64_t anchor_count(int64_t A, int32_t s, int32_t n, int32_t k, int32_t min_gap, int64_t* cf_out) {
  if (!anchor_args_ok(A, s, n, k, min_gap)) return -1;
  const int64_t cf = free_count(n, k - s, min_gap);
  if (cf < 0) return -1;
  const unsigned __int128 total = (unsigned __int128)(uint64_t)A * (uint64_t)cf;
  if (total >= ((unsigned __int128)1 << 63)) return -1;
  if (cf_out) *cf_out = cf;
  return (int64_t)total;
}

__device__ __forceinline__ void order2(int64_t& a, int64_t& b) {
  const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

__global__ __launch_bounds__(kRowsPerBlock) void kway_anchor_rows_kernel(const int64_t* __restrict__ anchors, int32_t s, int64_t lo, int32_t m, int32_t f,
                                                                         int32_t slack, int32_t min_gap, uint64_t cf, uint64_t total, int64_t rank0,
                                                                         const int64_t* __restrict__ ranks, int64_t count, int32_t L,
                                                                         int64_t* __restrict__ x, int32_t* __restrict__ flag) {
  __shared__ int64_t tile[kRowsPerBlock * kMaxK];
  const int k = s + f;
  for (int64_t base = (int64_t)blockIdx.x * kRowsPerBlock; base < count; base += (int64_t)gridDim.x * kRowsPerBlock) {
    const int64_t i = base + threadIdx.x;
    if (i < count) {
      const int64_t g = ranks ? ranks[i] : rank0 + i;
      const bool ok = g >= 0 && (uint64_t)g < total;                   // total > 0 here, so cf > 0
      int64_t v[kMaxK] = {0, 0, 0, 0, 0, 0, 0, 0};
      bool bad = !ok;
      if (ok) {
        uint64_t a, r;
        if (((uint64_t)g | cf) >> 32) {                                // the one 64-bit division of the row
          a = (uint64_t)g / cf;
          r = (uint64_t)g - a * cf;
        } else {
          const uint32_t a32 = (uint32_t)g / (uint32_t)cf;
          a = a32;
          r = (uint32_t)g - a32 * (uint32_t)cf;
        }
        int32_t y[kMaxK] = {0, 0, 0, 0, 0, 0, 0, 0};
        unrank(r, cf, m, f, y);
        const int64_t* __restrict__ arow = anchors + a * (uint64_t)s;
#pragma unroll
        for (int c = 0; c < kMaxK; ++c) {
          if (c < f) v[c] = lo + (int64_t)y[c] + (int64_t)c * slack;
          else if (c < k) v[c] = arow[c - f];
          else v[c] = INT64_MAX;
        }
        order2(v[0], v[2]); order2(v[1], v[3]); order2(v[4], v[6]); order2(v[5], v[7]);
        order2(v[0], v[4]); order2(v[1], v[5]); order2(v[2], v[6]); order2(v[3], v[7]);
        order2(v[0], v[1]); order2(v[2], v[3]); order2(v[4], v[5]); order2(v[6], v[7]);
        order2(v[2], v[4]); order2(v[3], v[5]);
        order2(v[1], v[4]); order2(v[3], v[6]);
        order2(v[1], v[2]); order2(v[3], v[4]); order2(v[5], v[6]);
#pragma unroll
        for (int c = 1; c < kMaxK; ++c)                                // sorted, so the unsigned difference is exact for any int64 ids
          if (c < k) bad |= (uint64_t)v[c] - (uint64_t)v[c - 1] < (uint64_t)min_gap;
      }
#pragma unroll
      for (int c = 0; c < kMaxK; ++c)
        if (c < L) tile[threadIdx.x * L + c] = (ok && c < k) ? v[c] : 0;
      flag[i] = bad ? 1 : 0;
    }
    __syncthreads();
    const int64_t rows = count - base < kRowsPerBlock ? count - base : kRowsPerBlock;
    const int elems = (int)rows * L;
    for (int e = threadIdx.x; e < elems; e += kRowsPerBlock) x[base * L + e] = tile[e];
    __syncthreads();                                                   // the tile is reused by the next run of rows
  }
}

// ---- segmented selection ---------------------------------------------------------------------------------------------------------
struct SegPlan {
  size_t off_key, off_score, off_rank;        // the state: A segments of K sorted pairs
  size_t off_tkey, off_tscore, off_trank;     // the merged rows of the touched segments before they are committed
  size_t off_ckey, off_cidx, off_skey, off_sidx, off_sort, sort_bytes, total;
  int64_t tmax;                               // the most segments one update can touch
};

bool seg_args_ok(int64_t A, int64_t K, int64_t seg_len, int64_t max_chunk) {
  const int64_t lim = ((int64_t)1 << 31) - 1;
  return K >= 1 && K <= lim && A >= 1 && A <= lim / K && seg_len >= 1 && max_chunk >= 1 && max_chunk <= lim;
}

// As make_tplan: the sort's scratch is a bound (64-bit keys and 32-bit values twice over plus histograms), checked in the update.
SegPlan make_splan(int64_t A, int64_t K, int64_t seg_len, int64_t max_chunk) {
  SegPlan pl;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  const int64_t by_chunk = (max_chunk - 1) / seg_len + 2;              // off0 < seg_len: (off0 + n - 1) / seg_len + 1 <= (n - 2) / seg_len + 2
  pl.tmax = A < by_chunk ? A : by_chunk;
  const size_t slots = (size_t)A * (size_t)K, tslots = (size_t)pl.tmax * (size_t)K;
  pl.off_key = take(slots * 4);
  pl.off_score = take(slots * 4);
  pl.off_rank = take(slots * 8);
  pl.off_tkey = take(tslots * 4);
  pl.off_tscore = take(tslots * 4);
  pl.off_trank = take(tslots * 8);
  pl.off_ckey = take((size_t)max_chunk * 8);
  pl.off_cidx = take((size_t)max_chunk * 4);
  pl.off_skey = take((size_t)max_chunk * 8);
  pl.off_sidx = take((size_t)max_chunk * 4);
  pl.sort_bytes = (size_t)max_chunk * 24 + ((size_t)4 << 20);
  pl.off_sort = take(pl.sort_bytes);
  pl.total = off;
  return pl;
}

__global__ __launch_bounds__(256) void segtopk_init_kernel(TopkState st, int64_t slots) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= slots) return;
  st.key[p] = kSentinel;
  st.score[p] = 0.f;
  st.rank[p] = -1;
}

// off0 = (rank of row 0) mod seg_len.  wide (seg_len >= 2^31 > n): a chunk touches at most two segments, one comparison; otherwise
// off0 + i < 2^32 and the division is a 32-bit one.
__global__ __launch_bounds__(256) void segtopk_keys_kernel(const float* __restrict__ scores, const int32_t* __restrict__ skip, int64_t n, uint64_t off0,
                                                           uint64_t seg_len, int wide, uint64_t* __restrict__ key, uint32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool skipped = skip && skip[i] != 0;
  const uint32_t k32 = skipped ? kSentinel : score_key(scores[i]);
  const uint32_t t = wide ? (uint32_t)(off0 + (uint64_t)i >= seg_len) : (uint32_t)(off0 + (uint64_t)i) / (uint32_t)seg_len;
  key[i] = ((uint64_t)t << 32) | k32;
  idx[i] = (uint32_t)i;
}

// thread (t, p): chunk segment t is state segment seg_first + t; its sorted run is [start, end) of the sorted chunk
__global__ __launch_bounds__(256) void segtopk_merge_kernel(TopkState st, uint32_t K, int64_t T, int64_t seg_first, uint64_t off0, uint64_t seg_len, int64_t n,
                                                            const uint64_t* __restrict__ skey, const uint32_t* __restrict__ sidx,
                                                            const float* __restrict__ scores, int64_t g0, TopkState out) {
  const int64_t flat = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (flat >= T * (int64_t)K) return;                                  // T K < 2^31
  const uint32_t t = (uint32_t)flat / K;
  const int64_t p = (int64_t)((uint32_t)flat - t * K);
  // t >= 1 only when seg_len <= off0 + n - 1 < 2^32, so the products below cannot overflow
  const int64_t start = t == 0 ? 0 : (int64_t)((uint64_t)t * seg_len - off0);
  const uint64_t room = ((uint64_t)t + 1) * seg_len - off0;            // rows of the chunk before the next segment begins
  const int64_t end = room < (uint64_t)n ? (int64_t)room : n;
  const int64_t len = end - start;
  const int64_t nb = len < (int64_t)K ? len : (int64_t)K;
  const int64_t sbase = (seg_first + (int64_t)t) * (int64_t)K;
  const uint32_t* __restrict__ akey = st.key + sbase;
  const int64_t* __restrict__ arank = st.rank + sbase;
  const uint64_t* __restrict__ bkey = skey + start;
  const uint32_t* __restrict__ bidx = sidx + start;
  int64_t lo = p > nb ? p - nb : 0, hi = p;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int64_t jb = p - 1 - mid;                                    // in [0, nb)
    if (state_first(akey[mid], arank[mid], (uint32_t)bkey[jb], g0 + (int64_t)bidx[jb])) lo = mid + 1;
    else hi = mid;
  }
  const int64_t ia = lo, ib = p - lo;
  bool from_a = true;
  if (ib < nb) from_a = state_first(akey[ia], arank[ia], (uint32_t)bkey[ib], g0 + (int64_t)bidx[ib]);
  uint32_t key;
  float score;
  int64_t rank;
  if (from_a) {
    key = akey[ia]; score = st.score[sbase + ia]; rank = arank[ia];
  } else {
    key = (uint32_t)bkey[ib]; score = scores[bidx[ib]]; rank = g0 + (int64_t)bidx[ib];
  }
  if (key == kSentinel) { score = 0.f; rank = -1; }
  out.key[flat] = key;
  out.score[flat] = score;
  out.rank[flat] = rank;
}

__global__ __launch_bounds__(256) void segtopk_commit_kernel(TopkState from, TopkState to, int64_t to_base, int64_t slots) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= slots) return;
  to.key[to_base + p] = from.key[p];
  to.score[to_base + p] = from.score[p];
  to.rank[to_base + p] = from.rank[p];
}

__global__ __launch_bounds__(256) void segtopk_read_kernel(TopkState st, uint32_t K, int64_t slots, float* __restrict__ scores_out,
                                                           int64_t* __restrict__ ranks_out, int64_t* __restrict__ counts_out) {
  const int64_t flat = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (flat >= slots) return;
  const uint32_t a = (uint32_t)flat / K, p = (uint32_t)flat - a * K;
  const bool valid = st.key[flat] != kSentinel;
  scores_out[flat] = st.score[flat];
  ranks_out[flat] = st.rank[flat];
  // the valid pairs of a segment are a prefix: its end has exactly one owner
  if (valid && (p == K - 1 || st.key[flat + 1] == kSentinel)) counts_out[a] = (int64_t)p + 1;
  if (!valid && p == 0) counts_out[a] = 0;
}

}  // namespace
}  // namespace matcha

extern "C" int64_t matcha_kway_anchor_count(int64_t A, int32_t s, int32_t n, int32_t k, int32_t min_gap) {
  return anchor_count(A, s, n, k, min_gap, nullptr);
}

extern "C" int matcha_kway_anchor_rows(const int64_t* anchors, int64_t A, int32_t s, int64_t lo, int32_t n, int32_t k, int32_t min_gap, int64_t rank0,
                                       const int64_t* ranks, int64_t count, int32_t L, int64_t* x, int32_t* flag, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(anchor_args_ok(A, s, n, k, min_gap),
                   "matcha_kway_anchor_rows: need A >= 0, n >= 1, 2 <= k <= %d, 1 <= s <= k - 1, min_gap >= 1 (A=%lld s=%d n=%d k=%d min_gap=%d)", kMaxK,
                   (long long)A, s, n, k, min_gap);
  MATCHA_CHECK_ARG(L >= k && L <= kMaxK, "matcha_kway_anchor_rows: row width L=%d must be in [k, %d]", L, kMaxK);
  MATCHA_CHECK_ARG(lo >= 0 && lo <= ((int64_t)1 << 62), "matcha_kway_anchor_rows: lo out of range");
  int64_t cf = 0;
  const int64_t total = anchor_count(A, s, n, k, min_gap, &cf);
  MATCHA_CHECK_ARG(total >= 0, "matcha_kway_anchor_rows: A C_f does not fit 63 bits (A=%lld s=%d n=%d k=%d min_gap=%d)", (long long)A, s, n, k, min_gap);
  MATCHA_CHECK_ARG(count >= 0 && count <= ((int64_t)1 << 40), "matcha_kway_anchor_rows: count out of range");
  if (!ranks)
    MATCHA_CHECK_ARG(rank0 >= 0 && rank0 <= total && count <= total - rank0,
                     "matcha_kway_anchor_rows: ranks [%lld, %lld) outside [0, %lld)", (long long)rank0, (long long)(rank0 + count), (long long)total);
  if (count == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(x && flag, "matcha_kway_anchor_rows: null output");
  MATCHA_CHECK_ARG(anchors || total == 0, "matcha_kway_anchor_rows: null anchors");
  const int32_t f = k - s, slack = min_gap - 1;
  const int64_t m64 = (int64_t)n - (int64_t)(f - 1) * slack;
  const int32_t m = m64 > 0 ? (int32_t)m64 : 0;
  int64_t blocks = cdiv(count, kRowsPerBlock);
  if (blocks > (1 << 20)) blocks = 1 << 20;
  hipLaunchKernelGGL(kway_anchor_rows_kernel, dim3((unsigned)blocks), dim3(kRowsPerBlock), 0, (hipStream_t)stream, anchors, s, lo, m, f, slack, min_gap,
                     (uint64_t)cf, (uint64_t)total, rank0, ranks, count, L, x, flag);
  MATCHA_CHECK_LAUNCH("kway_anchor_rows_kernel");
  return MATCHA_OK;
}

extern "C" size_t matcha_segtopk_bytes(int64_t A, int32_t K, int64_t seg_len, int64_t max_chunk) {
  if (!seg_args_ok(A, K, seg_len, max_chunk)) return 0;
  return make_splan(A, K, seg_len, max_chunk).total;
}

#define SEGTOPK_COMMON_ARGS(fn)                                                                                                       \
  MATCHA_CHECK_ARG(state, fn ": null state");                                                                                         \
  MATCHA_CHECK_ARG(seg_args_ok(A, K, seg_len, max_chunk),                                                                             \
                   fn ": need 1 <= K, 1 <= A, A K < 2^31, seg_len >= 1 and 1 <= max_chunk < 2^31 (A=%lld K=%d seg_len=%lld max_chunk=%lld)",   \
                   (long long)A, K, (long long)seg_len, (long long)max_chunk);                                                       \
  MATCHA_CHECK_ARG(((uintptr_t)state) % 8 == 0, fn ": state must be 8-byte aligned");                                                 \
  const SegPlan pl = make_splan(A, K, seg_len, max_chunk);                                                                            \
  MATCHA_CHECK_ARG(bytes >= pl.total, fn ": state too small (%zu bytes, matcha_segtopk_bytes says %zu)", bytes, pl.total)

extern "C" int matcha_segtopk_init(void* state, size_t bytes, int64_t A, int32_t K, int64_t seg_len, int64_t max_chunk, matcha_stream_t stream) {
  SEGTOPK_COMMON_ARGS("matcha_segtopk_init");
  const int64_t slots = A * K;
  hipLaunchKernelGGL(segtopk_init_kernel, dim3((unsigned)cdiv(slots, 256)), dim3(256), 0, (hipStream_t)stream,
                     state_at(state, pl.off_key, pl.off_score, pl.off_rank), slots);
  MATCHA_CHECK_LAUNCH("segtopk_init_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_segtopk_update(void* state, size_t bytes, int64_t A, int32_t K, int64_t seg_len, int64_t max_chunk, int64_t seg0, const float* scores,
                                     const int32_t* skip, int64_t n, int64_t g0, matcha_stream_t stream) {
  SEGTOPK_COMMON_ARGS("matcha_segtopk_update");
  MATCHA_CHECK_ARG(n >= 0 && n <= max_chunk, "matcha_segtopk_update: n=%lld outside [0, max_chunk=%lld]", (long long)n, (long long)max_chunk);
  MATCHA_CHECK_ARG(g0 >= 0 && g0 <= INT64_MAX - n && seg0 >= 0, "matcha_segtopk_update: g0 or seg0 out of range");
  {
    const __int128 first = (__int128)seg0 * seg_len, past = ((__int128)seg0 + A) * seg_len;
    MATCHA_CHECK_ARG((__int128)g0 >= first && (__int128)g0 + n <= past,
                     "matcha_segtopk_update: ranks [%lld, %lld) outside the %lld segments of %lld ranks from segment %lld", (long long)g0,
                     (long long)(g0 + n), (long long)A, (long long)seg_len, (long long)seg0);
  }
  if (n == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(scores, "matcha_segtopk_update: null scores");
  const int64_t seg_first = g0 / seg_len - seg0;                       // in [0, A)
  const uint64_t off0 = (uint64_t)(g0 % seg_len);
  const int64_t T = (int64_t)((off0 + (uint64_t)n - 1) / (uint64_t)seg_len) + 1;   // touched segments, <= pl.tmax
  if (T > pl.tmax || seg_first + T > A) {
    set_error("matcha_segtopk_update: %lld touched segments, room for %lld", (long long)T, (long long)pl.tmax);
    return MATCHA_EINVAL;
  }
  int bits = 0;
  while (((int64_t)1 << bits) < T) ++bits;
  const unsigned end_bit = 32u + (unsigned)bits;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)state;
  uint64_t* ckey = (uint64_t*)(w + pl.off_ckey);
  uint32_t* cidx = (uint32_t*)(w + pl.off_cidx);
  uint64_t* skey = (uint64_t*)(w + pl.off_skey);
  uint32_t* sidx = (uint32_t*)(w + pl.off_sidx);
  size_t need = 0;
  if (rocprim::radix_sort_pairs(nullptr, need, ckey, skey, cidx, sidx, (size_t)n, 0, end_bit, st) != hipSuccess || need > pl.sort_bytes) {
    set_error("matcha_segtopk_update: the radix sort asks for %zu bytes of scratch, %zu are reserved", need, pl.sort_bytes);
    return MATCHA_EHIP;
  }
  const int wide = seg_len >= ((int64_t)1 << 31);
  hipLaunchKernelGGL(segtopk_keys_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, scores, skip, n, off0, (uint64_t)seg_len, wide, ckey, cidx);
  MATCHA_CHECK_LAUNCH("segtopk_keys_kernel");
  size_t tb = pl.sort_bytes;
  if (rocprim::radix_sort_pairs(w + pl.off_sort, tb, ckey, skey, cidx, sidx, (size_t)n, 0, end_bit, st) != hipSuccess) {
    set_error("matcha_segtopk_update: radix sort failed");
    return MATCHA_EHIP;
  }
  const TopkState cur = state_at(state, pl.off_key, pl.off_score, pl.off_rank);
  const TopkState tmp = state_at(state, pl.off_tkey, pl.off_tscore, pl.off_trank);
  const int64_t slots = T * K;
  const unsigned blocks = (unsigned)cdiv(slots, 256);
  hipLaunchKernelGGL(segtopk_merge_kernel, dim3(blocks), dim3(256), 0, st, cur, (uint32_t)K, T, seg_first, off0, (uint64_t)seg_len, n, skey, sidx, scores, g0,
                     tmp);
  MATCHA_CHECK_LAUNCH("segtopk_merge_kernel");
  hipLaunchKernelGGL(segtopk_commit_kernel, dim3(blocks), dim3(256), 0, st, tmp, cur, seg_first * K, slots);
  MATCHA_CHECK_LAUNCH("segtopk_commit_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_segtopk_read(const void* state, size_t bytes, int64_t A, int32_t K, int64_t seg_len, int64_t max_chunk, float* scores_out,
                                   int64_t* ranks_out, int64_t* counts_out, matcha_stream_t stream) {
  SEGTOPK_COMMON_ARGS("matcha_segtopk_read");
  MATCHA_CHECK_ARG(scores_out && ranks_out && counts_out, "matcha_segtopk_read: null output");
  const int64_t slots = A * K;
  hipLaunchKernelGGL(segtopk_read_kernel, dim3((unsigned)cdiv(slots, 256)), dim3(256), 0, (hipStream_t)stream,
                     state_at((void*)state, pl.off_key, pl.off_score, pl.off_rank), (uint32_t)K, slots, scores_out, ranks_out, counts_out);
  MATCHA_CHECK_LAUNCH("segtopk_read_kernel");
  return MATCHA_OK;
}

// ==== cluster completion =============================================================================================
// Which further bins best extend clusters of 1 to 31 loci.  A cluster table is int64 [A, S], 1 <= S <= 31: row a holds s_a non-zero ids
// followed by zeros; only the leading non-zero run is read.  The free part is a candidate of size f (1 <= f <= 8) of the partner region
// under the rule above, the global rank g = a C_f + r as in the anchored sweep.  The candidate is the s_a + f ids sorted ascending
// (duplicates kept, a cluster id before an equal free id), zero-padded to L, S + f <= L <= 32.  It is valid iff s_a >= 1, the cluster's
// own ids are non-descending and every adjacent difference of the row is >= min_gap.  The free part keeps the gap by construction, so
// the test is: every cluster id against its predecessor in the cluster (v < prev, or v - prev < min_gap unsigned) and against every free
// id (|v - free| < min_gap) -- a pair closer than the gap has an adjacent pair closer than the gap between them, and the reverse.  A
// cluster row that descends somewhere cannot be merged by counting; its ids leave in their order with the free ids behind them, flagged.
//
//   kway_complete_rows_kernel  a wavefront serves 64 consecutive ranks.  Each lane divides and unranks ONE of them (free ids relative to
//                              lo, int32).  Then the two 32-lane halves walk the 64 rows, one row each per step: the row's owner
//                              broadcasts its cluster index and free ids (__shfl), lane j < S reads cluster id j (consecutive ranks share
//                              the cluster: a cache hit), s_a is the first zero of a ballot.  Lane j < s_a writes its id to column
//                              j + #(free ids below it), lane s_a + i writes free id i to column i + #(cluster ids <= it) -- a popcount of
//                              a ballot --, the lanes behind write the zero padding: one store instruction per row, its lanes covering one
//                              contiguous run of 8 L bytes.  No LDS, no scratch.  Every shuffle and ballot is executed by all 64 lanes:
//                              a half without a row, or a lane without an id, is predicated, never branched around (the step count is
//                              the same for the whole wavefront).  Flags are collected in the owner lanes and leave as one coalesced run.
namespace matcha {
namespace {

constexpr int kMaxWide = MATCHA_MAX_LONG_L;    // the widest row: S + f <= L <= 32

bool complete_args_ok(int64_t A, int32_t S, int32_t n, int32_t f, int32_t min_gap) {
  return A >= 0 && S >= 1 && S <= kMaxWide - 1 && n >= 1 && f >= 1 && f <= kMaxK && min_gap >= 1;
}

// A C_f, -1 for invalid arguments or a total >= 2^63; *cf_out = C_f
int64_t complete_count(int64_t A, int32_t S, int32_t n, int32_t f, int32_t min_gap, int64_t* cf_out) {
  if (!complete_args_ok(A, S, n, f, min_gap)) return -1;
  const int64_t cf = free_count(n, f, min_gap);
  if (cf < 0) return -1;
  const unsigned __int128 total = (unsigned __int128)(uint64_t)A * (uint64_t)cf;
  if (total >= ((unsigned __int128)1 << 63)) return -1;
  if (cf_out) *cf_out = cf;
  return (int64_t)total;
}

__device__ __forceinline__ int64_t shfl64(int64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)((uint64_t)v >> 32), src);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

__global__ __launch_bounds__(kRowsPerBlock) void kway_complete_rows_kernel(const int64_t* __restrict__ clusters, int32_t S, int64_t lo, int32_t m, int32_t f,
                                                                           int32_t slack, int32_t min_gap, uint64_t cf, uint64_t total, int64_t rank0,
                                                                           const int64_t* __restrict__ ranks, int64_t count, int32_t L,
                                                                           int64_t* __restrict__ x, int32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31;
  const int64_t wave0 = (int64_t)(threadIdx.x >> 6) * 64;
  const uint64_t gap = (uint64_t)min_gap;
  for (int64_t base = (int64_t)blockIdx.x * kRowsPerBlock; base < count; base += (int64_t)gridDim.x * kRowsPerBlock) {
    const int64_t w0 = base + wave0;                                   // the wavefront's first row; the same in all its lanes
    const int64_t left = count - w0;
    const int steps = left >= 64 ? 32 : left > 0 ? (int)((left + 1) >> 1) : 0;
    // ---- one rank per lane: cluster index and free ids ----
    const int64_t i = w0 + lane;
    const int64_t g = i < count ? (ranks ? ranks[i] : rank0 + i) : -1;
    const int ok = g >= 0 && (uint64_t)g < total;                      // total > 0 then, so cf > 0
    uint64_t a = 0;
    int32_t fid[kMaxK] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) {
      uint64_t r;
      if (((uint64_t)g | cf) >> 32) {                                  // the one 64-bit division of the row
        a = (uint64_t)g / cf;
        r = (uint64_t)g - a * cf;
      } else {
        const uint32_t a32 = (uint32_t)g / (uint32_t)cf;
        a = a32;
        r = (uint32_t)g - a32 * (uint32_t)cf;
      }
      unrank(r, cf, m, f, fid);
#pragma unroll
      for (int c = 0; c < kMaxK; ++c) fid[c] += c * slack;              // < n: relative to lo
    }
    // ---- two rows per step, one per half ----
    int bad_mine = 1;
    for (int t = 0; t < steps; ++t) {
      const int own = 2 * t + h;                                       // the lane that unranked this half's row
      const int64_t irow = w0 + own;
      const int ok0 = __shfl(ok, 2 * t), ok1 = __shfl(ok, 2 * t + 1);
      const int ok_r = h ? ok1 : ok0;
      const uint64_t a_r = (uint64_t)shfl64((int64_t)a, own);
      int64_t fv[kMaxK];
#pragma unroll
      for (int c = 0; c < kMaxK; ++c) {
        fv[c] = 0;
        if (c < f) fv[c] = lo + (int64_t)__shfl(fid[c], own);           // f is a kernel argument: the same branch in every lane
      }
      int64_t v = 0;
      if (ok_r && j < S) v = clusters[a_r * (uint64_t)S + (uint64_t)j];
      const uint64_t zb = __ballot(v == 0);                            // lane 31 of a half never holds an id (S <= 31): ctz is defined
      const int s0 = __builtin_ctz((uint32_t)zb | 0x80000000u), s1 = __builtin_ctz((uint32_t)(zb >> 32) | 0x80000000u);
      const int s = h ? s1 : s0;
      const bool mine = j < s;
      const int64_t prev = shfl64(v, j ? lane - 1 : lane);
      const bool desc = mine && j > 0 && v < prev;
      bool close = mine && j > 0 && (uint64_t)v - (uint64_t)prev < gap;
      int below = 0;
#pragma unroll
      for (int c = 0; c < kMaxK; ++c) {
        if (c < f) {
          below += fv[c] < v ? 1 : 0;
          const uint64_t dist = v >= fv[c] ? (uint64_t)v - (uint64_t)fv[c] : (uint64_t)fv[c] - (uint64_t)v;   // exact for any int64 ids
          close |= mine && dist < gap;
        }
      }
      const uint64_t db = __ballot(desc);
      const bool merge = (uint32_t)(db >> (32 * h)) == 0;              // the cluster's ids are non-descending
      int64_t val = mine ? v : 0;
      int col = (mine && merge) ? j + below : j;
#pragma unroll
      for (int c = 0; c < kMaxK; ++c) {
        if (c < f) {
          const uint64_t le = __ballot(mine && v <= fv[c]);
          const int n_le = __popc((uint32_t)(le >> (32 * h)));
          if (j - s == c) {
            val = fv[c];
            col = merge ? c + n_le : j;
          }
        }
      }
      if (!ok_r) { val = 0; col = j; }
      const uint64_t bb = __ballot(desc || close);
      const int bad0 = !ok0 || s0 == 0 || (uint32_t)bb != 0, bad1 = !ok1 || s1 == 0 || (uint32_t)(bb >> 32) != 0;
      if (lane == 2 * t) bad_mine = bad0;
      if (lane == 2 * t + 1) bad_mine = bad1;
      if (irow < count && j < L && col < L) x[irow * L + col] = val;
    }
    if (i < count) flag[i] = bad_mine;
  }
}

}  // namespace
}  // namespace matcha

extern "C" int64_t matcha_kway_complete_count(int64_t A, int32_t S, int32_t n, int32_t f, int32_t min_gap) {
  return complete_count(A, S, n, f, min_gap, nullptr);
}

extern "C" int matcha_kway_complete_rows(const int64_t* clusters, int64_t A, int32_t S, int64_t lo, int32_t n, int32_t f, int32_t min_gap, int64_t rank0,
                                         const int64_t* ranks, int64_t count, int32_t L, int64_t* x, int32_t* flag, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(complete_args_ok(A, S, n, f, min_gap),
                   "matcha_kway_complete_rows: need A >= 0, 1 <= S <= %d, n >= 1, 1 <= f <= %d, min_gap >= 1 (A=%lld S=%d n=%d f=%d min_gap=%d)", kMaxWide - 1,
                   kMaxK, (long long)A, S, n, f, min_gap);
  MATCHA_CHECK_ARG(L >= S + f && L <= kMaxWide, "matcha_kway_complete_rows: row width L=%d must be in [S + f, %d]", L, kMaxWide);
  MATCHA_CHECK_ARG(lo >= 0 && lo <= ((int64_t)1 << 62), "matcha_kway_complete_rows: lo out of range");
  int64_t cf = 0;
  const int64_t total = complete_count(A, S, n, f, min_gap, &cf);
  MATCHA_CHECK_ARG(total >= 0, "matcha_kway_complete_rows: A C_f does not fit 63 bits (A=%lld n=%d f=%d min_gap=%d)", (long long)A, n, f, min_gap);
  MATCHA_CHECK_ARG(count >= 0 && count <= ((int64_t)1 << 40), "matcha_kway_complete_rows: count out of range");
  if (!ranks)
    MATCHA_CHECK_ARG(rank0 >= 0 && rank0 <= total && count <= total - rank0,
                     "matcha_kway_complete_rows: %lld ranks from %lld lie outside [0, %lld)", (long long)count, (long long)rank0, (long long)total);
  if (count == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(x && flag, "matcha_kway_complete_rows: null output");
  MATCHA_CHECK_ARG(clusters || total == 0, "matcha_kway_complete_rows: null clusters");
  const int32_t slack = min_gap - 1;
  const int64_t m64 = (int64_t)n - (int64_t)(f - 1) * slack;
  const int32_t m = m64 > 0 ? (int32_t)m64 : 0;
  int64_t blocks = cdiv(count, kRowsPerBlock);
  if (blocks > (1 << 20)) blocks = 1 << 20;
  hipLaunchKernelGGL(kway_complete_rows_kernel, dim3((unsigned)blocks), dim3(kRowsPerBlock), 0, (hipStream_t)stream, clusters, S, lo, m, f, slack, min_gap,
                     (uint64_t)cf, (uint64_t)total, rank0, ranks, count, L, x, flag);
  MATCHA_CHECK_LAUNCH("kway_complete_rows_kernel");
  return MATCHA_OK;
}

// ==== cluster decomposition ==========================================================================================
// Which sub-hyperedges of a cluster of up to 32 loci are real: the candidates are subsets of the cluster's OWN ids.  A cluster table is
// int64 [A, S], 2 <= S <= 32; row a holds s_a non-zero ids followed by zeros, only the leading run is read.  A choice is an m-subset of
// the positions [0, S), 1 <= m <= 8, ranked lexicographically from 0: C_m = C(S, m) <= C(32, 8) of them, so a choice's rank fits 32 bits;
// the global rank is g = a C_m + r.  keep (complement = 0, m >= 2): the row is the ids at the chosen positions; drop (complement = 1):
// the ids at all other positions; both in position order, zero-padded to L.  A candidate is valid iff every chosen position is < s_a,
// the row has at least 2 ids, the cluster's own ids are non-descending and every adjacent difference of the row is >= min_gap
// (unsigned, as in 7.10).  A chosen position >= s_a gives an all-zero row, flagged; every other invalid candidate keeps its row.
//
//   cluster_subset_rows_kernel    a wavefront serves 64 consecutive ranks.  Each lane divides and unranks ONE of them with the sweep's
//                                 unrank (m = S: the positions are the "region") and folds the positions into a 32-bit mask.  Then the
//                                 two 32-lane halves walk the 64 rows, one row each per step: the owner broadcasts its cluster index and
//                                 mask, lane j reads cluster id j, s_a is the first zero of a ballot.  A kept id goes to the column
//                                 popcount(kept mask below the lane); the lanes that keep nothing write the zero padding behind the row
//                                 (there are 32 - kept of them and at most L - kept pads): one store instruction per row, its lanes
//                                 covering one contiguous run of 8 L bytes.  The gap test compares every kept id with the previous KEPT
//                                 id, fetched by a shuffle from the highest set bit of the mask below the lane; one ballot per row.  No
//                                 LDS, no scratch.  Every shuffle and ballot is executed by all 64 lanes (predicated, never branched
//                                 around; the step count is the same for the whole wavefront).
//   subset_support_update_kernel  per cluster and position, the fixed-point sum (rint(double(v) 2^32), PairMap's) and the number of the
//                                 accepted rows whose choice contains the position; it unranks the choice itself and never reads a row.
//                                 A block serves runs of kSupRun consecutive ranks, hence of consecutive clusters: it accumulates into
//                                 an LDS tile of (clusters of the run) x S cells per plane with LDS integer atomics and issues one global
//                                 atomic per touched cell; clusters of the run beyond the tile go to global atomics directly.  Integer
//                                 atomics only: the state does not depend on arrival order or on how the stream is cut.
namespace matcha {
namespace {

constexpr int kSupRun = 2048;                  // consecutive ranks per block run: 8 rows per thread
constexpr int kSupTile = 1024;                 // cells per LDS plane (2 planes x 8 KB): 32 clusters of 32 ids, 341 of 3
constexpr size_t kSupHeader = 256;             // int64 n_rows, int64 n_rejected, padding

bool subset_args_ok(int64_t A, int32_t S, int32_t m, int32_t complement) {
  return A >= 0 && S >= 2 && S <= kMaxWide && (complement == 0 || complement == 1) && m >= (complement ? 1 : 2) && m <= kMaxK;
}

// A C(S, m), -1 for invalid arguments or a total >= 2^63; *cm_out = C(S, m)
int64_t subset_count(int64_t A, int32_t S, int32_t m, int32_t complement, int64_t* cm_out) {
  if (!subset_args_ok(A, S, m, complement)) return -1;
  const int64_t cm = count_subsets(S, m);      // <= C(32, 8)
  const unsigned __int128 total = (unsigned __int128)(uint64_t)A * (uint64_t)cm;
  if (total >= ((unsigned __int128)1 << 63)) return -1;
  if (cm_out) *cm_out = cm;
  return (int64_t)total;
}

// g = a cm + r; one 64-bit division only when the operands need it
__device__ __forceinline__ void split_rank(uint64_t g, uint64_t cm, uint64_t& a, uint64_t& r) {
  if ((g | cm) >> 32) {
    a = g / cm;
    r = g - a * cm;
  } else {
    const uint32_t a32 = (uint32_t)g / (uint32_t)cm;
    a = a32;
    r = (uint32_t)g - a32 * (uint32_t)cm;
  }
}

__global__ __launch_bounds__(kRowsPerBlock) void cluster_subset_rows_kernel(const int64_t* __restrict__ clusters, int32_t S, int32_t m, int32_t complement,
                                                                            int32_t min_gap, uint64_t cm, uint64_t total, int64_t rank0,
                                                                            const int64_t* __restrict__ ranks, int64_t count, int32_t L,
                                                                            int64_t* __restrict__ x, int32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31;
  const int64_t wave0 = (int64_t)(threadIdx.x >> 6) * 64;
  const uint64_t gap = (uint64_t)min_gap;
  const uint32_t below_me = (1u << j) - 1u;                            // j <= 31
  for (int64_t base = (int64_t)blockIdx.x * kRowsPerBlock; base < count; base += (int64_t)gridDim.x * kRowsPerBlock) {
    const int64_t w0 = base + wave0;                                   // the wavefront's first row; the same in all its lanes
    const int64_t left = count - w0;
    const int steps = left >= 64 ? 32 : left > 0 ? (int)((left + 1) >> 1) : 0;
    // ---- one rank per lane: cluster index and the choice as a mask of positions ----
    const int64_t i = w0 + lane;
    const int64_t g = i < count ? (ranks ? ranks[i] : rank0 + i) : -1;
    const int ok = g >= 0 && (uint64_t)g < total;                      // total > 0 then, so cm > 0 and m <= S
    uint64_t a = 0;
    uint32_t mask = 0;
    if (ok) {
      uint64_t r;
      split_rank((uint64_t)g, cm, a, r);
      int32_t y[kMaxK] = {0, 0, 0, 0, 0, 0, 0, 0};
      unrank(r, cm, S, m, y);
#pragma unroll
      for (int c = 0; c < kMaxK; ++c)
        if (c < m) mask |= 1u << (y[c] & 31);                          // y[c] < S <= 32
    }
    // ---- two rows per step, one per half ----
    int bad_mine = 1;
    for (int t = 0; t < steps; ++t) {
      const int own = 2 * t + h;                                       // the lane that unranked this half's row
      const int64_t irow = w0 + own;
      const int ok0 = __shfl(ok, 2 * t), ok1 = __shfl(ok, 2 * t + 1);
      const int ok_r = h ? ok1 : ok0;
      const uint64_t a_r = (uint64_t)shfl64((int64_t)a, own);
      const uint32_t mask_r = (uint32_t)__shfl((int)mask, own);
      int64_t v = 0;
      if (ok_r && j < S) v = clusters[a_r * (uint64_t)S + (uint64_t)j];
      const uint64_t zb = __ballot(v == 0);
      const uint32_t z0 = (uint32_t)zb, z1 = (uint32_t)(zb >> 32);
      const int s0 = z0 ? __builtin_ctz(z0) : 32, s1 = z1 ? __builtin_ctz(z1) : 32;   // S = 32 and no zero: all 32 lanes hold an id
      const int s = h ? s1 : s0;
      const uint32_t in_cluster = (uint32_t)((1ull << s) - 1ull);
      const bool outside = (mask_r & ~in_cluster) != 0;                // a chosen position >= s_a: an all-zero row
      uint32_t keep = complement ? (~mask_r & in_cluster) : mask_r;
      keep = (ok_r && !outside) ? keep : 0u;
      const bool kept = (keep >> j) & 1u;
      const uint32_t kb = keep & below_me;
      const int n_below = __popc(kb), n_kept = __popc(keep);
      // the cluster's own order: every id against its neighbour; the row's gaps: every kept id against the previous kept id
      const int64_t prev = shfl64(v, j ? lane - 1 : lane);
      const bool desc = j < s && j > 0 && v < prev;
      const int64_t prev_kept = shfl64(v, kb ? (h << 5) + 31 - __builtin_clz(kb) : lane);
      const bool close = kept && kb != 0 && (uint64_t)v - (uint64_t)prev_kept < gap;
      const uint64_t bb = __ballot(desc || close);
      const uint32_t out0 = (uint32_t)__shfl((int)outside, 0), out1 = (uint32_t)__shfl((int)outside, 32);
      const int nk0 = __shfl(n_kept, 0), nk1 = __shfl(n_kept, 32);
      const int bad0 = !ok0 || out0 || nk0 < 2 || (uint32_t)bb != 0, bad1 = !ok1 || out1 || nk1 < 2 || (uint32_t)(bb >> 32) != 0;
      if (lane == 2 * t) bad_mine = bad0;
      if (lane == 2 * t + 1) bad_mine = bad1;
      const int col = kept ? n_below : n_kept + (j - n_below);         // the lanes that keep nothing write the pads behind the row
      const int64_t val = kept ? v : 0;
      if (irow < count && col < L) x[irow * L + col] = val;
    }
    if (i < count) flag[i] = bad_mine;
  }
}

struct SupportPlan {
  size_t off_sum, off_count, total;
  int64_t cells;
};

bool support_args_ok(int64_t A, int32_t S, int32_t m, float vmax) {
  return A >= 1 && A <= ((int64_t)1 << 40) && S >= 2 && S <= kMaxWide && m >= 1 && m <= kMaxK && vmax > 0.f && vmax <= 1048576.f;   // NaN fails
}

SupportPlan make_splan(int64_t A, int32_t S) {
  SupportPlan pl{};
  pl.cells = A * S;
  pl.off_sum = kSupHeader;
  pl.off_count = pl.off_sum + align_up((size_t)pl.cells * 8, 256);
  pl.total = pl.off_count + align_up((size_t)pl.cells * 8, 256);
  return pl;
}

__global__ __launch_bounds__(256) void subset_support_init_kernel(unsigned long long* __restrict__ p, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) p[i] = 0ull;
}

// Every lane of a wavefront runs the whole body: the trip counts depend on the block's run only, the ballots read all 64 lanes.
__global__ __launch_bounds__(256) void subset_support_update_kernel(unsigned long long* __restrict__ counters, unsigned long long* __restrict__ sum,
                                                                    unsigned long long* __restrict__ cnt, int32_t S, int32_t m, uint64_t cm, float vmax,
                                                                    const float* __restrict__ value, const int32_t* __restrict__ skip, int64_t n,
                                                                    int64_t g0) {
  __shared__ unsigned long long tsum[kSupTile], tcnt[kSupTile];
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t tile_clusters = (uint64_t)(kSupTile / S);              // >= 32
  uint32_t n_rows = 0, n_rej = 0;                                       // this wavefront's totals (identical in every lane)
  const int64_t runs = (n + kSupRun - 1) / kSupRun;
  for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
    const int64_t i0 = run * kSupRun;
    const int len = n - i0 < kSupRun ? (int)(n - i0) : kSupRun;
    const uint64_t a_first = (uint64_t)(g0 + i0) / cm, a_last = (uint64_t)(g0 + i0 + len - 1) / cm;
    const uint64_t span = a_last - a_first + 1 < tile_clusters ? a_last - a_first + 1 : tile_clusters;
    const int cells = (int)span * S;                                    // <= kSupTile
    for (int e = threadIdx.x; e < cells; e += 256) { tsum[e] = 0ull; tcnt[e] = 0ull; }
    __syncthreads();
    for (int off = 0; off < len; off += 256) {
      const int at = off + (int)threadIdx.x;
      float v = 0.f;
      bool live = false, rejected = false;
      if (at < len) {
        const bool skipped = skip && skip[i0 + at] != 0;
        v = value[i0 + at];
        const bool okv = v >= 0.f && v <= vmax;                         // false for NaN
        live = !skipped && okv;
        rejected = !skipped && !okv;
      }
      n_rows += (uint32_t)__popcll(__ballot(live));
      n_rej += (uint32_t)__popcll(__ballot(rejected));
      if (live) {
        v = v + 0.f;                                                    // -0.0 -> +0.0
        const unsigned long long q = (unsigned long long)__double2ll_rn((double)v * 4294967296.0);
        uint64_t a, r;
        split_rank((uint64_t)(g0 + i0 + at), cm, a, r);
        int32_t y[kMaxK] = {0, 0, 0, 0, 0, 0, 0, 0};
        unrank(r, cm, S, m, y);
        const uint64_t rel = a - a_first;
        const bool tiled = rel < span;
#pragma unroll
        for (int c = 0; c < kMaxK; ++c) {
          if (c < m) {
            if (tiled) {
              const int e = (int)rel * S + y[c];                        // < span S
              atomicAdd(&tsum[e], q);
              atomicAdd(&tcnt[e], 1ull);
            } else {
              const uint64_t e = a * (uint64_t)S + (uint64_t)y[c];      // a < A: the host checked g0 + n <= A cm
              atomicAdd(sum + e, q);
              atomicAdd(cnt + e, 1ull);
            }
          }
        }
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += 256) {
      const unsigned long long c = tcnt[e];
      if (c) {
        atomicAdd(sum + a_first * (uint64_t)S + (uint64_t)e, tsum[e]);
        atomicAdd(cnt + a_first * (uint64_t)S + (uint64_t)e, c);
      }
    }
    __syncthreads();                                                    // the tile is reused by the next run
  }
  if (lane == 0) {
    if (n_rows) atomicAdd(counters, (unsigned long long)n_rows);
    if (n_rej) atomicAdd(counters + 1, (unsigned long long)n_rej);
  }
}

__global__ __launch_bounds__(256) void subset_support_read_kernel(const unsigned long long* __restrict__ counters, const unsigned long long* __restrict__ sum,
                                                                  const unsigned long long* __restrict__ cnt, int64_t cells, int64_t* __restrict__ sum_out,
                                                                  int64_t* __restrict__ count_out, int64_t* __restrict__ counters_out) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < cells; p += (int64_t)gridDim.x * 256) {
    if (sum_out) sum_out[p] = (int64_t)sum[p];
    if (count_out) count_out[p] = (int64_t)cnt[p];
  }
  if (counters_out && blockIdx.x == 0 && threadIdx.x < 2) counters_out[threadIdx.x] = (int64_t)counters[threadIdx.x];
}

// ---- per-pair support ----
// Per cluster and PAIR of positions i < j, the same two quantities over the accepted rows whose choice contains both: two planes of
// A P cells, P = S (S - 1) / 2, the upper triangle packed row-major: cell a P + i (2 S - i - 1) / 2 + (j - i - 1).
//   subset_pair_update_kernel  the support kernel's structure and row handling; an accepted row adds to the C(m, 2) <= 28 cells of its
//                              choice.  m = 2: the choice IS one pair and its lexicographic rank is the packed index, so the row's
//                              cell is its global rank g -- no unranking, no tile, one coalesced global atomic per plane.  m >= 3: a
//                              block's run of kPairRun consecutive ranks accumulates into an LDS tile of kPairTile cells per plane
//                              (uint64 sums; uint32 counts, a run adds at most kPairRun to a cell) and flushes one global atomic per
//                              touched cell; clusters of the run beyond the tile (only where C(S, m) <= P: m >= S - 2) go to global
//                              atomics directly.  Sizes: 2 048 cells are 16 KB + 8 KB = 24 KB of LDS per block, six blocks (24 of
//                              32 wavefronts) per CU of 160 KB, and hold 4 clusters of 32 loci (496 cells), 56 of 9; a run of 2 048
//                              ranks is 8 rows per thread, as in the support kernel.  Integer atomics only.
constexpr int kPairRun = 2048;
constexpr int kPairTile = 2048;

struct PairPlan {
  size_t off_sum, off_count, total;
  int64_t cells;
  int32_t P;
};

bool pair_args_ok(int64_t A, int32_t S, int32_t m, float vmax) { return support_args_ok(A, S, m, vmax) && m >= 2; }

PairPlan make_pplan(int64_t A, int32_t S) {
  PairPlan pl{};
  pl.P = S * (S - 1) / 2;                                               // <= 496
  pl.cells = A * pl.P;                                                  // < 2^49
  pl.off_sum = kSupHeader;
  pl.off_count = pl.off_sum + align_up((size_t)pl.cells * 8, 256);
  pl.total = pl.off_count + align_up((size_t)pl.cells * 8, 256);
  return pl;
}

__global__ __launch_bounds__(256) void subset_pair_init_kernel(unsigned long long* __restrict__ p, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) p[i] = 0ull;
}

// Every lane of a wavefront runs the whole body: the trip counts depend on the block's run only (m is the launch's), the ballots read
// all 64 lanes and every barrier is reached by all four wavefronts.
__global__ __launch_bounds__(256) void subset_pair_update_kernel(unsigned long long* __restrict__ counters, unsigned long long* __restrict__ sum,
                                                                 unsigned long long* __restrict__ cnt, int32_t S, int32_t P, int32_t m, uint64_t cm,
                                                                 float vmax, const float* __restrict__ value, const int32_t* __restrict__ skip, int64_t n,
                                                                 int64_t g0) {
  __shared__ unsigned long long tsum[kPairTile];
  __shared__ unsigned int tcnt[kPairTile];
  const int lane = threadIdx.x & (kWave - 1);
  const bool direct = m == 2;                                           // cm == P and the choice's rank is its cell
  const uint64_t tile_clusters = (uint64_t)(kPairTile / P);             // >= 4
  uint32_t n_rows = 0, n_rej = 0;                                       // this wavefront's totals (identical in every lane)
  const int64_t runs = (n + kPairRun - 1) / kPairRun;
  for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
    const int64_t i0 = run * kPairRun;
    const int len = n - i0 < kPairRun ? (int)(n - i0) : kPairRun;
    const uint64_t a_first = (uint64_t)(g0 + i0) / cm, a_last = (uint64_t)(g0 + i0 + len - 1) / cm;
    const uint64_t span = a_last - a_first + 1 < tile_clusters ? a_last - a_first + 1 : tile_clusters;
    const int cells = direct ? 0 : (int)span * P;                       // <= kPairTile
    for (int e = threadIdx.x; e < cells; e += 256) { tsum[e] = 0ull; tcnt[e] = 0u; }
    __syncthreads();
    for (int off = 0; off < len; off += 256) {
      const int at = off + (int)threadIdx.x;
      float v = 0.f;
      bool live = false, rejected = false;
      if (at < len) {
        const bool skipped = skip && skip[i0 + at] != 0;
        v = value[i0 + at];
        const bool okv = v >= 0.f && v <= vmax;                         // false for NaN
        live = !skipped && okv;
        rejected = !skipped && !okv;
      }
      n_rows += (uint32_t)__popcll(__ballot(live));
      n_rej += (uint32_t)__popcll(__ballot(rejected));
      if (live) {
        v = v + 0.f;                                                    // -0.0 -> +0.0
        const unsigned long long q = (unsigned long long)__double2ll_rn((double)v * 4294967296.0);
        if (direct) {
          const uint64_t e = (uint64_t)(g0 + i0 + at);                  // < A cm = A P: the host checked g0 + n <= A cm
          atomicAdd(sum + e, q);
          atomicAdd(cnt + e, 1ull);
        } else {
          uint64_t a, r;
          split_rank((uint64_t)(g0 + i0 + at), cm, a, r);
          int32_t y[kMaxK] = {0, 0, 0, 0, 0, 0, 0, 0};
          unrank(r, cm, S, m, y);                                       // ascending, every y[c] < S for c < m
          const uint64_t rel = a - a_first;
          const bool tiled = rel < span;
          const int tbase = tiled ? (int)rel * P : 0;
          const uint64_t gbase = a * (uint64_t)P;                       // a < A
#pragma unroll
          for (int c = 0; c < kMaxK - 1; ++c) {
            const int row = y[c] * (2 * S - y[c] - 1) / 2 - y[c] - 1;   // + j: the cell of (y[c], j), j > y[c]
#pragma unroll
            for (int d = c + 1; d < kMaxK; ++d) {
              if (d < m) {
                const int e = row + y[d];                               // in [0, P)
                if (tiled) {
                  atomicAdd(&tsum[tbase + e], q);                       // tbase + e < span P
                  atomicAdd(&tcnt[tbase + e], 1u);
                } else {
                  atomicAdd(sum + gbase + (uint64_t)e, q);
                  atomicAdd(cnt + gbase + (uint64_t)e, 1ull);
                }
              }
            }
          }
        }
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < cells; e += 256) {
      const unsigned int c = tcnt[e];
      if (c) {
        atomicAdd(sum + a_first * (uint64_t)P + (uint64_t)e, tsum[e]);
        atomicAdd(cnt + a_first * (uint64_t)P + (uint64_t)e, (unsigned long long)c);
      }
    }
    __syncthreads();                                                    // the tile is reused by the next run
  }
  if (lane == 0) {
    if (n_rows) atomicAdd(counters, (unsigned long long)n_rows);
    if (n_rej) atomicAdd(counters + 1, (unsigned long long)n_rej);
  }
}

__global__ __launch_bounds__(256) void subset_pair_read_kernel(const unsigned long long* __restrict__ counters, const unsigned long long* __restrict__ sum,
                                                               const unsigned long long* __restrict__ cnt, int64_t cells, int64_t* __restrict__ sum_out,
                                                               int64_t* __restrict__ count_out, int64_t* __restrict__ counters_out) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < cells; p += (int64_t)gridDim.x * 256) {
    if (sum_out) sum_out[p] = (int64_t)sum[p];
    if (count_out) count_out[p] = (int64_t)cnt[p];
  }
  if (counters_out && blockIdx.x == 0 && threadIdx.x < 2) counters_out[threadIdx.x] = (int64_t)counters[threadIdx.x];
}

}  // namespace
}  // namespace matcha

extern "C" int64_t matcha_cluster_subset_count(int64_t A, int32_t S, int32_t m, int32_t complement) { return subset_count(A, S, m, complement, nullptr); }

extern "C" int matcha_cluster_subset_rows(const int64_t* clusters, int64_t A, int32_t S, int32_t m, int32_t complement, int32_t min_gap, int64_t rank0,
                                          const int64_t* ranks, int64_t count, int32_t L, int64_t* x, int32_t* flag, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(subset_args_ok(A, S, m, complement),
                   "matcha_cluster_subset_rows: need A >= 0, 2 <= S <= %d, complement 0 (keep, 2 <= m <= %d) or 1 (drop, 1 <= m <= %d) "
                   "(A=%lld S=%d m=%d complement=%d)", kMaxWide, kMaxK, kMaxK, (long long)A, S, m, complement);
  MATCHA_CHECK_ARG(min_gap >= 1, "matcha_cluster_subset_rows: min_gap=%d must be >= 1", min_gap);
  const int32_t l_min = complement ? (S - m > 1 ? S - m : 1) : m;
  MATCHA_CHECK_ARG(L >= l_min && L <= kMaxWide, "matcha_cluster_subset_rows: row width L=%d must be in [%d, %d] (keep: m, drop: S - m)", L, l_min, kMaxWide);
  int64_t cm = 0;
  const int64_t total = subset_count(A, S, m, complement, &cm);
  MATCHA_CHECK_ARG(total >= 0, "matcha_cluster_subset_rows: A C(S, m) does not fit 63 bits (A=%lld S=%d m=%d)", (long long)A, S, m);
  MATCHA_CHECK_ARG(count >= 0 && count <= ((int64_t)1 << 40), "matcha_cluster_subset_rows: count out of range");
  if (!ranks)
    MATCHA_CHECK_ARG(rank0 >= 0 && rank0 <= total && count <= total - rank0,
                     "matcha_cluster_subset_rows: %lld ranks from %lld lie outside [0, %lld)", (long long)count, (long long)rank0, (long long)total);
  if (count == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(x && flag, "matcha_cluster_subset_rows: null output");
  MATCHA_CHECK_ARG(clusters || total == 0, "matcha_cluster_subset_rows: null clusters");
  int64_t blocks = cdiv(count, kRowsPerBlock);
  if (blocks > (1 << 20)) blocks = 1 << 20;
  hipLaunchKernelGGL(cluster_subset_rows_kernel, dim3((unsigned)blocks), dim3(kRowsPerBlock), 0, (hipStream_t)stream, clusters, S, m, complement, min_gap,
                     (uint64_t)cm, (uint64_t)total, rank0, ranks, count, L, x, flag);
  MATCHA_CHECK_LAUNCH("cluster_subset_rows_kernel");
  return MATCHA_OK;
}

extern "C" size_t matcha_subset_support_bytes(int64_t A, int32_t S, int32_t m, float vmax) {
  if (!support_args_ok(A, S, m, vmax)) return 0;
  return make_splan(A, S).total;
}

#define SUPPORT_COMMON_ARGS(fn)                                                                                                     \
  MATCHA_CHECK_ARG(state, fn ": null state");                                                                                       \
  MATCHA_CHECK_ARG(support_args_ok(A, S, m, vmax), fn ": need 1 <= A <= 2^40, 2 <= S <= %d, 1 <= m <= %d, 0 < vmax <= 2^20 "        \
                                                      "(A=%lld S=%d m=%d vmax=%g)",                                                 \
                   kMaxWide, kMaxK, (long long)A, S, m, (double)vmax);                                                              \
  MATCHA_CHECK_ARG(((uintptr_t)state) % 8 == 0, fn ": state must be 8-byte aligned");                                               \
  const SupportPlan pl = make_splan(A, S);                                                                                          \
  MATCHA_CHECK_ARG(bytes >= pl.total, fn ": state too small (%zu bytes, matcha_subset_support_bytes says %zu)", bytes, pl.total)

extern "C" int matcha_subset_support_init(void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, matcha_stream_t stream) {
  SUPPORT_COMMON_ARGS("matcha_subset_support_init");
  const int64_t n8 = (int64_t)(pl.total / 8);                            // every offset is a multiple of 256
  int64_t blocks = cdiv(n8, 256);
  if (blocks > (1 << 14)) blocks = 1 << 14;
  hipLaunchKernelGGL(subset_support_init_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)state, n8);
  MATCHA_CHECK_LAUNCH("subset_support_init_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_subset_support_update(void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, const float* value,
                                            const int32_t* skip, int64_t n, int64_t g0, matcha_stream_t stream) {
  SUPPORT_COMMON_ARGS("matcha_subset_support_update");
  const int64_t cm = count_subsets(S, m);
  const int64_t total = A * cm;                                          // < 2^40 * 2^24
  MATCHA_CHECK_ARG(n >= 0 && n <= ((int64_t)1 << 40), "matcha_subset_support_update: n=%lld out of range", (long long)n);
  MATCHA_CHECK_ARG(g0 >= 0 && g0 <= total && n <= total - g0, "matcha_subset_support_update: %lld ranks from %lld lie outside [0, %lld)", (long long)n,
                   (long long)g0, (long long)total);
  if (n == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(value, "matcha_subset_support_update: null value");
  char* w = (char*)state;
  int64_t blocks = cdiv(n, kSupRun);
  if (blocks > (1 << 14)) blocks = 1 << 14;
  hipLaunchKernelGGL(subset_support_update_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)w,
                     (unsigned long long*)(w + pl.off_sum), (unsigned long long*)(w + pl.off_count), S, m, (uint64_t)cm, vmax, value, skip, n, g0);
  MATCHA_CHECK_LAUNCH("subset_support_update_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_subset_support_read(const void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, int64_t* sum_out,
                                          int64_t* count_out, int64_t* counters_out, matcha_stream_t stream) {
  SUPPORT_COMMON_ARGS("matcha_subset_support_read");
  MATCHA_CHECK_ARG(sum_out || count_out || counters_out, "matcha_subset_support_read: null output");
  const char* w = (const char*)state;
  int64_t blocks = cdiv(pl.cells, 256);
  if (blocks > (1 << 14)) blocks = 1 << 14;
  hipLaunchKernelGGL(subset_support_read_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)w,
                     (const unsigned long long*)(w + pl.off_sum), (const unsigned long long*)(w + pl.off_count), pl.cells, sum_out, count_out,
                     counters_out);
  MATCHA_CHECK_LAUNCH("subset_support_read_kernel");
  return MATCHA_OK;
}

extern "C" size_t matcha_subset_pair_bytes(int64_t A, int32_t S, int32_t m, float vmax) {
  if (!pair_args_ok(A, S, m, vmax)) return 0;
  return make_pplan(A, S).total;
}

#define PAIR_COMMON_ARGS(fn)                                                                                                        \
  MATCHA_CHECK_ARG(state, fn ": null state");                                                                                       \
  MATCHA_CHECK_ARG(pair_args_ok(A, S, m, vmax), fn ": need 1 <= A <= 2^40, 2 <= S <= %d, 2 <= m <= %d, 0 < vmax <= 2^20 "           \
                                                   "(A=%lld S=%d m=%d vmax=%g)",                                                    \
                   kMaxWide, kMaxK, (long long)A, S, m, (double)vmax);                                                              \
  MATCHA_CHECK_ARG(((uintptr_t)state) % 8 == 0, fn ": state must be 8-byte aligned");                                               \
  const PairPlan pl = make_pplan(A, S);                                                                                             \
  MATCHA_CHECK_ARG(bytes >= pl.total, fn ": state too small (%zu bytes, matcha_subset_pair_bytes says %zu)", bytes, pl.total)

extern "C" int matcha_subset_pair_init(void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, matcha_stream_t stream) {
  PAIR_COMMON_ARGS("matcha_subset_pair_init");
  const int64_t n8 = (int64_t)(pl.total / 8);                            // every offset is a multiple of 256
  int64_t blocks = cdiv(n8, 256);
  if (blocks > (1 << 14)) blocks = 1 << 14;
  hipLaunchKernelGGL(subset_pair_init_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)state, n8);
  MATCHA_CHECK_LAUNCH("subset_pair_init_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_subset_pair_update(void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, const float* value,
                                         const int32_t* skip, int64_t n, int64_t g0, matcha_stream_t stream) {
  PAIR_COMMON_ARGS("matcha_subset_pair_update");
  const int64_t cm = count_subsets(S, m);
  const int64_t total = A * cm;                                          // < 2^40 * 2^24
  MATCHA_CHECK_ARG(n >= 0 && n <= ((int64_t)1 << 40), "matcha_subset_pair_update: n=%lld out of range", (long long)n);
  MATCHA_CHECK_ARG(g0 >= 0 && g0 <= total && n <= total - g0, "matcha_subset_pair_update: %lld ranks from %lld lie outside [0, %lld)", (long long)n,
                   (long long)g0, (long long)total);
  if (n == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(value, "matcha_subset_pair_update: null value");
  char* w = (char*)state;
  int64_t blocks = cdiv(n, kPairRun);
  if (blocks > (1 << 14)) blocks = 1 << 14;
  hipLaunchKernelGGL(subset_pair_update_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (unsigned long long*)w,
                     (unsigned long long*)(w + pl.off_sum), (unsigned long long*)(w + pl.off_count), S, pl.P, m, (uint64_t)cm, vmax, value, skip, n, g0);
  MATCHA_CHECK_LAUNCH("subset_pair_update_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_subset_pair_read(const void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, int64_t* sum_out,
                                       int64_t* count_out, int64_t* counters_out, matcha_stream_t stream) {
  PAIR_COMMON_ARGS("matcha_subset_pair_read");
  MATCHA_CHECK_ARG(sum_out || count_out || counters_out, "matcha_subset_pair_read: null output");
  const char* w = (const char*)state;
  int64_t blocks = cdiv(pl.cells, 256);
  if (blocks > (1 << 14)) blocks = 1 << 14;
  hipLaunchKernelGGL(subset_pair_read_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)w,
                     (const unsigned long long*)(w + pl.off_sum), (const unsigned long long*)(w + pl.off_count), pl.cells, sum_out, count_out,
                     counters_out);
  MATCHA_CHECK_LAUNCH("subset_pair_read_kernel");
  return MATCHA_OK;
}

// ==== multi-region sweep ===============================================================================================
// Candidates whose bins come from several regions: P parts, 1 <= P <= 8; part p is a region [lo_p, lo_p + n_p) and a number m_p >= 1 of
// bins drawn from it, k = sum m_p in [2, 8].  The regions are ascending and disjoint, so the concatenation, part by part, of one 7.3
// candidate of every part is an ascending row as it stands.  Part p has C_p = C(n_p - (m_p - 1)(min_gap - 1), m_p) candidates, ranked r_p
// as kway_rows_kernel ranks them; the global rank is the mixed radix g = ((r_0 C_1 + r_1) C_2 + ...) C_{P-1} + r_{P-1}, 0 <= g < T = prod
// C_p < 2^63: rank order is the lexicographic order of the rows.  The gap rule holds inside every part by construction; across a part
// boundary (two regions closer than min_gap) it may fail, and such a candidate keeps its rank and its row with its flag set.
//
//   kway_region_rows_kernel   one thread per row.  The rank is decoded from the last part backwards, one division per part (none for
//                             part 0), 32-bit when the rest of the rank and the radix both fit.  A part of one bin is lo_p + r_p; any
//                             other goes through unrank.  A part's ids go straight into the row's slice of the LDS tile at the part's
//                             column offset (an LDS address, not an index into a register array); the boundary test uses the part's
//                             last id and the next part's first id while both are in registers.  The loop over parts is unrolled to 8
//                             and predicated on p < P; the parts travel by value in one kernel argument, indexed statically.  The tile
//                             leaves as the coalesced copy of the other rows kernels.  No atomics, no scratch.
namespace matcha {
namespace {

constexpr int kMaxParts = 8;

struct RegionParts {
  int64_t lo[kMaxParts];      // first node id of the region
  uint64_t C[kMaxParts];      // candidates of the part (the radix)
  int32_t M[kMaxParts];       // n_p - (m_p - 1)(min_gap - 1), clamped at 0: the part's candidates are the m_p-subsets of [0, M_p)
  int32_t m[kMaxParts];       // bins drawn from the part
  int32_t P;
};

// T, -1 for invalid arguments or T >= 2^63; *k_out = sum m_p, parts filled when given
int64_t region_count(int32_t P, const int64_t* lo, const int32_t* n, const int32_t* m, int32_t min_gap, RegionParts* parts, int32_t* k_out) {
  if (P < 1 || P > kMaxParts || !lo || !n || !m || min_gap < 1) return -1;
  int64_t k = 0;
  for (int p = 0; p < P; ++p) {
    if (m[p] < 1 || n[p] < 1 || lo[p] < 0 || lo[p] > ((int64_t)1 << 62)) return -1;
    if (p > 0 && lo[p - 1] + (int64_t)n[p - 1] > lo[p]) return -1;
    k += m[p];
  }
  if (k < 2 || k > kMaxK) return -1;
  unsigned __int128 total = 1;
  bool empty = false;
  for (int p = 0; p < P; ++p) {
    const int64_t M = (int64_t)n[p] - (int64_t)(m[p] - 1) * (min_gap - 1);
    const int64_t c = count_subsets(M, m[p]);
    if (c < 0) return -1;
    empty |= c == 0;
    if (!empty) {
      total *= (unsigned __int128)(uint64_t)c;
      if (total >= ((unsigned __int128)1 << 63)) return -1;
    }
    if (parts) {
      parts->lo[p] = lo[p];
      parts->C[p] = (uint64_t)c;
      parts->M[p] = M > 0 ? (int32_t)M : 0;
      parts->m[p] = m[p];
    }
  }
  if (k_out) *k_out = (int32_t)k;
  return empty ? 0 : (int64_t)total;
}

__global__ __launch_bounds__(kRowsPerBlock) void kway_region_rows_kernel(RegionParts parts, int32_t k, int32_t slack, int32_t min_gap, uint64_t total,
                                                                         int64_t rank0, const int64_t* __restrict__ ranks, int64_t count, int32_t L,
                                                                         int64_t* __restrict__ x, int32_t* __restrict__ flag) {
  __shared__ int64_t tile[kRowsPerBlock * kMaxK];
  for (int64_t base = (int64_t)blockIdx.x * kRowsPerBlock; base < count; base += (int64_t)gridDim.x * kRowsPerBlock) {
    const int64_t i = base + threadIdx.x;
    if (i < count) {
      const int64_t g = ranks ? ranks[i] : rank0 + i;
      const bool ok = g >= 0 && (uint64_t)g < total;                   // total > 0 then, so every C_p > 0
      int64_t* __restrict__ row = tile + threadIdx.x * L;
#pragma unroll
      for (int c = 0; c < kMaxK; ++c)
        if (c < L && (!ok || c >= k)) row[c] = 0;
      bool bad = !ok;
      if (ok) {
        uint64_t rest = (uint64_t)g;
        int col = k;                                                   // one past the part's last column
        int64_t next_first = 0;                                        // first id of part p + 1
#pragma unroll
        for (int p = kMaxParts - 1; p >= 0; --p) {
          if (p < parts.P) {
            const uint64_t cp = parts.C[p];
            const int mp = parts.m[p];
            uint64_t r;
            if (p == 0) {
              r = rest;                                                // rest < C_0: nothing left to divide
            } else if ((rest | cp) >> 32) {                            // the part's one 64-bit division
              const uint64_t q = rest / cp;
              r = rest - q * cp;
              rest = q;
            } else {
              const uint32_t q32 = (uint32_t)rest / (uint32_t)cp;
              r = (uint32_t)rest - q32 * (uint32_t)cp;
              rest = q32;
            }
            col -= mp;
            int64_t first, last;
            if (mp == 1) {
              first = last = parts.lo[p] + (int64_t)r;
              row[col] = first;
            } else {
              int32_t y[kMaxK] = {0, 0, 0, 0, 0, 0, 0, 0};
              unrank(r, cp, parts.M[p], mp, y);
              first = last = parts.lo[p] + (int64_t)y[0];
#pragma unroll
              for (int c = 0; c < kMaxK; ++c) {
                if (c < mp) {
                  const int64_t v = parts.lo[p] + (int64_t)y[c] + (int64_t)c * slack;
                  row[col + c] = v;
                  last = v;
                }
              }
            }
            if (p + 1 < parts.P) bad |= next_first - last < (int64_t)min_gap;      // regions ascend: the difference is positive
            next_first = first;
          }
        }
      }
      flag[i] = bad ? 1 : 0;
    }
    __syncthreads();
    const int64_t rows = count - base < kRowsPerBlock ? count - base : kRowsPerBlock;
    const int elems = (int)rows * L;
    for (int e = threadIdx.x; e < elems; e += kRowsPerBlock) x[base * L + e] = tile[e];
    __syncthreads();                                                   // the tile is reused by the next run of rows
  }
}

}  // namespace
}  // namespace matcha

extern "C" int64_t matcha_kway_region_count(int32_t P, const int64_t* lo, const int32_t* n, const int32_t* m, int32_t min_gap) {
  return region_count(P, lo, n, m, min_gap, nullptr, nullptr);
}

extern "C" int matcha_kway_region_rows(int32_t P, const int64_t* lo, const int32_t* n, const int32_t* m, int32_t min_gap, int64_t rank0,
                                       const int64_t* ranks, int64_t count, int32_t L, int64_t* x, int32_t* flag, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(P >= 1 && P <= kMaxParts, "matcha_kway_region_rows: need 1 <= P <= %d parts (P=%d)", kMaxParts, P);
  MATCHA_CHECK_ARG(lo && n && m, "matcha_kway_region_rows: null part arrays");
  MATCHA_CHECK_ARG(min_gap >= 1, "matcha_kway_region_rows: need min_gap >= 1 (min_gap=%d)", min_gap);
  int64_t k = 0;
  for (int p = 0; p < P; ++p) {
    MATCHA_CHECK_ARG(m[p] >= 1 && n[p] >= 1, "matcha_kway_region_rows: part %d needs n >= 1 bins and m >= 1 drawn (n=%d m=%d)", p, n[p], m[p]);
    MATCHA_CHECK_ARG(lo[p] >= 0 && lo[p] <= ((int64_t)1 << 62), "matcha_kway_region_rows: lo of part %d out of range", p);
    MATCHA_CHECK_ARG(p == 0 || lo[p - 1] + (int64_t)n[p - 1] <= lo[p],
                     "matcha_kway_region_rows: the regions must be ascending and disjoint (part %d begins at %lld, part %d ends at %lld)", p,
                     (long long)lo[p], p - 1, (long long)(lo[p - 1] + (int64_t)n[p - 1]));
    k += m[p];
  }
  MATCHA_CHECK_ARG(k >= 2 && k <= kMaxK, "matcha_kway_region_rows: need 2 <= k <= %d bins per candidate (k=%lld)", kMaxK, (long long)k);
  MATCHA_CHECK_ARG(L >= k && L <= kMaxK, "matcha_kway_region_rows: row width L=%d must be in [k, %d]", L, kMaxK);
  RegionParts parts = {};
  parts.P = P;
  const int64_t total = region_count(P, lo, n, m, min_gap, &parts, nullptr);
  MATCHA_CHECK_ARG(total >= 0, "matcha_kway_region_rows: the product of the parts' counts does not fit 63 bits (P=%d k=%lld min_gap=%d)", P, (long long)k,
                   min_gap);
  MATCHA_CHECK_ARG(count >= 0 && count <= ((int64_t)1 << 40), "matcha_kway_region_rows: count out of range");
  if (!ranks)
    MATCHA_CHECK_ARG(rank0 >= 0 && rank0 <= total && count <= total - rank0,
                     "matcha_kway_region_rows: %lld ranks from %lld lie outside [0, %lld)", (long long)count, (long long)rank0, (long long)total);
  if (count == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(x && flag, "matcha_kway_region_rows: null output");
  int64_t blocks = cdiv(count, kRowsPerBlock);
  if (blocks > (1 << 20)) blocks = 1 << 20;
  hipLaunchKernelGGL(kway_region_rows_kernel, dim3((unsigned)blocks), dim3(kRowsPerBlock), 0, (hipStream_t)stream, parts, (int32_t)k, min_gap - 1, min_gap,
                     (uint64_t)total, rank0, ranks, count, L, x, flag);
  MATCHA_CHECK_LAUNCH("kway_region_rows_kernel");
  return MATCHA_OK;
}
