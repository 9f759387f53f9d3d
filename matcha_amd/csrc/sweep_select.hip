// The streaming selection of the sweeps: the best K (score, rank) pairs of every segment of seg_len consecutive
// global ranks, kept across chunks without the scores ever leaving the device.  matcha_segtopk_* is the selection itself (the anchored
// sweep: seg_len = C_f, segment = anchor); matcha_topk_* is the same selection with ONE segment that holds every rank, a state of K slots
// and 32-bit sort keys.  A chunk may cover a fraction of one segment or thousands of them.
//
// The total order is: higher score first (IEEE comparison: -0.0 == +0.0, +inf highest, -inf lowest), then lower rank; NaN scores and rows
// with skip[i] != 0 are never kept.  The state is, per segment, the K best pairs so far, sorted, padded with sentinels.
//
//   select_init_kernel     fills the state with sentinels (no memset): all A K slots.
//   topk_keys_kernel       score -> 32-bit key that sorts ascending in the order above (-0.0 folded onto +0.0 in the key only; the stored
//                          score keeps its bits), invalid rows -> the sentinel key; value = the row's index in the chunk.
//   segtopk_keys_kernel    64-bit key = (segment index within the chunk) << 32 | score key; value = the row's index in the chunk.
//   rocPRIM radix sort of (key, index) over the bits in use: stable, and the chunk's ranks ascend with the index, so every row stays in
//                          its segment's group in the total order (sentinel rows last), and the sorted run of chunk segment t begins at
//                          max(0, t seg_len - off0), known by arithmetic.
//   select_merge_kernel    one thread per (touched segment, position p < K): merge path over the segment's sorted state and the best
//                          min(K, run length) rows of its run: output position p finds its split by a binary search on the composite
//                          (key, rank) and takes one element.  Templated on the sorted key's type.
//   select_commit_kernel   copies the merged rows of the touched segments (a contiguous range of the state) back.
//   select_read_kernel     scores, ranks and per-segment counts of valid pairs (the first sentinel's position).
//
// The launch log names these kernels by the entry that ran them, topk_*_kernel under matcha_topk_* and segtopk_*_kernel under
// matcha_segtopk_*: the tests assert which selection a sweep ran.
//
// No atomics of any kind: every output element has one owner, so the state after a sequence of updates depends only on the multiset of
// (score, rank) pairs seen -- not on how the stream was cut, and not on timing.  Segments a chunk does not touch are neither read nor
// written.
#include <hip/hip_runtime.h>

#include <cstdint>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.hpp"

namespace matcha {
namespace {

constexpr uint32_t kSentinel = 0xFFFFFFFFu;    // sorts behind every real key (the worst real key is -inf: 0xFF800000)

#define SELECT_KERNEL_NAME(seg, stem) ((seg) ? "segtopk_" stem "_kernel" : "topk_" stem "_kernel")

__device__ __forceinline__ uint32_t score_key(float s) {
  if (s != s) return kSentinel;
  uint32_t b = __builtin_bit_cast(uint32_t, s);
  if (b == 0x80000000u) b = 0;                                         // -0.0 == +0.0: one key, the rank decides
  const uint32_t asc = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ~asc;                                                         // ascending key = descending score
}

struct SelectPlan {
  size_t off_key, off_score, off_rank;        // the state: A segments of K sorted pairs
  size_t off_tkey, off_tscore, off_trank;     // the merged rows of the touched segments before they are committed
  size_t off_ckey, off_cidx, off_skey, off_sidx, off_sort, sort_bytes, total;
  int64_t tmax;                               // the most segments one update can touch
};

bool topk_args_ok(int64_t K, int64_t max_chunk) {
  return K >= 1 && K <= ((int64_t)1 << 31) - 1 && max_chunk >= 1 && max_chunk <= ((int64_t)1 << 31) - 1;
}

bool seg_args_ok(int64_t A, int64_t K, int64_t seg_len, int64_t max_chunk) {
  const int64_t lim = ((int64_t)1 << 31) - 1;
  return K >= 1 && K <= lim && A >= 1 && A <= lim / K && seg_len >= 1 && max_chunk >= 1 && max_chunk <= lim;
}

// The radix sort's scratch is reserved by a bound (two buffers of keys and of 32-bit values plus its histograms and look-back state), not
// by asking rocPRIM: sizing must work where there is no device.  select_update checks the bound against what rocPRIM asks for.
SelectPlan make_plan(int64_t A, int64_t K, int64_t seg_len, int64_t max_chunk, size_t key_bytes) {
  SelectPlan pl;
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
  pl.off_ckey = take((size_t)max_chunk * key_bytes);
  pl.off_cidx = take((size_t)max_chunk * 4);
  pl.off_skey = take((size_t)max_chunk * key_bytes);
  pl.off_sidx = take((size_t)max_chunk * 4);
  pl.sort_bytes = (size_t)max_chunk * (2 * key_bytes + 8) + ((size_t)4 << 20);
  pl.off_sort = take(pl.sort_bytes);
  pl.total = off;
  return pl;
}

// the plain selection: one segment that no chunk leaves
constexpr int64_t kOneSegment = INT64_MAX;
SelectPlan make_topk_plan(int64_t K, int64_t max_chunk) { return make_plan(1, K, kOneSegment, max_chunk, 4); }

struct TopkState {
  uint32_t* key;
  float* score;
  int64_t* rank;
};

TopkState state_at(const void* base, size_t off_key, size_t off_score, size_t off_rank) {
  char* w = (char*)base;
  return TopkState{(uint32_t*)(w + off_key), (float*)(w + off_score), (int64_t*)(w + off_rank)};
}

__global__ __launch_bounds__(256) void select_init_kernel(TopkState st, int64_t slots) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= slots) return;
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

// (key, rank) of the state before (key, rank) of the chunk?  Equal pairs (the same rank fed twice) go either way: they are the same pair.
__device__ __forceinline__ bool state_first(uint32_t ka, int64_t ra, uint32_t kb, int64_t rb) { return ka < kb || (ka == kb && ra <= rb); }

// thread (t, p): chunk segment t is state segment seg_first + t; its sorted run is [start, end) of the sorted chunk.  With 32-bit keys
// (the plain selection) there is one segment, the state's first, and its run is the whole chunk: t, start, end and sbase are constants.
template <class KeyT>
__global__ __launch_bounds__(256) void select_merge_kernel(TopkState st, uint32_t K, int64_t T, int64_t seg_first, uint64_t off0, uint64_t seg_len, int64_t n,
                                                           const KeyT* __restrict__ skey, const uint32_t* __restrict__ sidx,
                                                           const float* __restrict__ scores, int64_t g0, TopkState out) {
  const int64_t flat = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (flat >= T * (int64_t)K) return;                                  // T K < 2^31
  int64_t p = flat, start = 0, end = n, sbase = 0;
  if constexpr (sizeof(KeyT) == 8) {
    const uint32_t t = (uint32_t)flat / K;
    p = (int64_t)((uint32_t)flat - t * K);
    // t >= 1 only when seg_len <= off0 + n - 1 < 2^32, so the products below cannot overflow
    start = t == 0 ? 0 : (int64_t)((uint64_t)t * seg_len - off0);
    const uint64_t room = ((uint64_t)t + 1) * seg_len - off0;          // rows of the chunk before the next segment begins
    end = room < (uint64_t)n ? (int64_t)room : n;
    sbase = (seg_first + (int64_t)t) * (int64_t)K;
  }
  const int64_t len = end - start;
  const int64_t nb = len < (int64_t)K ? len : (int64_t)K;
  const uint32_t* __restrict__ akey = st.key + sbase;
  const int64_t* __restrict__ arank = st.rank + sbase;
  const KeyT* __restrict__ bkey = skey + start;
  const uint32_t* __restrict__ bidx = sidx + start;
  // ia = how many of the first p merged elements come from the state: the smallest ia whose successor in the state does not precede the
  // chunk element it would displace
  int64_t lo = p > nb ? p - nb : 0, hi = p;                            // p < K, so ia <= p < K
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

__global__ __launch_bounds__(256) void select_commit_kernel(TopkState from, TopkState to, int64_t to_base, int64_t slots) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= slots) return;
  to.key[to_base + p] = from.key[p];
  to.score[to_base + p] = from.score[p];
  to.rank[to_base + p] = from.rank[p];
}

__global__ __launch_bounds__(256) void select_read_kernel(TopkState st, uint32_t K, int64_t slots, float* __restrict__ scores_out,
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

int select_init(bool seg, void* state, const SelectPlan& pl, int64_t slots, matcha_stream_t stream) {
  hipLaunchKernelGGL(select_init_kernel, dim3((unsigned)cdiv(slots, 256)), dim3(256), 0, (hipStream_t)stream,
                     state_at(state, pl.off_key, pl.off_score, pl.off_rank), slots);
  MATCHA_CHECK_LAUNCH(SELECT_KERNEL_NAME(seg, "init"));
  return MATCHA_OK;
}

// One update, n >= 1 rows of global ranks g0 + i: keys -> sort -> merge -> commit.  The chunk's first row lies off0 ranks into state
// segment seg_first and the chunk touches T <= pl.tmax segments.  KeyT = uint32_t is the plain selection (T = 1), uint64_t the segmented.
template <class KeyT>
int select_update(const char* fn, void* state, const SelectPlan& pl, int32_t K, int64_t T, int64_t seg_first, uint64_t off0, int64_t seg_len,
                  const float* scores, const int32_t* skip, int64_t n, int64_t g0, matcha_stream_t stream) {
  constexpr bool seg = sizeof(KeyT) == 8;
  int bits = 0;
  while (((int64_t)1 << bits) < T) ++bits;
  const unsigned end_bit = 32u + (unsigned)bits;
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)state;
  KeyT* ckey = (KeyT*)(w + pl.off_ckey);
  uint32_t* cidx = (uint32_t*)(w + pl.off_cidx);
  KeyT* skey = (KeyT*)(w + pl.off_skey);
  uint32_t* sidx = (uint32_t*)(w + pl.off_sidx);
  size_t need = 0;
  if (rocprim::radix_sort_pairs(nullptr, need, ckey, skey, cidx, sidx, (size_t)n, 0, end_bit, st) != hipSuccess || need > pl.sort_bytes) {
    set_error("%s: the radix sort asks for %zu bytes of scratch, %zu are reserved", fn, need, pl.sort_bytes);
    return MATCHA_EHIP;
  }
  if constexpr (seg) {
    const int wide = seg_len >= ((int64_t)1 << 31);
    hipLaunchKernelGGL(segtopk_keys_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, scores, skip, n, off0, (uint64_t)seg_len, wide, ckey, cidx);
  } else {
    hipLaunchKernelGGL(topk_keys_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, scores, skip, n, ckey, cidx);
  }
  MATCHA_CHECK_LAUNCH(SELECT_KERNEL_NAME(seg, "keys"));
  size_t tb = pl.sort_bytes;
  if (rocprim::radix_sort_pairs(w + pl.off_sort, tb, ckey, skey, cidx, sidx, (size_t)n, 0, end_bit, st) != hipSuccess) {
    set_error("%s: radix sort failed", fn);
    return MATCHA_EHIP;
  }
  const TopkState cur = state_at(state, pl.off_key, pl.off_score, pl.off_rank);
  const TopkState tmp = state_at(state, pl.off_tkey, pl.off_tscore, pl.off_trank);
  const int64_t slots = T * K;
  const unsigned blocks = (unsigned)cdiv(slots, 256);
  hipLaunchKernelGGL(select_merge_kernel<KeyT>, dim3(blocks), dim3(256), 0, st, cur, (uint32_t)K, T, seg_first, off0, (uint64_t)seg_len, n, skey, sidx, scores,
                     g0, tmp);
  MATCHA_CHECK_LAUNCH(SELECT_KERNEL_NAME(seg, "merge"));
  hipLaunchKernelGGL(select_commit_kernel, dim3(blocks), dim3(256), 0, st, tmp, cur, seg_first * K, slots);
  MATCHA_CHECK_LAUNCH(SELECT_KERNEL_NAME(seg, "commit"));
  return MATCHA_OK;
}

int select_read(bool seg, const void* state, const SelectPlan& pl, int32_t K, int64_t slots, float* scores_out, int64_t* ranks_out, int64_t* counts_out,
                matcha_stream_t stream) {
  hipLaunchKernelGGL(select_read_kernel, dim3((unsigned)cdiv(slots, 256)), dim3(256), 0, (hipStream_t)stream,
                     state_at(state, pl.off_key, pl.off_score, pl.off_rank), (uint32_t)K, slots, scores_out, ranks_out, counts_out);
  MATCHA_CHECK_LAUNCH(SELECT_KERNEL_NAME(seg, "read"));
  return MATCHA_OK;
}

}  // namespace
}  // namespace matcha

using namespace matcha;

// What every state-taking entry checks first; declares the plan `pl`.  need: the argument rule as a format and its values.
#define SELECT_COMMON_ARGS(fn, bytes_fn, args_ok, plan, ...)                                                                          \
  MATCHA_CHECK_ARG(state, fn ": null state");                                                                                         \
  MATCHA_CHECK_ARG(args_ok, fn ": need " __VA_ARGS__);                                                                                \
  MATCHA_CHECK_ARG(((uintptr_t)state) % 8 == 0, fn ": state must be 8-byte aligned");                                                 \
  const SelectPlan pl = plan;                                                                                                         \
  MATCHA_CHECK_ARG(bytes >= pl.total, fn ": state too small (%zu bytes, " bytes_fn " says %zu)", bytes, pl.total)

#define TOPK_COMMON_ARGS(fn)                                                                                                          \
  SELECT_COMMON_ARGS(fn, "matcha_topk_bytes", topk_args_ok(K, max_chunk), make_topk_plan(K, max_chunk),                               \
                     "1 <= K < 2^31 and 1 <= max_chunk < 2^31 (K=%d max_chunk=%lld)", K, (long long)max_chunk)

#define SEGTOPK_COMMON_ARGS(fn)                                                                                                       \
  SELECT_COMMON_ARGS(fn, "matcha_segtopk_bytes", seg_args_ok(A, K, seg_len, max_chunk), make_plan(A, K, seg_len, max_chunk, 8),       \
                     "1 <= K, 1 <= A, A K < 2^31, seg_len >= 1 and 1 <= max_chunk < 2^31 (A=%lld K=%d seg_len=%lld max_chunk=%lld)",  \
                     (long long)A, K, (long long)seg_len, (long long)max_chunk)

extern "C" size_t matcha_topk_bytes(int32_t K, int64_t max_chunk) {
  if (!topk_args_ok(K, max_chunk)) return 0;
  return make_topk_plan(K, max_chunk).total;
}

extern "C" int matcha_topk_init(void* state, size_t bytes, int32_t K, int64_t max_chunk, matcha_stream_t stream) {
  TOPK_COMMON_ARGS("matcha_topk_init");
  return select_init(false, state, pl, K, stream);
}

extern "C" int matcha_topk_update(void* state, size_t bytes, int32_t K, int64_t max_chunk, const float* scores, const int32_t* skip, int64_t n,
                                  int64_t rank0, matcha_stream_t stream) {
  TOPK_COMMON_ARGS("matcha_topk_update");
  MATCHA_CHECK_ARG(n >= 0 && n <= max_chunk, "matcha_topk_update: n=%lld outside [0, max_chunk=%lld]", (long long)n, (long long)max_chunk);
  MATCHA_CHECK_ARG(rank0 >= 0 && rank0 <= INT64_MAX - n, "matcha_topk_update: rank0 out of range");
  if (n == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(scores, "matcha_topk_update: null scores");
  return select_update<uint32_t>("matcha_topk_update", state, pl, K, 1, 0, 0, kOneSegment, scores, skip, n, rank0, stream);
}

extern "C" int matcha_topk_read(const void* state, size_t bytes, int32_t K, int64_t max_chunk, float* scores_out, int64_t* ranks_out,
                                int64_t* n_out, matcha_stream_t stream) {
  TOPK_COMMON_ARGS("matcha_topk_read");
  MATCHA_CHECK_ARG(scores_out && ranks_out && n_out, "matcha_topk_read: null output");
  return select_read(false, state, pl, K, K, scores_out, ranks_out, n_out, stream);
}

extern "C" size_t matcha_segtopk_bytes(int64_t A, int32_t K, int64_t seg_len, int64_t max_chunk) {
  if (!seg_args_ok(A, K, seg_len, max_chunk)) return 0;
  return make_plan(A, K, seg_len, max_chunk, 8).total;
}

extern "C" int matcha_segtopk_init(void* state, size_t bytes, int64_t A, int32_t K, int64_t seg_len, int64_t max_chunk, matcha_stream_t stream) {
  SEGTOPK_COMMON_ARGS("matcha_segtopk_init");
  return select_init(true, state, pl, A * K, stream);
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
  return select_update<uint64_t>("matcha_segtopk_update", state, pl, K, T, seg_first, off0, seg_len, scores, skip, n, g0, stream);
}

extern "C" int matcha_segtopk_read(const void* state, size_t bytes, int64_t A, int32_t K, int64_t seg_len, int64_t max_chunk, float* scores_out,
                                   int64_t* ranks_out, int64_t* counts_out, matcha_stream_t stream) {
  SEGTOPK_COMMON_ARGS("matcha_segtopk_read");
  MATCHA_CHECK_ARG(scores_out && ranks_out && counts_out, "matcha_segtopk_read: null output");
  return select_read(true, state, pl, K, A * K, scores_out, ranks_out, counts_out, stream);
}
