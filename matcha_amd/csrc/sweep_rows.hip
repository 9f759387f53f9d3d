// The candidate rows of every sweep, made on the device from their rank: five rows kernels with their *_count and *_rows entries.  The
// rank arithmetic, the range checks and the kernels' shared frames are sweep_rank.hpp's.  Every kernel serves a range of ranks
// (rank0 + i) and a device list of ranks (the winners at the end); a rank outside [0, total) gives a zero row (flagged, where there is
// a flag).  No atomics, no scratch.
//
// De novo k-way sweep.  A candidate of size k in the region [lo, lo + n) is a strictly ascending k-tuple of node ids
// whose adjacent differences are all >= min_gap (generate_kmers.py:18, :33 and the sampler's rule with min_gap = min_distance + 1).  With
// s = min_gap - 1 and m = n - (k - 1) s, y_j = x_j - lo - j s maps them, order preserved, onto the plain k-subsets of [0, m): C(m, k) of
// them, ranked lexicographically from 0.
//
//   kway_rows_kernel   one thread per row.  The lexicographic rank r of y equals total - 1 - (colexicographic rank of the mirrored set
//                      z_j = m - 1 - y_j), so the row is read off the combinatorial number system of q = total - 1 - r: for j = k .. 1
//                      the largest c with C(c, j) <= q (z_{k-j} = c, q -= C(c, j)).  c is estimated as (q j!)^(1/j) + (j - 1) / 2 in
//                      float64 and corrected with exact integer binomials, so the result does not depend on the estimate.  64-bit
//                      integers throughout: C(a, j) is built as C(a-j+i, i) = C(a-j+i-1, i-1) (a-j+i) / i with gcd(a-j+i, i) divided out
//                      of both factors first, which keeps every intermediate <= the result (n = 120 000, k = 4 has C > 2^61, where
//                      the plain product passes 2^64).  Rows go through LDS and leave as one contiguous, coalesced run per block.
#include <hip/hip_runtime.h>

#include "sweep_rank.hpp"

namespace matcha {
namespace {

bool kway_args_ok(int32_t n, int32_t k, int32_t min_gap) { return n >= 1 && k >= 2 && k <= kMaxK && min_gap >= 1; }

// C_f = C(n - (f - 1)(min_gap - 1), f) for f >= 1 (f = 1: n), -1 when it does not fit 63 bits
int64_t free_count(int32_t n, int32_t f, int32_t min_gap) {
  return count_subsets((int64_t)n - (int64_t)(f - 1) * (min_gap - 1), f);
}

int64_t kway_count(int32_t n, int32_t k, int32_t min_gap) { return kway_args_ok(n, k, min_gap) ? free_count(n, k, min_gap) : -1; }

// m = n - (f - 1) slack clamped at 0: the free part's candidates are the f-subsets of [0, m)
int32_t free_m(int32_t n, int32_t f, int32_t slack) {
  const int64_t m64 = (int64_t)n - (int64_t)(f - 1) * slack;
  return m64 > 0 ? (int32_t)m64 : 0;
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
    flush_row_tile(tile, base, count, L, x);
  }
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
bool anchor_args_ok(int64_t A, int32_t s, int32_t n, int32_t k, int32_t min_gap) {
  return A >= 0 && n >= 1 && k >= 2 && k <= kMaxK && s >= 1 && s <= k - 1 && min_gap >= 1;
}

// A C_f, -1 for invalid arguments or a total >= 2^63; *cf_out = C_f
int64_t anchor_count(int64_t A, int32_t s, int32_t n, int32_t k, int32_t min_gap, int64_t* cf_out) {
  return anchor_args_ok(A, s, n, k, min_gap) ? segmented_total(A, free_count(n, k - s, min_gap), cf_out) : -1;
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
        split_rank((uint64_t)g, cf, a, r);                             // the one 64-bit division of the row
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
    flush_row_tile(tile, base, count, L, x);
  }
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
bool complete_args_ok(int64_t A, int32_t S, int32_t n, int32_t f, int32_t min_gap) {
  return A >= 0 && S >= 1 && S <= kMaxWide - 1 && n >= 1 && f >= 1 && f <= kMaxK && min_gap >= 1;
}

// A C_f, -1 for invalid arguments or a total >= 2^63; *cf_out = C_f
int64_t complete_count(int64_t A, int32_t S, int32_t n, int32_t f, int32_t min_gap, int64_t* cf_out) {
  return complete_args_ok(A, S, n, f, min_gap) ? segmented_total(A, free_count(n, f, min_gap), cf_out) : -1;
}

__global__ __launch_bounds__(kRowsPerBlock) void kway_complete_rows_kernel(const int64_t* __restrict__ clusters, int32_t S, int64_t lo, int32_t m, int32_t f,
                                                                           int32_t slack, int32_t min_gap, uint64_t cf, uint64_t total, int64_t rank0,
                                                                           const int64_t* __restrict__ ranks, int64_t count, int32_t L,
                                                                           int64_t* __restrict__ x, int32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31;
  const uint64_t gap = (uint64_t)min_gap;
  for (int64_t base = (int64_t)blockIdx.x * kRowsPerBlock; base < count; base += (int64_t)gridDim.x * kRowsPerBlock) {
    // ---- one rank per lane: cluster index and free ids ----
    const WaveRows w = wave_rows(base, count, rank0, ranks, total);
    const int ok = w.ok;
    uint64_t a = 0;
    int32_t fid[kMaxK] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) {
      uint64_t r;
      split_rank((uint64_t)w.g, cf, a, r);                              // the one 64-bit division of the row
      unrank(r, cf, m, f, fid);
#pragma unroll
      for (int c = 0; c < kMaxK; ++c) fid[c] += c * slack;              // < n: relative to lo
    }
    // ---- two rows per step, one per half ----
    int bad_mine = 1;
    for (int t = 0; t < w.steps; ++t) {
      const int own = 2 * t + h;                                       // the lane that unranked this half's row
      const int64_t irow = w.w0 + own;
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
    if (w.i < count) flag[w.i] = bad_mine;
  }
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
// The per-locus and per-pair support of the same choices is sweep_support.hip's.
bool subset_args_ok(int64_t A, int32_t S, int32_t m, int32_t complement) {
  return A >= 0 && S >= 2 && S <= kMaxWide && (complement == 0 || complement == 1) && m >= (complement ? 1 : 2) && m <= kMaxK;
}

// A C(S, m), -1 for invalid arguments or a total >= 2^63; *cm_out = C(S, m) <= C(32, 8)
int64_t subset_count(int64_t A, int32_t S, int32_t m, int32_t complement, int64_t* cm_out) {
  return subset_args_ok(A, S, m, complement) ? segmented_total(A, count_subsets(S, m), cm_out) : -1;
}

__global__ __launch_bounds__(kRowsPerBlock) void cluster_subset_rows_kernel(const int64_t* __restrict__ clusters, int32_t S, int32_t m, int32_t complement,
                                                                            int32_t min_gap, uint64_t cm, uint64_t total, int64_t rank0,
                                                                            const int64_t* __restrict__ ranks, int64_t count, int32_t L,
                                                                            int64_t* __restrict__ x, int32_t* __restrict__ flag) {
  const int lane = threadIdx.x & 63, h = lane >> 5, j = lane & 31;
  const uint64_t gap = (uint64_t)min_gap;
  const uint32_t below_me = (1u << j) - 1u;                            // j <= 31
  for (int64_t base = (int64_t)blockIdx.x * kRowsPerBlock; base < count; base += (int64_t)gridDim.x * kRowsPerBlock) {
    // ---- one rank per lane: cluster index and the choice as a mask of positions ----
    const WaveRows w = wave_rows(base, count, rank0, ranks, total);    // ok: cm > 0 and m <= S
    const int ok = w.ok;
    uint64_t a = 0;
    uint32_t mask = 0;
    if (ok) {
      uint64_t r;
      split_rank((uint64_t)w.g, cm, a, r);
      int32_t y[kMaxK] = {0, 0, 0, 0, 0, 0, 0, 0};
      unrank(r, cm, S, m, y);
#pragma unroll
      for (int c = 0; c < kMaxK; ++c)
        if (c < m) mask |= 1u << (y[c] & 31);                          // y[c] < S <= 32
    }
    // ---- two rows per step, one per half ----
    int bad_mine = 1;
    for (int t = 0; t < w.steps; ++t) {
      const int own = 2 * t + h;                                       // the lane that unranked this half's row
      const int64_t irow = w.w0 + own;
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
    if (w.i < count) flag[w.i] = bad_mine;
  }
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
            uint64_t r = rest;                                         // part 0: rest < C_0, nothing left to divide
            if (p > 0) split_rank(rest, cp, rest, r);                  // the part's one 64-bit division; the quotient is the rest
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
    flush_row_tile(tile, base, count, L, x);
  }
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
  MATCHA_ROWS_RANGE("matcha_kway_rows", ranks != nullptr, kRowsPerBlock);
  if (count == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(x, "matcha_kway_rows: null output");
  const int32_t slack = min_gap - 1;
  hipLaunchKernelGGL(kway_rows_kernel, dim3(blocks), dim3(kRowsPerBlock), 0, (hipStream_t)stream, lo, free_m(n, k, slack), k, slack, (uint64_t)total,
                     rank0, ranks, count, L, x);
  MATCHA_CHECK_LAUNCH("kway_rows_kernel");
  return MATCHA_OK;
}

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
  MATCHA_ROWS_RANGE("matcha_kway_anchor_rows", ranks != nullptr, kRowsPerBlock);
  if (count == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(x && flag, "matcha_kway_anchor_rows: null output");
  MATCHA_CHECK_ARG(anchors || total == 0, "matcha_kway_anchor_rows: null anchors");
  const int32_t f = k - s, slack = min_gap - 1;
  hipLaunchKernelGGL(kway_anchor_rows_kernel, dim3(blocks), dim3(kRowsPerBlock), 0, (hipStream_t)stream, anchors, s, lo, free_m(n, f, slack), f, slack,
                     min_gap, (uint64_t)cf, (uint64_t)total, rank0, ranks, count, L, x, flag);
  MATCHA_CHECK_LAUNCH("kway_anchor_rows_kernel");
  return MATCHA_OK;
}

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
  MATCHA_ROWS_RANGE("matcha_kway_complete_rows", ranks != nullptr, kRowsPerBlock);
  if (count == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(x && flag, "matcha_kway_complete_rows: null output");
  MATCHA_CHECK_ARG(clusters || total == 0, "matcha_kway_complete_rows: null clusters");
  const int32_t slack = min_gap - 1;
  hipLaunchKernelGGL(kway_complete_rows_kernel, dim3(blocks), dim3(kRowsPerBlock), 0, (hipStream_t)stream, clusters, S, lo, free_m(n, f, slack), f, slack,
                     min_gap, (uint64_t)cf, (uint64_t)total, rank0, ranks, count, L, x, flag);
  MATCHA_CHECK_LAUNCH("kway_complete_rows_kernel");
  return MATCHA_OK;
}

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
  MATCHA_ROWS_RANGE("matcha_cluster_subset_rows", ranks != nullptr, kRowsPerBlock);
  if (count == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(x && flag, "matcha_cluster_subset_rows: null output");
  MATCHA_CHECK_ARG(clusters || total == 0, "matcha_cluster_subset_rows: null clusters");
  hipLaunchKernelGGL(cluster_subset_rows_kernel, dim3(blocks), dim3(kRowsPerBlock), 0, (hipStream_t)stream, clusters, S, m, complement, min_gap,
                     (uint64_t)cm, (uint64_t)total, rank0, ranks, count, L, x, flag);
  MATCHA_CHECK_LAUNCH("cluster_subset_rows_kernel");
  return MATCHA_OK;
}

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
  MATCHA_ROWS_RANGE("matcha_kway_region_rows", ranks != nullptr, kRowsPerBlock);
  if (count == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(x && flag, "matcha_kway_region_rows: null output");
  hipLaunchKernelGGL(kway_region_rows_kernel, dim3(blocks), dim3(kRowsPerBlock), 0, (hipStream_t)stream, parts, (int32_t)k, min_gap - 1, min_gap,
                     (uint64_t)total, rank0, ranks, count, L, x, flag);
  MATCHA_CHECK_LAUNCH("kway_region_rows_kernel");
  return MATCHA_OK;
}
