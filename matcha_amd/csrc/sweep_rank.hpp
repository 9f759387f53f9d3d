// What the sweep files (sweep_rows.hip, sweep_select.hip, sweep_support.hip) and grow.hip share: the combinatorics of a rank space
// (exact binomials, C(m, k) on the host, unrank, the split of a global rank g = a c + r), the checks every *_rows entry makes on its range
// of ranks, and the two frames of a rows kernel -- the LDS tile's coalesced flush and the wavefront kernels' one-rank-per-lane prologue.
#pragma once

#include <cmath>
#include <cstdint>

#include "common.hpp"

namespace matcha {

constexpr int kMaxK = MATCHA_MAX_L;            // candidate sizes 2 .. 8
constexpr int kMaxWide = MATCHA_MAX_LONG_L;    // the widest row: S + f <= L <= 32
constexpr int kRowsPerBlock = 256;

__host__ __device__ __forceinline__ uint32_t gcd_small(uint32_t a, uint32_t b) {
  while (b) { const uint32_t t = a % b; a = b; b = t; }
  return a;
}

// r / d for d in 1 .. 8 with constant divisors (a 64-bit division by a variable is a long software routine on the device)
template <class T>
__host__ __device__ __forceinline__ T div_by_small(T r, uint32_t d) {
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
__host__ __device__ __forceinline__ uint64_t div_small(uint64_t r, uint32_t d) { return div_by_small(r, d); }
__host__ __device__ __forceinline__ uint32_t div_small32(uint32_t r, uint32_t d) { return div_by_small(r, d); }

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
inline int64_t count_subsets(int64_t m, int k) {
  if (m < k) return 0;
  unsigned __int128 r = 1;
  const unsigned __int128 lim = (unsigned __int128)1 << 63;
  for (int i = 1; i <= k; ++i) {
    r = r * (unsigned __int128)(m - k + i) / (unsigned __int128)i;
    if (r >= lim) return -1;
  }
  return (int64_t)r;
}

// A c, the ranks of A segments of c candidates each: -1 for c < 0 (a count that did not fit) or a total >= 2^63; *c_out = c
inline int64_t segmented_total(int64_t A, int64_t c, int64_t* c_out) {
  if (c < 0) return -1;
  const unsigned __int128 total = (unsigned __int128)(uint64_t)A * (uint64_t)c;
  if (total >= ((unsigned __int128)1 << 63)) return -1;
  if (c_out) *c_out = c;
  return (int64_t)total;
}

// one block per per_block rows, clamped: the kernels stride over what is left
inline unsigned rows_grid(int64_t count, int per_block) {
  const int64_t blocks = cdiv(count, per_block);
  return (unsigned)(blocks > (1 << 20) ? 1 << 20 : blocks);
}

// The part of a *_rows entry that every one of them repeats: `count`, the range [rank0, rank0 + count) against `total` when there is no
// list of ranks, and the grid.  Reads the entry's `count`, `rank0` and `total` (int64_t, total >= 0) and declares `blocks`.
#define MATCHA_ROWS_RANGE(fn, has_list, per_block)                                                                                  \
  MATCHA_CHECK_ARG(count >= 0 && count <= ((int64_t)1 << 40), fn ": count out of range");                                           \
  MATCHA_CHECK_ARG((has_list) || (rank0 >= 0 && rank0 <= total && count <= total - rank0), fn ": %lld ranks from %lld lie outside [0, %lld)", \
                   (long long)count, (long long)rank0, (long long)total);                                                           \
  const unsigned blocks = rows_grid(count, per_block)

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

__device__ __forceinline__ int64_t shfl64(int64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)((uint64_t)v >> 32), src);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The end of an LDS-tile rows kernel's run: the block's rows, written at tile[thread L + c], leave as one contiguous, coalesced run.
__device__ __forceinline__ void flush_row_tile(const int64_t* tile, int64_t base, int64_t count, int32_t L, int64_t* __restrict__ x) {
  __syncthreads();
  const int64_t rows = count - base < kRowsPerBlock ? count - base : kRowsPerBlock;
  const int elems = (int)rows * L;
  for (int e = threadIdx.x; e < elems; e += kRowsPerBlock) x[base * L + e] = tile[e];
  __syncthreads();                                                   // the tile is reused by the next run of rows
}

// The start of a wavefront rows kernel's run: the wavefront serves the 64 rows from w0, two per step, and every lane owns ONE of them.
struct WaveRows {
  int64_t w0;      // the wavefront's first row; the same in all its lanes
  int steps;       // the same for the whole wavefront
  int64_t i, g;    // the lane's row and its global rank (-1 behind the last row)
  int ok;          // g in [0, total): total > 0 then, so the segment length is > 0
};
__device__ __forceinline__ WaveRows wave_rows(int64_t base, int64_t count, int64_t rank0, const int64_t* __restrict__ ranks, uint64_t total) {
  WaveRows w;
  w.w0 = base + (int64_t)(threadIdx.x >> 6) * 64;
  const int64_t left = count - w.w0;
  w.steps = left >= 64 ? 32 : left > 0 ? (int)((left + 1) >> 1) : 0;
  w.i = w.w0 + (threadIdx.x & 63);
  w.g = w.i < count ? (ranks ? ranks[w.i] : rank0 + w.i) : -1;
  w.ok = w.g >= 0 && (uint64_t)w.g < total;
  return w;
}

}  // namespace matcha
