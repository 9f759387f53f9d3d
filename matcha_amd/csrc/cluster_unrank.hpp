// The pair of positions of a rank inside one cluster (cluster_adj.hip; checked on the host by tests/host/cluster_adj_checks.hip).
//
// The s (s - 1) / 2 pairs i < j of a cluster of s nodes are ranked row by row: row i holds j = i + 1 .. s - 1 and starts at
// R(i) = i (2 s - i - 1) / 2, so consecutive ranks of a row address consecutive j.  i is the largest row with R(i) <= r: the root of
// i^2 - (2 s - 1) i + 2 r = 0 in double, then an integer step either way -- the root alone is not trusted at a row's first and last rank.
// s <= 65535 keeps every rank below 2^31 and (2 s - 1)^2 - 8 r an exact double.
#pragma once

#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace matcha {

constexpr int32_t kMaxClusterNodes = 65535;

__host__ __device__ __forceinline__ int64_t tri_row_start(int64_t i, int64_t s) { return i * (2 * s - i - 1) / 2; }

// 0 <= r < s (s - 1) / 2, 2 <= s <= kMaxClusterNodes
__host__ __device__ __forceinline__ void tri_unrank(int64_t r, int32_t s, int32_t& i_out, int32_t& j_out) {
  const double b = (double)(2 * (int64_t)s - 1);
  double disc = b * b - 8.0 * (double)r;
  disc = disc > 0.0 ? disc : 0.0;
  int64_t i = (int64_t)((b - sqrt(disc)) * 0.5);
  i = i < 0 ? 0 : i;
  i = i > s - 2 ? s - 2 : i;
  while (tri_row_start(i, s) > r) --i;                    // R(0) = 0 <= r ends it
  while (i < s - 2 && tri_row_start(i + 1, s) <= r) ++i;
  i_out = (int32_t)i;
  j_out = (int32_t)(i + 1 + (r - tri_row_start(i, s)));
}

}  // namespace matcha
