// Cluster completion's host side (csrc/sweep_rows.hip: matcha_kway_complete_count and the argument checks of matcha_kway_complete_rows, DESIGN.md
// 7.10) under AddressSanitizer + UndefinedBehaviorSanitizer on the host, next to tests/host/route_pairs.hip: the same host-only objects,
// model.hip included as source for the library's error and option plumbing, a driver of its own.  No kernel runs: every call to the rows
// entry point below is refused, or is a no-op, before any device call, on pointers that are never dereferenced.
#include "host_driver.hpp"

// C(m, f) in 128 bits, -1 from 2^63 on: the definition, multiplied out
static __int128 choose(int64_t m, int f) {
  if (m < f) return 0;
  __int128 r = 1;
  for (int i = 1; i <= f; ++i) {
    r = r * (m - f + i) / i;
    if (r >= ((__int128)1 << 63)) return -1;
  }
  return r;
}

static int64_t want_count(int64_t A, int S, int n, int f, int g) {
  if (A < 0 || S < 1 || S > 31 || n < 1 || f < 1 || f > 8 || g < 1) return -1;
  const __int128 cf = choose((int64_t)n - (int64_t)(f - 1) * (g - 1), f);
  if (cf < 0) return -1;
  const __int128 total = (__int128)A * cf;
  return total >= ((__int128)1 << 63) ? -1 : (int64_t)total;
}

int main() {
  const int64_t As[] = {-1, 0, 1, 7, 1000003, (int64_t)1 << 40, INT64_MAX};
  const int Ss[] = {-1, 0, 1, 8, 9, 31, 32, INT32_MAX};
  const int ns[] = {INT32_MIN, 0, 1, 7, 16, 250, 2491, 120000, INT32_MAX};
  const int fs[] = {INT32_MIN, 0, 1, 2, 5, 8, 9, INT32_MAX};
  const int gs[] = {INT32_MIN, 0, 1, 2, 3, 1000, INT32_MAX};
  for (int64_t A : As)
    for (int S : Ss)
      for (int n : ns)
        for (int f : fs)
          for (int g : gs) CHECK(matcha_kway_complete_count(A, S, n, f, g) == want_count(A, S, n, f, g));
  CHECK(matcha_kway_complete_count(3, 31, 16, 1, 1) == 48);
  CHECK(matcha_kway_complete_count(3, 1, 6, 3, 3) == 0);

  int64_t host[8] = {0};
  int32_t hflag[8] = {0};
  int64_t* const p = host;
  int32_t* const q = hflag;
  // clusters, A, S, lo, n, f, min_gap, rank0, ranks, count, L, x, flag
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, 1, 16, 1, 1, 0, nullptr, 4, 10, nullptr, q, nullptr), "null output"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, 1, 16, 1, 1, 0, nullptr, 4, 10, p, nullptr, nullptr), "null output"));
  CHECK(refused(matcha_kway_complete_rows(nullptr, 4, 9, 1, 16, 1, 1, 0, nullptr, 4, 10, p, q, nullptr), "null clusters"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 0, 1, 16, 1, 1, 0, nullptr, 4, 10, p, q, nullptr), "S"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 32, 1, 16, 1, 1, 0, nullptr, 4, 32, p, q, nullptr), "S"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, 1, 16, 0, 1, 0, nullptr, 4, 10, p, q, nullptr), "f"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, 1, 16, 9, 1, 0, nullptr, 4, 18, p, q, nullptr), "f"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, 1, 16, 2, 1, 0, nullptr, 4, 10, p, q, nullptr), "width"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 31, 1, 16, 1, 1, 0, nullptr, 4, 33, p, q, nullptr), "width"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 31, 1, 16, 8, 1, 0, nullptr, 4, 32, p, q, nullptr), "width"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, 1, 16, 1, 1, 0, nullptr, 4, INT32_MAX, p, q, nullptr), "width"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, 1, 16, 1, 0, 0, nullptr, 4, 10, p, q, nullptr), "min_gap"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, -1, 16, 1, 1, 0, nullptr, 4, 10, p, q, nullptr), "lo"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, INT64_MAX, 16, 1, 1, 0, nullptr, 4, 10, p, q, nullptr), "lo"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, 1, 16, 1, 1, 62, nullptr, 4, 10, p, q, nullptr), "outside"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, 1, 16, 1, 1, -1, nullptr, 1, 10, p, q, nullptr), "outside"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, 1, 16, 1, 1, INT64_MAX, nullptr, 1, 10, p, q, nullptr), "outside"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, 1, 16, 1, 1, 0, nullptr, -1, 10, p, q, nullptr), "count"));
  CHECK(refused(matcha_kway_complete_rows(p, 4, 9, 1, 16, 1, 1, 0, nullptr, INT64_MAX, 10, p, q, nullptr), "count"));
  CHECK(refused(matcha_kway_complete_rows(p, (int64_t)1 << 40, 9, 1, 2491, 4, 1, 0, nullptr, 1, 13, p, q, nullptr), "63 bits"));
  CHECK(refused(matcha_kway_complete_rows(p, INT64_MAX, 9, 1, INT32_MAX, 8, 1, 0, nullptr, 1, 17, p, q, nullptr), "63 bits"));
  // no-ops: accepted, nothing launched
  CHECK(matcha_kway_complete_rows(p, 4, 9, 1, 16, 1, 1, 0, nullptr, 0, 10, nullptr, nullptr, nullptr) == MATCHA_OK);
  CHECK(matcha_kway_complete_rows(p, 4, 9, 1, 16, 1, 1, 64, nullptr, 0, 10, nullptr, nullptr, nullptr) == MATCHA_OK);
  CHECK(matcha_kway_complete_rows(nullptr, 0, 9, 1, 16, 1, 1, 0, nullptr, 0, 10, nullptr, nullptr, nullptr) == MATCHA_OK);
  CHECK(matcha_kway_complete_rows(p, 4, 9, 1, 16, 1, 1, 0, p, 0, 10, nullptr, nullptr, nullptr) == MATCHA_OK);

  return finish("CLUSTER COMPLETION HOST CHECKS");
}
