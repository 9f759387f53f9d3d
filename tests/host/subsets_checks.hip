// Cluster decomposition's host side (csrc/sweep_rows.hip and csrc/sweep_support.hip: matcha_cluster_subset_count, the argument checks of matcha_cluster_subset_rows and of
// matcha_subset_support_*) under AddressSanitizer + UndefinedBehaviorSanitizer on the host, next to
// tests/host/complete_checks.hip: the same host-only objects, model.hip included as source for the library's error and option plumbing, a
// driver of its own.  No kernel runs: every call below is refused, or is a no-op, before any device call, on pointers that are never
// dereferenced.
#include "host_driver.hpp"

// C(S, m) in 128 bits: the definition, multiplied out
static __int128 choose(int64_t S, int m) {
  if (S < m) return 0;
  __int128 r = 1;
  for (int i = 1; i <= m; ++i) r = r * (S - m + i) / i;
  return r;
}

static int64_t want_count(int64_t A, int S, int m, int complement) {
  if (A < 0 || S < 2 || S > 32 || (complement != 0 && complement != 1) || m < (complement ? 1 : 2) || m > 8) return -1;
  const __int128 total = (__int128)A * choose(S, m);
  return total >= ((__int128)1 << 63) ? -1 : (int64_t)total;
}

int main() {
  const int64_t As[] = {-1, 0, 1, 7, 1000003, (int64_t)1 << 40, (int64_t)1 << 50, INT64_MAX};
  const int Ss[] = {INT32_MIN, -1, 0, 1, 2, 3, 8, 9, 31, 32, 33, INT32_MAX};
  const int ms[] = {INT32_MIN, 0, 1, 2, 3, 5, 8, 9, INT32_MAX};
  const int cs[] = {INT32_MIN, -1, 0, 1, 2, INT32_MAX};
  for (int64_t A : As)
    for (int S : Ss)
      for (int m : ms)
        for (int c : cs) CHECK(matcha_cluster_subset_count(A, S, m, c) == want_count(A, S, m, c));
  CHECK(matcha_cluster_subset_count(1, 32, 8, 0) == 10518300);
  CHECK(matcha_cluster_subset_count(3, 9, 1, 1) == 27);
  CHECK(matcha_cluster_subset_count(3, 2, 3, 0) == 0);
  CHECK(matcha_cluster_subset_count(INT64_MAX / 10518300, 32, 8, 0) == INT64_MAX / 10518300 * 10518300);
  CHECK(matcha_cluster_subset_count(INT64_MAX / 10518300 + 1, 32, 8, 0) == -1);                  // >= 2^63: refused, not truncated

  int64_t host[8] = {0};
  int32_t hflag[8] = {0};
  float hval[8] = {0};
  int64_t* const p = host;
  int32_t* const q = hflag;
  // clusters, A, S, m, complement, min_gap, rank0, ranks, count, L, x, flag
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 3, 0, 1, 0, nullptr, 4, 3, nullptr, q, nullptr), "null output"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 3, 0, 1, 0, nullptr, 4, 3, p, nullptr, nullptr), "null output"));
  CHECK(refused(matcha_cluster_subset_rows(nullptr, 4, 9, 3, 0, 1, 0, nullptr, 4, 3, p, q, nullptr), "null clusters"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 1, 2, 0, 1, 0, nullptr, 0, 2, p, q, nullptr), "S"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 33, 2, 0, 1, 0, nullptr, 4, 2, p, q, nullptr), "S"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 1, 0, 1, 0, nullptr, 4, 2, p, q, nullptr), "keep"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 0, 1, 1, 0, nullptr, 4, 9, p, q, nullptr), "drop"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 9, 0, 1, 0, nullptr, 4, 9, p, q, nullptr), "m"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 9, 1, 1, 0, nullptr, 4, 9, p, q, nullptr), "m"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 3, 2, 1, 0, nullptr, 4, 9, p, q, nullptr), "complement"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 3, -1, 1, 0, nullptr, 4, 9, p, q, nullptr), "complement"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 3, 0, 0, 0, nullptr, 4, 3, p, q, nullptr), "min_gap"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 3, 0, 1, 0, nullptr, 4, 2, p, q, nullptr), "width"));       // keep: L < m
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 3, 0, 1, 0, nullptr, 4, 33, p, q, nullptr), "width"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 2, 1, 1, 0, nullptr, 4, 6, p, q, nullptr), "width"));       // drop: L < S - m
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 2, 1, 1, 0, nullptr, 4, INT32_MAX, p, q, nullptr), "width"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 2, 8, 1, 1, 0, nullptr, 0, 0, p, q, nullptr), "width"));       // drop, S - m < 1: L >= 1
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 1, 1, 1, 34, nullptr, 4, 9, p, q, nullptr), "outside"));    // 4 * 9 global ranks
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 1, 1, 1, -1, nullptr, 1, 9, p, q, nullptr), "outside"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 1, 1, 1, INT64_MAX, nullptr, 1, 9, p, q, nullptr), "outside"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 1, 1, 1, 0, nullptr, -1, 9, p, q, nullptr), "count"));
  CHECK(refused(matcha_cluster_subset_rows(p, 4, 9, 1, 1, 1, 0, nullptr, INT64_MAX, 9, p, q, nullptr), "count"));
  CHECK(refused(matcha_cluster_subset_rows(p, INT64_MAX, 32, 8, 0, 1, 0, nullptr, 1, 8, p, q, nullptr), "63 bits"));
  CHECK(refused(matcha_cluster_subset_rows(p, -1, 9, 3, 0, 1, 0, nullptr, 0, 3, p, q, nullptr), "A"));
  // no-ops: accepted, nothing launched
  CHECK(matcha_cluster_subset_rows(p, 4, 9, 3, 0, 1, 0, nullptr, 0, 3, nullptr, nullptr, nullptr) == MATCHA_OK);
  CHECK(matcha_cluster_subset_rows(p, 4, 9, 3, 0, 1, 4 * 84, nullptr, 0, 3, nullptr, nullptr, nullptr) == MATCHA_OK);
  CHECK(matcha_cluster_subset_rows(nullptr, 0, 9, 3, 0, 1, 0, nullptr, 0, 3, nullptr, nullptr, nullptr) == MATCHA_OK);
  CHECK(matcha_cluster_subset_rows(p, 4, 9, 3, 1, 1, 0, p, 0, 6, nullptr, nullptr, nullptr) == MATCHA_OK);      // an empty rank list
  CHECK(matcha_cluster_subset_rows(p, 4, 2, 3, 0, 1, 0, nullptr, 0, 3, nullptr, nullptr, nullptr) == MATCHA_OK); // m > S: no candidates

  // the support state: sizes, refusals, no-ops
  CHECK(matcha_subset_support_bytes(5, 32, 8, 1.f) == 256 + 2 * 1280);
  CHECK(matcha_subset_support_bytes(1, 2, 1, 1048576.f) == 256 + 2 * 256);
  CHECK(matcha_subset_support_bytes(0, 9, 3, 1.f) == 0 && matcha_subset_support_bytes(5, 1, 1, 1.f) == 0 && matcha_subset_support_bytes(5, 33, 1, 1.f) == 0);
  CHECK(matcha_subset_support_bytes(5, 9, 0, 1.f) == 0 && matcha_subset_support_bytes(5, 9, 9, 1.f) == 0 && matcha_subset_support_bytes(5, 9, 3, 0.f) == 0);
  CHECK(matcha_subset_support_bytes(5, 9, 3, -1.f) == 0 && matcha_subset_support_bytes(5, 9, 3, 2097152.f) == 0 && matcha_subset_support_bytes(5, 9, 3, NAN) == 0);
  CHECK(matcha_subset_support_bytes(((int64_t)1 << 40) + 1, 9, 3, 1.f) == 0 && matcha_subset_support_bytes(INT64_MAX, 32, 8, 1.f) == 0);
  const size_t need = matcha_subset_support_bytes(4, 9, 3, 1.f);
  CHECK(refused(matcha_subset_support_init(nullptr, need, 4, 9, 3, 1.f, nullptr), "null state"));
  CHECK(refused(matcha_subset_support_init(p, need - 1, 4, 9, 3, 1.f, nullptr), "too small"));
  CHECK(refused(matcha_subset_support_init(p, need, 4, 1, 3, 1.f, nullptr), "S"));
  CHECK(refused(matcha_subset_support_init((char*)p + 4, need, 4, 9, 3, 1.f, nullptr), "aligned"));
  CHECK(refused(matcha_subset_support_update(nullptr, need, 4, 9, 3, 1.f, hval, q, 4, 0, nullptr), "null state"));
  CHECK(refused(matcha_subset_support_update(p, need - 1, 4, 9, 3, 1.f, hval, q, 4, 0, nullptr), "too small"));
  CHECK(refused(matcha_subset_support_update(p, need, 4, 9, 3, NAN, hval, q, 4, 0, nullptr), "vmax"));
  CHECK(refused(matcha_subset_support_update(p, need, 4, 9, 3, 1.f, nullptr, q, 4, 0, nullptr), "null value"));
  CHECK(refused(matcha_subset_support_update(p, need, 4, 9, 3, 1.f, hval, q, -1, 0, nullptr), "n="));
  CHECK(refused(matcha_subset_support_update(p, need, 4, 9, 3, 1.f, hval, q, INT64_MAX, 0, nullptr), "n="));
  CHECK(refused(matcha_subset_support_update(p, need, 4, 9, 3, 1.f, hval, q, 4, 4 * 84 - 3, nullptr), "outside"));
  CHECK(refused(matcha_subset_support_update(p, need, 4, 9, 3, 1.f, hval, q, 1, -1, nullptr), "outside"));
  CHECK(refused(matcha_subset_support_update(p, need, 4, 9, 3, 1.f, hval, q, 1, INT64_MAX, nullptr), "outside"));
  CHECK(matcha_subset_support_update(p, need, 4, 9, 3, 1.f, nullptr, nullptr, 0, 0, nullptr) == MATCHA_OK);
  CHECK(matcha_subset_support_update(p, need, 4, 9, 3, 1.f, hval, q, 0, 4 * 84, nullptr) == MATCHA_OK);
  CHECK(refused(matcha_subset_support_read(nullptr, need, 4, 9, 3, 1.f, p, p, p, nullptr), "null state"));
  CHECK(refused(matcha_subset_support_read(p, need - 1, 4, 9, 3, 1.f, p, p, p, nullptr), "too small"));
  CHECK(refused(matcha_subset_support_read(p, need, 4, 9, 3, 1.f, nullptr, nullptr, nullptr, nullptr), "null output"));

  return finish("CLUSTER DECOMPOSITION HOST CHECKS");
}
