// Cluster growth's host side (csrc/grow.hip: the argument checks of matcha_grow_twins and matcha_grow_twin_flags) under
// AddressSanitizer + UndefinedBehaviorSanitizer on the host, next to tests/host/complete_checks.hip: the same host-only objects, model.hip
// included as source for the library's error and option plumbing, a driver of its own.  No kernel runs: every call below is refused, or is
// a no-op, before any device call, on pointers that are never dereferenced.
#include "host_driver.hpp"

int main() {
  int64_t host[8] = {0};
  int32_t hflag[8] = {0};
  int64_t* const p = host;
  int32_t* const q = hflag;
  // beam, A, B, S, twin
  CHECK(refused(matcha_grow_twins(p, 4, 0, 9, p, nullptr), "B="));
  CHECK(refused(matcha_grow_twins(p, 4, 65, 9, p, nullptr), "B="));
  CHECK(refused(matcha_grow_twins(p, 4, INT32_MIN, 9, p, nullptr), "B="));
  CHECK(refused(matcha_grow_twins(p, 4, INT32_MAX, 9, p, nullptr), "B="));
  CHECK(refused(matcha_grow_twins(p, 4, 8, 0, p, nullptr), "S="));
  CHECK(refused(matcha_grow_twins(p, 4, 8, 32, p, nullptr), "S="));
  CHECK(refused(matcha_grow_twins(p, 4, 8, INT32_MAX, p, nullptr), "S="));
  CHECK(refused(matcha_grow_twins(p, -1, 8, 9, p, nullptr), "A="));
  CHECK(refused(matcha_grow_twins(p, INT64_MAX, 8, 9, p, nullptr), "A="));
  CHECK(refused(matcha_grow_twins(nullptr, 4, 8, 9, p, nullptr), "null beam"));
  CHECK(refused(matcha_grow_twins(p, 4, 8, 9, nullptr, nullptr), "null output"));
  CHECK(matcha_grow_twins(nullptr, 0, 8, 9, nullptr, nullptr) == MATCHA_OK);
  // twin, A, B, lo, n, rank0, count, flag
  CHECK(refused(matcha_grow_twin_flags(p, 4, 0, 1, 16, 0, 4, q, nullptr), "B="));
  CHECK(refused(matcha_grow_twin_flags(p, 4, 65, 1, 16, 0, 4, q, nullptr), "B="));
  CHECK(refused(matcha_grow_twin_flags(p, 4, 8, 1, 0, 0, 0, q, nullptr), "n="));
  CHECK(refused(matcha_grow_twin_flags(p, 4, 8, 1, INT32_MIN, 0, 0, q, nullptr), "n="));
  CHECK(refused(matcha_grow_twin_flags(p, -1, 8, 1, 16, 0, 0, q, nullptr), "A="));
  CHECK(refused(matcha_grow_twin_flags(p, 4, 8, -1, 16, 0, 4, q, nullptr), "lo"));
  CHECK(refused(matcha_grow_twin_flags(p, 4, 8, INT64_MAX, 16, 0, 4, q, nullptr), "lo"));
  CHECK(refused(matcha_grow_twin_flags(p, (int64_t)1 << 40, 64, 1, 1 << 17, 0, 1, q, nullptr), "63 bits"));       // 2^40 2^6 2^17 = 2^63
  CHECK(refused(matcha_grow_twin_flags(p, INT64_MAX, 64, 1, INT32_MAX, 0, 1, q, nullptr), "63 bits"));
  CHECK(refused(matcha_grow_twin_flags(p, 4, 8, 1, 16, 510, 4, q, nullptr), "outside"));                          // 4 * 8 * 16 = 512 ranks
  CHECK(refused(matcha_grow_twin_flags(p, 4, 8, 1, 16, -1, 1, q, nullptr), "outside"));
  CHECK(refused(matcha_grow_twin_flags(p, 4, 8, 1, 16, INT64_MAX, 1, q, nullptr), "outside"));
  CHECK(refused(matcha_grow_twin_flags(p, 4, 8, 1, 16, 513, 0, q, nullptr), "outside"));
  CHECK(refused(matcha_grow_twin_flags(p, 4, 8, 1, 16, 0, -1, q, nullptr), "count"));
  CHECK(refused(matcha_grow_twin_flags(p, 4, 8, 1, 16, 0, INT64_MAX, q, nullptr), "count"));
  CHECK(refused(matcha_grow_twin_flags(nullptr, 4, 8, 1, 16, 0, 4, q, nullptr), "null twin"));
  CHECK(refused(matcha_grow_twin_flags(p, 4, 8, 1, 16, 0, 4, nullptr, nullptr), "null flag"));
  // no-ops: accepted, nothing launched
  CHECK(matcha_grow_twin_flags(p, 4, 8, 1, 16, 0, 0, nullptr, nullptr) == MATCHA_OK);
  CHECK(matcha_grow_twin_flags(p, 4, 8, 1, 16, 512, 0, nullptr, nullptr) == MATCHA_OK);
  CHECK(matcha_grow_twin_flags(nullptr, 0, 8, 1, 16, 0, 0, nullptr, nullptr) == MATCHA_OK);
  CHECK(matcha_grow_twin_flags(p, ((int64_t)1 << 40) - 1, 64, 1, 1 << 17, 0, 0, nullptr, nullptr) == MATCHA_OK);  // just below 2^63

  return finish("CLUSTER GROWTH HOST CHECKS");
}
