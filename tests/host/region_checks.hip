// The multi-region sweep's host side (csrc/sweep_rows.hip: matcha_kway_region_count and the argument checks of matcha_kway_region_rows,
// DESIGN.md 7.14) under AddressSanitizer + UndefinedBehaviorSanitizer on the host, next to tests/host/grow_checks.hip: the same
// host-only objects, model.hip included as source for the library's error and option plumbing, a driver of its own.  The three part
// arrays are host memory of exactly P elements, so a read past them is an ASan report; no kernel runs: every rows call below is refused,
// or is a no-op, before any device call, and x / flag / ranks are never dereferenced.
#include <vector>

#include "host_driver.hpp"

struct Parts {
  std::vector<int64_t> lo;
  std::vector<int32_t> n, m;
  Parts(std::vector<int64_t> lo_, std::vector<int32_t> n_, std::vector<int32_t> m_) : lo(lo_), n(n_), m(m_) {}
  int32_t P() const { return (int32_t)lo.size(); }
};

static int64_t count(const Parts& s, int32_t gap) { return matcha_kway_region_count(s.P(), s.lo.data(), s.n.data(), s.m.data(), gap); }
static int rows(const Parts& s, int32_t gap, int64_t rank0, const int64_t* ranks, int64_t cnt, int32_t L, int64_t* x, int32_t* flag) {
  return matcha_kway_region_rows(s.P(), s.lo.data(), s.n.data(), s.m.data(), gap, rank0, ranks, cnt, L, x, flag, nullptr);
}

int main() {
  int64_t host[8] = {0};
  int32_t hflag[8] = {0};
  int64_t* const p = host;
  int32_t* const q = hflag;
  const Parts two({1, 33}, {16, 16}, {1, 2});                            // 16 C(16, 2) = 1920
  const Parts touch({17, 23}, {6, 10}, {2, 2});                          // gap 3: C(4, 2) C(8, 2) = 168
  const Parts eight({1, 201, 401, 601, 801, 1001, 1201, 1401}, {200, 200, 200, 200, 200, 200, 200, 200}, {1, 1, 1, 1, 1, 1, 1, 1});
  const Parts one8({5}, {30}, {8});
  // ---- counts ----
  CHECK(count(two, 1) == 1920);
  CHECK(count(two, 2) == 16 * 105);
  CHECK(count(touch, 3) == 168);
  CHECK(count(eight, 1) == 2560000000000000000ll);                       // 200^8 = 2.56e18 < 2^63
  CHECK(count(eight, 7) == 2560000000000000000ll);                       // single bins: the gap does not enter
  CHECK(count(one8, 1) == 5852925);                                      // C(30, 8)
  CHECK(count(one8, 4) == 9);                                            // C(30 - 21, 8)
  CHECK(count(one8, 5) == 0);                                            // C(2, 8): nothing fits
  CHECK(count(Parts({1, 40}, {6, 16}, {3, 2}), 4) == 0);                 // C(0, 3) = 0 in one part: T = 0
  CHECK(count(Parts({1, 40}, {2, 16}, {3, 2}), 4) == 0);                 // n - (m - 1)(gap - 1) < 0
  CHECK(count(Parts({0, 1 << 20}, {1 << 20, 1 << 20}, {1, 1}), 1) == (int64_t)1 << 40);
  // T >= 2^63 is -1, never truncated: 2^21 bins x 2 parts x ... and one part whose own count overflows
  CHECK(count(Parts({0, (int64_t)1 << 31, (int64_t)1 << 32}, {1 << 21, 1 << 21, 1 << 21}, {1, 1, 1}), 1) == -1);   // 2^63 exactly
  CHECK(count(Parts({0, (int64_t)1 << 31, (int64_t)1 << 32}, {1 << 21, 1 << 21, (1 << 21) - 1}, {1, 1, 1}), 1) == ((int64_t)1 << 42) * ((1 << 21) - 1));
  CHECK(count(Parts({0}, {INT32_MAX}, {8}), 1) == -1);                   // C(2^31 - 1, 8) alone
  CHECK(count(Parts({0, (int64_t)1 << 31}, {INT32_MAX, INT32_MAX}, {4, 4}), 1) == -1);
  CHECK(count(Parts({0, (int64_t)1 << 31}, {INT32_MAX, 3}, {6, 2}), 5) == -1);      // an overflowing part beside an empty one is still refused
  // invalid arguments
  CHECK(matcha_kway_region_count(0, two.lo.data(), two.n.data(), two.m.data(), 1) == -1);
  CHECK(matcha_kway_region_count(9, two.lo.data(), two.n.data(), two.m.data(), 1) == -1);
  CHECK(matcha_kway_region_count(INT32_MIN, two.lo.data(), two.n.data(), two.m.data(), 1) == -1);
  CHECK(matcha_kway_region_count(2, nullptr, two.n.data(), two.m.data(), 1) == -1);
  CHECK(matcha_kway_region_count(2, two.lo.data(), nullptr, two.m.data(), 1) == -1);
  CHECK(matcha_kway_region_count(2, two.lo.data(), two.n.data(), nullptr, 1) == -1);
  CHECK(count(two, 0) == -1);
  CHECK(count(two, INT32_MIN) == -1);
  CHECK(count(Parts({1, 33}, {16, 16}, {0, 2}), 1) == -1);
  CHECK(count(Parts({1, 33}, {16, 0}, {1, 2}), 1) == -1);
  CHECK(count(Parts({1, 33}, {16, INT32_MIN}, {1, 2}), 1) == -1);
  CHECK(count(Parts({1}, {16}, {1}), 1) == -1);                          // k = 1
  CHECK(count(Parts({1, 33}, {16, 16}, {4, 5}), 1) == -1);               // k = 9
  CHECK(count(Parts({1, 33}, {16, 16}, {INT32_MAX, INT32_MAX}), 1) == -1);
  CHECK(count(Parts({1, 16}, {16, 16}, {1, 2}), 1) == -1);               // overlap by one bin
  CHECK(count(Parts({33, 1}, {16, 16}, {1, 2}), 1) == -1);               // descending
  CHECK(count(Parts({1, 17}, {16, 16}, {1, 2}), 1) == 1920);             // touching is fine
  CHECK(count(Parts({-1, 33}, {16, 16}, {1, 2}), 1) == -1);
  CHECK(count(Parts({1, INT64_MAX}, {16, 16}, {1, 2}), 1) == -1);
  CHECK(count(Parts({1, INT64_MAX - 3}, {16, 16}, {1, 2}), 1) == -1);
  // ---- rows: every refusal, before any device call ----
  CHECK(refused(matcha_kway_region_rows(0, two.lo.data(), two.n.data(), two.m.data(), 1, 0, nullptr, 4, 3, p, q, nullptr), "P="));
  CHECK(refused(matcha_kway_region_rows(9, two.lo.data(), two.n.data(), two.m.data(), 1, 0, nullptr, 4, 3, p, q, nullptr), "P="));
  CHECK(refused(matcha_kway_region_rows(2, nullptr, two.n.data(), two.m.data(), 1, 0, nullptr, 4, 3, p, q, nullptr), "null part"));
  CHECK(refused(matcha_kway_region_rows(2, two.lo.data(), nullptr, two.m.data(), 1, 0, nullptr, 4, 3, p, q, nullptr), "null part"));
  CHECK(refused(matcha_kway_region_rows(2, two.lo.data(), two.n.data(), nullptr, 1, 0, nullptr, 4, 3, p, q, nullptr), "null part"));
  CHECK(refused(rows(two, 0, 0, nullptr, 4, 3, p, q), "min_gap"));
  CHECK(refused(rows(Parts({1, 33}, {16, 16}, {0, 2}), 1, 0, nullptr, 4, 3, p, q), "m=0"));
  CHECK(refused(rows(Parts({1, 33}, {16, 0}, {1, 2}), 1, 0, nullptr, 4, 3, p, q), "n=0"));
  CHECK(refused(rows(Parts({1}, {16}, {1}), 1, 0, nullptr, 4, 3, p, q), "k=1"));
  CHECK(refused(rows(Parts({1, 33}, {16, 16}, {4, 5}), 1, 0, nullptr, 4, 8, p, q), "k=9"));
  CHECK(refused(rows(Parts({1, 33}, {16, 16}, {INT32_MAX, INT32_MAX}), 1, 0, nullptr, 4, 8, p, q), "k="));
  CHECK(refused(rows(Parts({1, 16}, {16, 16}, {1, 2}), 1, 0, nullptr, 4, 3, p, q), "ascending and disjoint"));
  CHECK(refused(rows(Parts({33, 1}, {16, 16}, {1, 2}), 1, 0, nullptr, 4, 3, p, q), "ascending and disjoint"));
  CHECK(refused(rows(Parts({-1, 33}, {16, 16}, {1, 2}), 1, 0, nullptr, 4, 3, p, q), "lo of part 0"));
  CHECK(refused(rows(Parts({1, INT64_MAX}, {16, 16}, {1, 2}), 1, 0, nullptr, 4, 3, p, q), "lo of part 1"));
  CHECK(refused(rows(two, 1, 0, nullptr, 4, 2, p, q), "L=2"));
  CHECK(refused(rows(two, 1, 0, nullptr, 4, 9, p, q), "L=9"));
  CHECK(refused(rows(Parts({0, (int64_t)1 << 31, (int64_t)1 << 32}, {1 << 21, 1 << 21, 1 << 21}, {1, 1, 1}), 1, 0, nullptr, 4, 3, p, q), "63 bits"));
  CHECK(refused(rows(Parts({0}, {INT32_MAX}, {8}), 1, 0, nullptr, 4, 8, p, q), "63 bits"));
  CHECK(refused(rows(two, 1, 1918, nullptr, 4, 3, p, q), "outside"));
  CHECK(refused(rows(two, 1, -1, nullptr, 1, 3, p, q), "outside"));
  CHECK(refused(rows(two, 1, INT64_MAX, nullptr, 1, 3, p, q), "outside"));
  CHECK(refused(rows(two, 1, 1921, nullptr, 0, 3, p, q), "outside"));
  CHECK(refused(rows(one8, 5, 0, nullptr, 1, 8, p, q), "outside"));       // T = 0: no rank exists
  CHECK(refused(rows(two, 1, 0, nullptr, -1, 3, p, q), "count"));
  CHECK(refused(rows(two, 1, 0, p, ((int64_t)1 << 40) + 1, 3, p, q), "count"));
  CHECK(refused(rows(two, 1, 0, p, INT64_MAX, 3, p, q), "count"));
  CHECK(refused(rows(two, 1, 0, nullptr, 4, 3, nullptr, q), "null output"));
  CHECK(refused(rows(two, 1, 0, nullptr, 4, 3, p, nullptr), "null output"));
  CHECK(refused(rows(two, 1, 0, p, 4, 3, nullptr, nullptr), "null output"));
  // no-ops: accepted, nothing launched
  CHECK(rows(two, 1, 0, nullptr, 0, 3, nullptr, nullptr) == MATCHA_OK);
  CHECK(rows(two, 1, 1920, nullptr, 0, 8, nullptr, nullptr) == MATCHA_OK);
  CHECK(rows(two, 1, 0, p, 0, 3, nullptr, nullptr) == MATCHA_OK);
  CHECK(rows(eight, 1, 2560000000000000000ll, nullptr, 0, 8, nullptr, nullptr) == MATCHA_OK);
  CHECK(rows(one8, 5, 0, nullptr, 0, 8, nullptr, nullptr) == MATCHA_OK);

  return finish("MULTI-REGION HOST CHECKS");
}
