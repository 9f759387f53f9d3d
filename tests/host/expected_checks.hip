// The host side of the distance-matched expectation (csrc/expected.hip: matcha_gap_strata_count, matcha_gap_stats_bytes and the argument
// checks of the five launching entry points) under AddressSanitizer + UndefinedBehaviorSanitizer on the host, next to
// tests/host/region_checks.hip: the same host-only objects, model.hip included as source for the library's error and option plumbing, a
// driver of its own.  The edge arrays are host memory of exactly n_edges elements, so a read past them is an ASan report; no kernel runs:
// every launching call below is refused, or is a no-op, before any device call, and state / x / value are never dereferenced.
#include <vector>

#include "host_driver.hpp"

static int64_t ipow(int64_t b, int e) {
  int64_t r = 1;
  while (e-- > 0) r *= b;
  return r;
}

int main() {
  alignas(8) static char blob[8] = {0};
  void* const st = blob;                                                  // a non-null, aligned state that is never dereferenced
  int64_t rows[8] = {0};
  float vals[8] = {0};
  int32_t ids[8] = {0};
  const std::vector<int64_t> e3{2, 4, 8};
  std::vector<int64_t> e15;
  for (int j = 0; j < 15; ++j) e15.push_back(2 + 3 * j);
  std::vector<int64_t> e16(e15);
  e16.push_back(1000);

  // ---- matcha_gap_strata_count: G^(k-1) up to the 2^20 boundary ----
  for (int k = 2; k <= 8; ++k)
    for (int ne = 0; ne <= 15; ++ne) {
      const int64_t want = ipow(ne + 1, k - 1);
      CHECK(matcha_gap_strata_count(k, ne) == (want <= (1 << 20) ? want : -1));
    }
  CHECK(matcha_gap_strata_count(3, 3) == 16 && matcha_gap_strata_count(5, 15) == 65536);
  CHECK(matcha_gap_strata_count(6, 15) == 1 << 20);                       // 16^5: exactly the boundary
  CHECK(matcha_gap_strata_count(7, 15) == -1 && matcha_gap_strata_count(8, 7) == -1 && matcha_gap_strata_count(8, 6) == 823543);
  CHECK(matcha_gap_strata_count(5, 31) == -1);                            // 32^4 = 2^20, but 31 edges are too many
  CHECK(matcha_gap_strata_count(1, 3) == -1 && matcha_gap_strata_count(9, 0) == -1 && matcha_gap_strata_count(INT32_MIN, 0) == -1);
  CHECK(matcha_gap_strata_count(3, -1) == -1 && matcha_gap_strata_count(3, 16) == -1 && matcha_gap_strata_count(3, INT32_MAX) == -1);
  CHECK(matcha_gap_strata_count(8, 0) == 1);

  // ---- matcha_gap_stats_bytes: a 256-byte header, then every plane present padded to 256 bytes ----
  auto pad = [](int64_t n) { return (size_t)((n * 8 + 255) / 256 * 256); };
  for (int k = 2; k <= 8; ++k)
    for (int ne = 0; ne <= 15; ++ne)
      for (int planes = 0; planes <= 16; ++planes) {
        const int64_t ns = matcha_gap_strata_count(k, ne);
        const bool ok = ns > 0 && (planes & 7) != 0 && planes < 16;
        const int held = (planes & 1) + ((planes >> 1) & 1) + ((planes >> 2) & 1);
        CHECK(matcha_gap_stats_bytes(k, ne, planes) == (ok ? 256 + held * pad(ns) : 0));
      }
  CHECK(matcha_gap_stats_bytes(3, 3, 7) == 256 + 3 * 256);                // 16 strata: 128 bytes, padded
  CHECK(matcha_gap_stats_bytes(6, 15, 7) == 256 + 3 * ((size_t)8 << 20)); // three planes of 8 MiB
  CHECK(matcha_gap_stats_bytes(3, 3, 15) == matcha_gap_stats_bytes(3, 3, 7));      // DIRECT takes no memory
  CHECK(matcha_gap_stats_bytes(3, 3, 8) == 0 && matcha_gap_stats_bytes(3, 3, -1) == 0 && matcha_gap_stats_bytes(3, 3, INT32_MIN) == 0);
  CHECK(matcha_gap_stats_bytes(7, 15, 1) == 0 && matcha_gap_stats_bytes(1, 3, 1) == 0 && matcha_gap_stats_bytes(3, 16, 1) == 0);

  const size_t b3 = matcha_gap_stats_bytes(3, 3, 7);
  // ---- init ----
  CHECK(refused(matcha_gap_stats_init(st, b3, 1, 3, 7, nullptr), "k=1"));
  CHECK(refused(matcha_gap_stats_init(st, b3, 9, 3, 7, nullptr), "k=9"));
  CHECK(refused(matcha_gap_stats_init(st, b3, 3, 16, 7, nullptr), "n_edges=16"));
  CHECK(refused(matcha_gap_stats_init(st, b3, 3, -1, 7, nullptr), "n_edges=-1"));
  CHECK(refused(matcha_gap_stats_init(st, b3, 7, 15, 7, nullptr), "2^20"));
  CHECK(refused(matcha_gap_stats_init(st, b3, 3, 3, 0, nullptr), "planes=0"));
  CHECK(refused(matcha_gap_stats_init(st, b3, 3, 3, 8, nullptr), "planes=8"));       // DIRECT alone holds no plane
  CHECK(refused(matcha_gap_stats_init(st, b3, 3, 3, 16, nullptr), "planes=16"));
  CHECK(refused(matcha_gap_stats_init(st, b3, 3, 3, -1, nullptr), "planes=-1"));
  CHECK(refused(matcha_gap_stats_init(nullptr, b3, 3, 3, 7, nullptr), "null state"));
  CHECK(refused(matcha_gap_stats_init(blob + 4, b3, 3, 3, 7, nullptr), "aligned"));
  CHECK(refused(matcha_gap_stats_init(st, b3 - 1, 3, 3, 7, nullptr), "matcha_gap_stats_bytes says"));
  CHECK(refused(matcha_gap_stats_init(st, b3 + 256, 3, 3, 7, nullptr), "matcha_gap_stats_bytes says"));
  CHECK(refused(matcha_gap_stats_init(st, b3, 3, 3, 3, nullptr), "matcha_gap_stats_bytes says"));       // another mask, another size
  CHECK(refused(matcha_gap_stats_init(st, 0, 3, 3, 7, nullptr), "matcha_gap_stats_bytes says"));

  // ---- update ----
  auto update = [&](int k, const int64_t* edges, int ne, int planes, int shift, float vmax, int L, int64_t n, void* state = nullptr, size_t bytes = 0,
                    const int64_t* x = nullptr, const float* v = nullptr) {
    return matcha_gap_stats_update(state ? state : st, bytes ? bytes : matcha_gap_stats_bytes(k, ne, planes), k, edges, ne, planes, shift, vmax,
                                   x ? x : rows, L, v ? v : vals, nullptr, n, nullptr);
  };
  CHECK(refused(matcha_gap_stats_update(st, b3, 1, e3.data(), 3, 7, 32, 1.f, rows, 3, vals, nullptr, 4, nullptr), "k=1"));
  CHECK(refused(matcha_gap_stats_update(st, b3, 9, e3.data(), 3, 7, 32, 1.f, rows, 8, vals, nullptr, 4, nullptr), "k=9"));
  CHECK(refused(update(3, e3.data(), 3, 7, 32, 1.f, 2, 4), "L=2"));        // L < k
  CHECK(refused(update(3, e3.data(), 3, 7, 32, 1.f, 9, 4), "L=9"));
  CHECK(refused(update(2, e3.data(), 3, 7, 32, 1.f, 1, 4), "L=1"));
  CHECK(refused(matcha_gap_stats_update(st, b3, 3, e16.data(), 16, 7, 32, 1.f, rows, 3, vals, nullptr, 4, nullptr), "n_edges=16"));
  CHECK(refused(matcha_gap_stats_update(st, b3, 7, e15.data(), 15, 7, 32, 1.f, rows, 8, vals, nullptr, 4, nullptr), "2^20"));
  {
    const std::vector<int64_t> same{2, 4, 4}, down{2, 8, 4}, zero{0, 4, 8}, neg{-3, 4, 8}, huge{2, 4, INT64_MAX};
    for (const auto* bad : {&same, &down, &zero, &neg, &huge}) CHECK(refused(update(3, bad->data(), 3, 7, 32, 1.f, 3, 4), "strictly ascending"));
    CHECK(refused(update(3, nullptr, 3, 7, 32, 1.f, 3, 4), "strictly ascending"));       // edges announced, none given
  }
  CHECK(refused(update(3, e3.data(), 3, 0, 32, 1.f, 3, 4, st, b3), "planes=0"));
  CHECK(refused(update(3, e3.data(), 3, 8, 32, 1.f, 3, 4, st, b3), "planes=8"));
  CHECK(refused(update(3, e3.data(), 3, 16, 32, 1.f, 3, 4, st, b3), "planes=16"));
  CHECK(refused(update(3, e3.data(), 3, 7, 15, 1.f, 3, 4), "shift=15"));
  CHECK(refused(update(3, e3.data(), 3, 7, 33, 1.f, 3, 4), "shift=33"));
  CHECK(refused(update(3, e3.data(), 3, 7, INT32_MIN, 1.f, 3, 4), "shift="));
  CHECK(refused(update(3, e3.data(), 3, 7, 32, 0.f, 3, 4), "vmax="));
  CHECK(refused(update(3, e3.data(), 3, 7, 32, -1.f, 3, 4), "vmax="));
  CHECK(refused(update(3, e3.data(), 3, 7, 32, 1048577.f, 3, 4), "vmax="));
  CHECK(refused(update(3, e3.data(), 3, 7, 32, NAN, 3, 4), "vmax="));
  CHECK(refused(update(3, e3.data(), 3, 7, 32, INFINITY, 3, 4), "vmax="));
  CHECK(refused(update(3, e3.data(), 3, 7, 32, 1048576.f, 3, 4), "2^62"));               // SUMSQ: 2^40 2^32 does not fit one term
  CHECK(refused(update(3, e3.data(), 3, 4, 24, 1048576.f, 3, 4), "2^62"));
  CHECK(refused(update(3, e3.data(), 3, 7, 32, 1.f, 3, -1), "n=-1"));
  CHECK(refused(update(3, e3.data(), 3, 7, 32, 1.f, 3, ((int64_t)1 << 40) + 1), "out of range"));
  CHECK(refused(matcha_gap_stats_update(st, b3 + 8, 3, e3.data(), 3, 7, 32, 1.f, rows, 3, vals, nullptr, 4, nullptr), "matcha_gap_stats_bytes says"));
  CHECK(refused(matcha_gap_stats_update(nullptr, b3, 3, e3.data(), 3, 7, 32, 1.f, rows, 3, vals, nullptr, 4, nullptr), "null state"));
  CHECK(refused(matcha_gap_stats_update(st, b3, 3, e3.data(), 3, 7, 32, 1.f, nullptr, 3, vals, nullptr, 4, nullptr), "null x or value"));
  CHECK(refused(matcha_gap_stats_update(st, b3, 3, e3.data(), 3, 7, 32, 1.f, rows, 3, nullptr, nullptr, 4, nullptr), "null x or value"));
  // accepted, nothing launched: n = 0 (the widest table, the largest vmax that SUMSQ takes at shift 16, DIRECT, no edges at all)
  CHECK(update(3, e3.data(), 3, 7, 32, 1.f, 3, 0) == MATCHA_OK);
  CHECK(update(3, e3.data(), 3, 15, 32, 1.f, 8, 0) == MATCHA_OK);
  CHECK(update(6, e15.data(), 15, 7, 16, 1048576.f, 6, 0) == MATCHA_OK);
  CHECK(update(3, e3.data(), 3, 3, 32, 1048576.f, 3, 0) == MATCHA_OK);                   // without SUMSQ the largest vmax at the largest shift
  CHECK(update(8, nullptr, 0, 7, 32, 1.f, 8, 0) == MATCHA_OK);
  CHECK(matcha_gap_stats_update(st, b3, 3, e3.data(), 3, 7, 32, 1.f, nullptr, 3, nullptr, nullptr, 0, nullptr) == MATCHA_OK);

  // ---- read ----
  int64_t* const o = rows;
  CHECK(refused(matcha_gap_stats_read(st, b3, 1, 3, 7, o, o, o, o, nullptr), "k=1"));
  CHECK(refused(matcha_gap_stats_read(st, b3, 3, 16, 7, o, o, o, o, nullptr), "n_edges=16"));
  CHECK(refused(matcha_gap_stats_read(st, b3, 7, 15, 7, o, o, o, o, nullptr), "2^20"));
  CHECK(refused(matcha_gap_stats_read(st, b3, 3, 3, 0, o, o, o, o, nullptr), "planes=0"));
  CHECK(refused(matcha_gap_stats_read(st, b3, 3, 3, 32, o, o, o, o, nullptr), "planes=32"));
  CHECK(refused(matcha_gap_stats_read(nullptr, b3, 3, 3, 7, o, o, o, o, nullptr), "null state"));
  CHECK(refused(matcha_gap_stats_read(st, b3 - 8, 3, 3, 7, o, o, o, o, nullptr), "matcha_gap_stats_bytes says"));
  CHECK(refused(matcha_gap_stats_read(st, matcha_gap_stats_bytes(3, 3, 1), 3, 3, 1, o, o, nullptr, o, nullptr), "does not hold"));
  CHECK(refused(matcha_gap_stats_read(st, matcha_gap_stats_bytes(3, 3, 6), 3, 3, 6, o, o, o, o, nullptr), "does not hold"));
  CHECK(refused(matcha_gap_stats_read(st, matcha_gap_stats_bytes(3, 3, 3), 3, 3, 3, o, o, o, nullptr, nullptr), "does not hold"));
  CHECK(refused(matcha_gap_stats_read(st, b3, 3, 3, 7, nullptr, nullptr, nullptr, nullptr, nullptr), "null outputs"));

  // ---- enrich and strata ids ----
  float* const f = vals;
  CHECK(refused(matcha_gap_enrich(1, e3.data(), 3, rows, 4, 3, f, f, f, ids, f, nullptr), "k=1"));
  CHECK(refused(matcha_gap_enrich(9, e3.data(), 3, rows, 4, 8, f, f, f, ids, f, nullptr), "k=9"));
  CHECK(refused(matcha_gap_enrich(3, e3.data(), 3, rows, 4, 2, f, f, f, ids, f, nullptr), "L=2"));
  CHECK(refused(matcha_gap_enrich(3, e3.data(), 3, rows, 4, 9, f, f, f, ids, f, nullptr), "L=9"));
  CHECK(refused(matcha_gap_enrich(3, e16.data(), 16, rows, 4, 3, f, f, f, ids, f, nullptr), "n_edges=16"));
  CHECK(refused(matcha_gap_enrich(7, e15.data(), 15, rows, 4, 8, f, f, f, ids, f, nullptr), "2^20"));
  {
    const std::vector<int64_t> down{8, 4, 2}, zero{0};
    CHECK(refused(matcha_gap_enrich(3, down.data(), 3, rows, 4, 3, f, f, f, ids, f, nullptr), "strictly ascending"));
    CHECK(refused(matcha_gap_enrich(3, zero.data(), 1, rows, 4, 3, f, f, f, ids, f, nullptr), "strictly ascending"));
  }
  CHECK(refused(matcha_gap_enrich(3, e3.data(), 3, rows, -1, 3, f, f, f, ids, f, nullptr), "n=-1"));
  CHECK(refused(matcha_gap_enrich(3, e3.data(), 3, rows, 4, 3, f, nullptr, f, ids, f, nullptr), "go together"));
  CHECK(refused(matcha_gap_enrich(3, e3.data(), 3, rows, 4, 3, f, f, nullptr, ids, f, nullptr), "go together"));
  CHECK(refused(matcha_gap_enrich(3, e3.data(), 3, rows, 4, 3, f, f, f, ids, nullptr, nullptr), "go together"));
  CHECK(refused(matcha_gap_enrich(3, e3.data(), 3, rows, 4, 3, nullptr, f, f, ids, nullptr, nullptr), "go together"));
  CHECK(refused(matcha_gap_enrich(3, e3.data(), 3, rows, 4, 3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "go together"));
  CHECK(refused(matcha_gap_enrich(3, e3.data(), 3, nullptr, 4, 3, f, f, f, ids, f, nullptr), "null x"));
  CHECK(matcha_gap_enrich(3, e3.data(), 3, nullptr, 0, 3, f, f, f, nullptr, f, nullptr) == MATCHA_OK);
  CHECK(matcha_gap_enrich(6, e15.data(), 15, nullptr, 0, 8, nullptr, nullptr, nullptr, ids, nullptr, nullptr) == MATCHA_OK);
  CHECK(refused(matcha_gap_strata_ids(3, e3.data(), 3, rows, 4, 3, nullptr, nullptr), "null stratum_out"));
  CHECK(refused(matcha_gap_strata_ids(3, e3.data(), 3, rows, 4, 2, ids, nullptr), "L=2"));
  CHECK(refused(matcha_gap_strata_ids(7, e15.data(), 15, rows, 4, 8, ids, nullptr), "2^20"));
  CHECK(refused(matcha_gap_strata_ids(3, e3.data(), 3, nullptr, 4, 3, ids, nullptr), "null x"));
  CHECK(matcha_gap_strata_ids(3, e3.data(), 3, nullptr, 0, 3, ids, nullptr) == MATCHA_OK);
  CHECK(matcha_gap_strata_ids(2, nullptr, 0, nullptr, 0, 2, ids, nullptr) == MATCHA_OK);

  return finish("EXPECTATION HOST CHECKS");
}
