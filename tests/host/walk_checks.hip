// The argument validation of the hypergraph walk (matcha_hyper_walk, csrc/walk.hip) and of the skip-gram pass (matcha_sgns_epoch,
// csrc/sgns.hip) under AddressSanitizer + UndefinedBehaviorSanitizer on the host, next to tests/host/outlier_checks.hip: the
// same host-only objects, model.hip included as source for the library's error plumbing, a driver of its own.  No kernel runs: every call
// below is refused, or is a no-op, before any device call, on pointers that are never dereferenced (thresholds, a HOST array, is read).
#include "host_driver.hpp"

static void hyper_walk_checks() {
  int64_t host[8] = {0};
  int32_t hint[8] = {0};
  uint64_t cum[8] = {0};
  uint64_t seed = 1;
  int64_t* const e = host;            // inc_ptr, the sets' edge lists
  int32_t* const q = hint;            // inc_nb, the sets' tables, nodes, out, status
  const int64_t A = (int64_t)1 << 32, M = ((int64_t)1 << 31) - 1;
  int64_t thr[3] = {A / 8, A / 4, A};
  // pair set (n, L), triple set (n, L), thresholds, n_start, w0, w1, walk_length, max_trials
  auto call = [&](const int64_t* ptr, const int32_t* nb, const uint64_t* cm, int32_t n_nodes, const void* ps, const int64_t* pe, int64_t np, int32_t lp,
                  const void* ts, const int64_t* te, int64_t nt, int32_t lt, const int64_t* th, const int32_t* nodes, int64_t n_start, int64_t w0,
                  int64_t w1, int32_t len, int32_t trials, const uint64_t* sd, int32_t* out) {
    return matcha_hyper_walk(ptr, nb, cm, n_nodes, ps, pe, np, lp, ts, te, nt, lt, th, nodes, n_start, w0, w1, len, trials, sd, out, q, nullptr);
  };
  CHECK(refused(call(nullptr, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "null pointer"));
  CHECK(refused(call(e, nullptr, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "null pointer"));
  CHECK(refused(call(e, q, nullptr, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "null pointer"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, nullptr, q, 4, 0, 8, 80, 1024, &seed, q), "null pointer"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, nullptr, 4, 0, 8, 80, 1024, &seed, q), "null pointer"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, nullptr, q), "null pointer"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, nullptr), "null pointer"));
  CHECK(refused(call(e, q, cum, 0, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "n_nodes=0"));
  CHECK(refused(call(e, q, cum, INT32_MIN, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "n_nodes="));
  CHECK(refused(call(e, q, cum, 10, nullptr, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "non-empty pair set without buffers"));
  CHECK(refused(call(e, q, cum, 10, q, nullptr, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "non-empty pair set without buffers"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, nullptr, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "non-empty triple set without buffers"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, nullptr, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "non-empty triple set without buffers"));
  CHECK(refused(call(e, q, cum, 10, q, e, -1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "n_pair_edges=-1"));
  CHECK(refused(call(e, q, cum, 10, q, e, M + 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "n_pair_edges="));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, -1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "n_triple_edges=-1"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, INT64_MAX, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "n_triple_edges="));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 1, q, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "L_pair=1"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 33, q, e, 1, 3, thr, q, 4, 0, 8, 80, 1024, &seed, q), "L_pair=33"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 2, thr, q, 4, 0, 8, 80, 1024, &seed, q), "L_triple=2"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 33, thr, q, 4, 0, 8, 80, 1024, &seed, q), "L_triple=33"));
  int64_t bad[3] = {A / 8, -1, A};
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, bad, q, 4, 0, 8, 80, 1024, &seed, q), "thresholds[1]=-1"));
  bad[1] = A + 1;
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, bad, q, 4, 0, 8, 80, 1024, &seed, q), "thresholds[1]="));
  bad[1] = INT64_MIN; bad[0] = INT64_MAX;
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, bad, q, 4, 0, 8, 80, 1024, &seed, q), "thresholds[0]="));
  int64_t none[3] = {A - 1, A - 1, A - 1};
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, none, q, 4, 0, 8, 80, 1024, &seed, q), "no class accepts always"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 0, 0, 8, 80, 1024, &seed, q), "n_start=0"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, INT64_MIN, 0, 8, 80, 1024, &seed, q), "n_start="));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 0, 1024, &seed, q), "walk_length=0"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 16385, 1024, &seed, q), "walk_length=16385"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, INT32_MIN, 1024, &seed, q), "walk_length="));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, 0, &seed, q), "max_trials=0"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, 65537, &seed, q), "max_trials=65537"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, 8, 80, INT32_MAX, &seed, q), "max_trials="));
  // the walk's id is a 32-bit counter: the integer extremes of the range
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, -1, 8, 80, 1024, &seed, q), "walk ids"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, INT64_MIN, 8, 80, 1024, &seed, q), "walk ids"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, M + 1, 80, 1024, &seed, q), "walk ids"));
  CHECK(refused(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 0, INT64_MAX, 80, 1024, &seed, q), "walk ids"));
  // no-ops: an empty range (also a reversed one); empty sets need no buffers and no widths
  CHECK(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 8, 8, 80, 1024, &seed, q) == MATCHA_OK);
  CHECK(call(e, q, cum, 10, q, e, 1, 2, q, e, 1, 3, thr, q, 4, 9, 8, 80, 1024, &seed, q) == MATCHA_OK);
  CHECK(call(e, q, cum, 10, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, 0, thr, q, 4, M, M, 1, 1, &seed, q) == MATCHA_OK);
}

static void sgns_checks() {
  int32_t walks[8] = {0};
  float tab[8] = {0};
  uint64_t cum[8] = {0};
  uint64_t seed = 1;
  int32_t st[4] = {0};
  const int64_t A = (int64_t)1 << 32;
  // n_walks, walk_length, w0, w1, n_nodes, d, window, negative, lr0, lr1, g_base, g_total
  auto call = [&](const int32_t* w, int64_t n_walks, int32_t len, int64_t w0, int64_t w1, int32_t n_nodes, int32_t d, float* s0, float* s1,
                  const uint64_t* cm, int32_t window, int32_t negative, double lr0, double lr1, int64_t g_base, int64_t g_total, const uint64_t* sd) {
    return matcha_sgns_epoch(w, n_walks, len, w0, w1, n_nodes, d, s0, s1, cm, window, negative, lr0, lr1, g_base, g_total, sd, st, nullptr);
  };
  CHECK(refused(call(nullptr, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 32, &seed), "null pointer"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, nullptr, tab, cum, 5, 5, 0.025, 1e-4, 0, 32, &seed), "null pointer"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, nullptr, cum, 5, 5, 0.025, 1e-4, 0, 32, &seed), "null pointer"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, nullptr, 5, 5, 0.025, 1e-4, 0, 32, &seed), "null pointer"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 32, nullptr), "null pointer"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 32, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 32, &seed), "d=32"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 192, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 32, &seed), "d=192"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, INT32_MIN, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 32, &seed), "d="));
  CHECK(refused(call(walks, 8, 4, 0, 8, 0, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 32, &seed), "n_nodes=0"));
  CHECK(refused(call(walks, 8, 0, 0, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 32, &seed), "walk_length=0"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 0, 5, 0.025, 1e-4, 0, 32, &seed), "window=0"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 1025, 5, 0.025, 1e-4, 0, 32, &seed), "window=1025"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, -1, 0.025, 1e-4, 0, 32, &seed), "negative=-1"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 33, 0.025, 1e-4, 0, 32, &seed), "negative=33"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 5, 1e-4, 0.025, 0, 32, &seed), "learning rates"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, -1.0, 0, 32, &seed), "learning rates"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 5, (double)NAN, 1e-4, 0, 32, &seed), "learning rates"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 5, (double)INFINITY, 1e-4, 0, 32, &seed), "learning rates"));
  CHECK(refused(call(walks, 8, 4, -1, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 32, &seed), "walks ["));
  CHECK(refused(call(walks, 8, 4, 0, 9, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 32, &seed), "walks ["));
  CHECK(refused(call(walks, -1, 4, 0, 0, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 32, &seed), "walks ["));
  CHECK(refused(call(walks, 8, 4, INT64_MIN, INT64_MAX, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 32, &seed), "walks ["));
  // the global position is a 32-bit counter: g_base + n_walks * walk_length <= g_total <= 2^32, without overflow at the extremes
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 0, &seed), "g_total=0"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, A + 1, &seed), "g_total="));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, INT64_MAX, &seed), "g_total="));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, -1, 32, &seed), "g_base=-1"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 1, 32, &seed), "pass g_total=32"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 31, &seed), "pass g_total=31"));
  CHECK(refused(call(walks, 8, 4, 0, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, INT64_MAX, 32, &seed), "g_base="));
  CHECK(refused(call(walks, INT64_MAX, INT32_MAX, 0, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, A, &seed), "pass g_total="));
  CHECK(refused(call(walks, A, 2, 0, 8, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, A, &seed), "pass g_total="));
  // no-ops: an empty range, an empty corpus
  CHECK(call(walks, 8, 4, 3, 3, 10, 64, tab, tab, cum, 5, 5, 0.025, 1e-4, 0, 32, &seed) == MATCHA_OK);
  CHECK(call(walks, 8, 4, 5, 3, 10, 256, tab, tab, cum, 1, 0, 0.025, 0.025, 32, 64, &seed) == MATCHA_OK);
  CHECK(call(walks, 0, 4, 0, 0, 10, 128, tab, tab, cum, 1024, 32, 0.0, 0.0, 0, 1, &seed) == MATCHA_OK);
}

int main() {
  hyper_walk_checks();
  sgns_checks();
  return finish("WALK HOST CHECKS");
}
