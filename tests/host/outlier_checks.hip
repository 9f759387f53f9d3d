// The host side of outlier identification (matcha_locus_scores in csrc/forward_long.hip, matcha_outlier_plant in csrc/sampler.hip, DESIGN.md
// 7.15) under AddressSanitizer + UndefinedBehaviorSanitizer on the host, next to tests/host/complete_checks.hip: the same host-only objects,
// model.hip included as source for the library's error and option plumbing, a driver of its own.  No kernel runs: every call below is
// refused, or is a no-op, before any device call, on pointers that are never dereferenced.
#include "host_driver.hpp"

static void locus_scores_checks() {
  matcha_shape s;
  s.d = 16; s.n_attr = 24; s.n_nodes = 3067; s.n_chrom = 0; s.mode = 0; s.max_bins = 0;
  static float dummy[4];
  matcha_tensors p;
  float** slots = reinterpret_cast<float**>(&p);
  for (size_t i = 0; i < sizeof(p) / sizeof(float*); ++i) slots[i] = dummy;
  matcha_frozen f;
  memset(&f, 0, sizeof(f));
  f.attr_table = dummy;
  matcha_step_opts o;
  memset(&o, 0, sizeof(o));
  o.forward_only = 1;
  const int64_t B = 5;
  const int32_t L = 9;
  const size_t need = matcha_workspace_bytes_long(&s, B, L);
  CHECK(need > 0 && need % 256 == 0);
  char* ws = (char*)aligned_alloc(256, need);
  int64_t x[1] = {0}, order[1] = {0};
  float scores[1] = {0}, logits[1] = {0};

  // the shape and the bounds of matcha_forward_long, under this entry's name
  CHECK(refused(matcha_locus_scores(nullptr, &p, &f, &o, x, B, L, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "matcha_locus_scores: null shape"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, B, 1, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "L=1 outside 2..32"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, B, 33, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "L=33 outside 2..32"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, B, INT32_MAX, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "outside 2..32"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, B, INT32_MIN, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "outside 2..32"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, 0, L, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "must be >= 1"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, -1, L, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "must be >= 1"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, (int64_t)1 << 31, 2, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "2^31 - 2"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, 65535ll * 128 / 2, 2, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "token rows"));
  matcha_shape bad = s;
  bad.d = 20;
  CHECK(refused(matcha_locus_scores(&bad, &p, &f, &o, x, B, L, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "embed_dim d=20"));
  // its own arguments
  CHECK(refused(matcha_locus_scores(&s, nullptr, &f, &o, x, B, L, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "null pointer"));
  CHECK(refused(matcha_locus_scores(&s, &p, nullptr, &o, x, B, L, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "null pointer"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, nullptr, x, B, L, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "null pointer"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, nullptr, B, L, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "null pointer"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, B, L, nullptr, logits, 0, nullptr, nullptr, ws, need, nullptr), "null pointer"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, B, L, scores, logits, 0, nullptr, nullptr, nullptr, need, nullptr), "null pointer"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, B, L, scores, logits, -1, order, nullptr, ws, need, nullptr), "lowest=-1 outside 0..32"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, B, L, scores, logits, 33, order, nullptr, ws, need, nullptr), "lowest=33 outside 0..32"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, B, L, scores, logits, INT32_MAX, order, nullptr, ws, need, nullptr), "outside 0..32"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, B, L, scores, logits, INT32_MIN, order, nullptr, ws, need, nullptr), "outside 0..32"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, B, L, scores, logits, 3, nullptr, nullptr, ws, need, nullptr), "order must be null when lowest == 0 and only then"));
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, B, L, scores, logits, 0, order, nullptr, ws, need, nullptr), "order must be null when lowest == 0 and only then"));
  // inference only
  matcha_step_opts t = o;
  t.training = 1;
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &t, x, B, L, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "inference-only"));
  t = o;
  t.forward_only = 0;
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &t, x, B, L, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "inference-only"));
  t = o;
  int32_t cell = 0;
  t.random_chrom_dev = &cell;
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &t, x, B, L, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "random_chrom_dev"));
  // what both long forwards ask behind that
  CHECK(refused(matcha_locus_scores(&s, &p, &f, &o, x, B, L, scores, logits, 0, nullptr, nullptr, ws + 64, need, nullptr), "256-byte aligned"));
  matcha_tensors q = p;
  q.cls_w = nullptr;
  CHECK(refused(matcha_locus_scores(&s, &q, &f, &o, x, B, L, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "a parameter pointer is null"));
  q = p;
  q.table = nullptr;
  CHECK(refused(matcha_locus_scores(&s, &q, &f, &o, x, B, L, scores, logits, 0, nullptr, nullptr, ws, need, nullptr), "table mode without table"));
  // the workspace is matcha_workspace_bytes_long's: one byte less is refused as too small
  CHECK(matcha_locus_scores(&s, &p, &f, &o, x, B, L, scores, logits, 0, nullptr, nullptr, ws, need - 1, nullptr) == MATCHA_ENOMEM);
  CHECK(strstr(matcha_last_error(), "matcha_locus_scores: workspace") != nullptr);
  CHECK(matcha_locus_scores(&s, &p, &f, &o, x, B, L, scores, logits, 3, order, nullptr, ws, 0, nullptr) == MATCHA_ENOMEM);
  free(ws);
}

static void outlier_plant_checks() {
  int64_t host[8] = {0};
  int32_t hint[8] = {0};
  uint64_t seed = 1;
  int64_t* const e = host;            // edges / pos / out
  int32_t* const q = hint;            // tables, node2chrom, chrom_range (8-byte aligned below), planted, status
  alignas(8) int32_t range[2] = {1, 2};
  const int64_t M = ((int64_t)1 << 31) - 1;
  // set, set_edges, n_set, L_set, pair_set, pair_edges, n_pair, L_pair, pos, P, L, draws, cycle, min_dis, node2chrom, n_nodes, chrom_range, n_chrom, seed, n0, out, planted, status
  auto call = [&](const void* set, const int64_t* se, int64_t ns, int32_t ls, const void* ps, const int64_t* pe, int64_t np, int32_t lp, const int64_t* pos,
                  int64_t P, int32_t L, int32_t draws, const int32_t* n2c, int32_t n_nodes, const int32_t* cr, int32_t n_chrom, const uint64_t* sd, int64_t n0,
                  int64_t* out, int32_t* planted) {
    return matcha_outlier_plant(set, se, ns, ls, ps, pe, np, lp, pos, P, L, draws, 0, 0, n2c, n_nodes, cr, n_chrom, sd, n0, out, planted, q, nullptr);
  };
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, nullptr, 4, 3, 1, q, 10, range, 1, &seed, 0, e, q), "null pointer"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 3, 1, q, 10, range, 1, &seed, 0, nullptr, q), "null pointer"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 3, 1, q, 10, range, 1, &seed, 0, e, nullptr), "null pointer"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 3, 1, nullptr, 10, range, 1, &seed, 0, e, q), "null pointer"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 3, 1, q, 10, nullptr, 1, &seed, 0, e, q), "null pointer"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 3, 1, q, 10, range, 1, nullptr, 0, e, q), "null pointer"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 3, 1, q, 10, range + 1, 1, &seed, 0, e, q), "8-byte aligned"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 3, 1, q, 0, range, 1, &seed, 0, e, q), "n_nodes=0"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 3, 1, q, 10, range, 0, &seed, 0, e, q), "n_chrom=0"));
  CHECK(refused(call(nullptr, e, 1, 3, q, e, 1, 2, e, 4, 3, 1, q, 10, range, 1, &seed, 0, e, q), "non-empty set without buffers"));
  CHECK(refused(call(q, nullptr, 1, 3, q, e, 1, 2, e, 4, 3, 1, q, 10, range, 1, &seed, 0, e, q), "non-empty set without buffers"));
  CHECK(refused(call(q, e, 1, 3, nullptr, e, 1, 2, e, 4, 3, 1, q, 10, range, 1, &seed, 0, e, q), "non-empty pair set without buffers"));
  CHECK(refused(call(q, e, 1, 3, q, nullptr, 1, 2, e, 4, 3, 1, q, 10, range, 1, &seed, 0, e, q), "non-empty pair set without buffers"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 0, 1, q, 10, range, 1, &seed, 0, e, q), "L=0"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 33, 1, q, 10, range, 1, &seed, 0, e, q), "L=33"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, INT32_MAX, 1, q, 10, range, 1, &seed, 0, e, q), "L="));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 3, 0, q, 10, range, 1, &seed, 0, e, q), "draws=0"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 3, INT32_MIN, q, 10, range, 1, &seed, 0, e, q), "draws="));
  CHECK(refused(call(q, e, 1, 0, q, e, 1, 2, e, 4, 3, 1, q, 10, range, 1, &seed, 0, e, q), "L_set=0"));
  CHECK(refused(call(q, e, 1, 33, q, e, 1, 2, e, 4, 3, 1, q, 10, range, 1, &seed, 0, e, q), "L_set=33"));
  CHECK(refused(call(q, e, -1, 3, q, e, 1, 2, e, 4, 3, 1, q, 10, range, 1, &seed, 0, e, q), "n_set_edges=-1"));
  CHECK(refused(call(q, e, M + 1, 3, q, e, 1, 2, e, 4, 3, 1, q, 10, range, 1, &seed, 0, e, q), "n_set_edges="));
  CHECK(refused(call(q, e, 1, 3, q, e, -1, 2, e, 4, 3, 1, q, 10, range, 1, &seed, 0, e, q), "n_pair_edges=-1"));
  CHECK(refused(call(q, e, 1, 3, q, e, INT64_MAX, 2, e, 4, 3, 1, q, 10, range, 1, &seed, 0, e, q), "n_pair_edges="));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 1, e, 4, 3, 1, q, 10, range, 1, &seed, 0, e, q), "L_pair=1"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 33, e, 4, 3, 1, q, 10, range, 1, &seed, 0, e, q), "L_pair=33"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 3, 1, q, 10, range, 1, &seed, -1, e, q), "n0=-1 must not be negative"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 3, 1, q, 10, range, 1, &seed, INT64_MIN, e, q), "must not be negative"));
  // the integer extremes of n0 + P*draws: the row's global index is a 32-bit counter
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, M + 1, 3, 1, q, 10, range, 1, &seed, 0, e, q), "rows"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, INT64_MAX, 3, 1, q, 10, range, 1, &seed, 0, e, q), "rows"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, INT64_MAX, 3, INT32_MAX, q, 10, range, 1, &seed, 0, e, q), "rows"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 2, 3, INT32_MAX, q, 10, range, 1, &seed, 0, e, q), "rows"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, M / 3 + 1, 3, 3, q, 10, range, 1, &seed, 0, e, q), "rows"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, M, 3, 1, q, 10, range, 1, &seed, 1, e, q), "reach 2^31"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 1, 3, 1, q, 10, range, 1, &seed, M, e, q), "reach 2^31"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 1, 3, 1, q, 10, range, 1, &seed, INT64_MAX, e, q), "reach 2^31"));
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 4, 3, 3, q, 10, range, 1, &seed, M - 1 - 9, e, q), "reach 2^31"));     // 12 rows from 2^31 - 11 on
  CHECK(refused(call(q, e, 1, 3, q, e, 1, 2, e, 1, 3, INT32_MAX, q, 10, range, 1, &seed, INT32_MAX, e, q), "reach 2^31"));
  // no-ops: accepted, nothing launched (no positives; empty sets need no buffers and no pair width)
  CHECK(call(q, e, 1, 3, q, e, 1, 2, e, 0, 3, 1, q, 10, range, 1, &seed, 0, e, q) == MATCHA_OK);
  CHECK(call(nullptr, nullptr, 0, 3, nullptr, nullptr, 0, 0, e, 0, 32, 7, q, 10, range, 1, &seed, 14, e, q) == MATCHA_OK);
  CHECK(call(q, e, 1, 3, q, e, 1, 2, e, -5, 3, 1, q, 10, range, 1, &seed, M, e, q) == MATCHA_OK);
}

int main() {
  locus_scores_checks();
  outlier_plant_checks();
  return finish("OUTLIER HOST CHECKS");
}
