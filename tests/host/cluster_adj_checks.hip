// Contact matrices from the clusters (csrc/cluster_adj.hip) under AddressSanitizer + UndefinedBehaviorSanitizer on the host, next
// to tests/host/walk_checks.hip: the pair unrank of csrc/cluster_unrank.hpp -- the very function the kernel calls -- at every row boundary of the
// triangle, the host-only pair count, and the argument validation of the four entries.  No kernel runs: every call below is refused, or is a
// no-op, before any device call, on pointers that are never dereferenced (the pair count reads its HOST offsets); without a device the launch
// attempts come back as MATCHA_EHIP.
#include "host_driver.hpp"

#include "../../matcha_amd/csrc/cluster_unrank.hpp"

// every rank on either side of every row boundary: the first rank of row i is (i, i + 1), the rank before it (i - 1, s - 1); the rank after it
// (i, i + 2) where the row has one; and the last rank of the cluster
static int64_t unrank_mismatches(int32_t s) {
  const int64_t p = (int64_t)s * (s - 1) / 2;
  int64_t wrong = 0;
  auto at = [&](int64_t r, int64_t i, int64_t j) {
    int32_t gi = -1, gj = -1;
    tri_unrank(r, s, gi, gj);
    if (gi != i || gj != j) {
      if (++wrong <= 5) fprintf(stderr, "  tri_unrank(%lld, %d) = (%d, %d), wanted (%lld, %lld)\n", (long long)r, s, gi, gj, (long long)i, (long long)j);
    }
  };
  int64_t r = 0;                                     // the first rank of row i, counted up row by row: independent of tri_row_start
  for (int64_t i = 0; i + 1 < s; ++i) {
    at(r, i, i + 1);
    if (i > 0) at(r - 1, i - 1, s - 1);
    if (i + 2 < s) at(r + 1, i, i + 2);
    r += s - 1 - i;
  }
  if (r != p) ++wrong;
  at(p - 1, s - 2, s - 1);
  return wrong;
}

static void unrank_checks() {
  const int32_t sizes[] = {2, 3, 64, 65, 1000, 65535};
  for (int32_t s : sizes) CHECK(unrank_mismatches(s) == 0);
  // a small triangle in full
  int64_t r = 0, wrong = 0;
  for (int32_t i = 0; i < 37; ++i)
    for (int32_t j = i + 1; j < 37; ++j, ++r) {
      int32_t gi, gj;
      tri_unrank(r, 37, gi, gj);
      wrong += gi != i || gj != j;
    }
  CHECK(wrong == 0 && r == 37 * 36 / 2);
  CHECK(kMaxClusterNodes == 65535 && (int64_t)kMaxClusterNodes * (kMaxClusterNodes - 1) / 2 < ((int64_t)1 << 31));
}

static void pair_count_checks() {
  const int64_t off[] = {0, 2, 5, 5, 6, 70, 1070};            // sizes 2, 3, 0, 1, 64, 1000
  CHECK(matcha_cluster_pairs_count(off, 0) == 0);
  CHECK(matcha_cluster_pairs_count(off, 1) == 1);
  CHECK(matcha_cluster_pairs_count(off, 4) == 1 + 3);
  CHECK(matcha_cluster_pairs_count(off, 6) == 1 + 3 + 2016 + 499500);
  const int64_t big[] = {0, 65535, 131071};                    // 65535 nodes, then 65536
  CHECK(matcha_cluster_pairs_count(big, 1) == (int64_t)65535 * 65534 / 2);
  CHECK(matcha_cluster_pairs_count(big, 2) == -1);
  const int64_t back[] = {0, 5, 3};
  CHECK(matcha_cluster_pairs_count(back, 2) == -1);
  CHECK(matcha_cluster_pairs_count(nullptr, 1) == -1 && matcha_cluster_pairs_count(off, -1) == -1);
  // many large clusters: the sum passes 2^47 and stays exact (leaving int63 takes 2^32 clusters of 65535 nodes: no offsets array here holds them)
  std::vector<int64_t> many((size_t)1 << 16);
  for (size_t i = 0; i < many.size(); ++i) many[i] = (int64_t)i * 65535;
  const int64_t per = (int64_t)65535 * 65534 / 2;
  CHECK(matcha_cluster_pairs_count(many.data(), (int64_t)many.size() - 1) == per * ((int64_t)many.size() - 1));
}

static void entry_checks() {
  int64_t host[8] = {0, 2, 0, 0, 0, 0, 0, 0};
  int32_t hint[8] = {1, 2, 0, 0, 0, 0, 0, 0};
  double mat[16] = {0};
  int64_t* const e = host;
  int32_t* const q = hint;
  // update: ids, offsets, q, pair_ptr, M, n_nodes, acc, status
  CHECK(refused(matcha_cluster_adj_update(q, e, e, e, -1, 4, e, q, nullptr), "M=-1"));
  CHECK(refused(matcha_cluster_adj_update(q, e, e, e, INT64_MAX, 4, e, q, nullptr), "M="));
  CHECK(refused(matcha_cluster_adj_update(q, e, e, e, 1, 0, e, q, nullptr), "n_nodes=0"));
  CHECK(refused(matcha_cluster_adj_update(q, e, e, e, 1, INT32_MIN, e, q, nullptr), "n_nodes="));
  CHECK(refused(matcha_cluster_adj_update(q, e, e, e, 1, 4, nullptr, q, nullptr), "null acc"));
  CHECK(refused(matcha_cluster_adj_update(q, e, e, e, 1, 4, (int64_t*)((char*)e + 4), q, nullptr), "aligned"));
  CHECK(refused(matcha_cluster_adj_update(nullptr, e, e, e, 1, 4, e, q, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_adj_update(q, nullptr, e, e, 1, 4, e, q, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_adj_update(q, e, nullptr, e, 1, 4, e, q, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_adj_update(q, e, e, nullptr, 1, 4, e, q, nullptr), "null pointer"));
  CHECK(matcha_cluster_adj_update(nullptr, nullptr, nullptr, nullptr, 0, 4, e, nullptr, nullptr) == MATCHA_OK);      // no clusters: a no-op
  // finish: acc, node2chrom, n_nodes, intra, inter
  CHECK(refused(matcha_cluster_adj_finish(e, q, 0, mat, mat + 8, nullptr), "n_nodes=0"));
  CHECK(refused(matcha_cluster_adj_finish(nullptr, q, 2, mat, mat + 8, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_adj_finish(e, q, 2, nullptr, mat + 8, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_adj_finish(e, nullptr, 2, mat, mat + 8, nullptr), "needs node2chrom"));
  CHECK(refused(matcha_cluster_adj_finish(e, q, 2, mat, mat, nullptr), "alias"));
  // normalise: A, n_nodes, ranges, n_ranges, ws, ws_bytes
  CHECK(matcha_block_colmax_workspace_bytes(0, 3) == 0 && matcha_block_colmax_workspace_bytes(70, 0) == 0 && matcha_block_colmax_workspace_bytes(-1, -1) == 0);
  CHECK(matcha_block_colmax_workspace_bytes(70, 3) == 1792 && matcha_block_colmax_workspace_bytes(32, 1) == 256);
  const size_t need = matcha_block_colmax_workspace_bytes(2, 1);
  CHECK(refused(matcha_block_colmax_normalise(mat, 0, e, 1, mat + 8, need, nullptr), "n_nodes=0"));
  CHECK(refused(matcha_block_colmax_normalise(mat, 2, e, -1, mat + 8, need, nullptr), "n_ranges=-1"));
  CHECK(refused(matcha_block_colmax_normalise(mat, 2, e, INT32_MAX, mat + 8, need, nullptr), "n_ranges="));
  CHECK(refused(matcha_block_colmax_normalise(nullptr, 2, e, 1, mat + 8, need, nullptr), "null pointer"));
  CHECK(refused(matcha_block_colmax_normalise(mat, 2, nullptr, 1, mat + 8, need, nullptr), "null pointer"));
  CHECK(refused(matcha_block_colmax_normalise(mat, 2, e, 1, nullptr, need, nullptr), "null pointer"));
  CHECK(refused(matcha_block_colmax_normalise(mat, 2, e, 1, (char*)(mat + 8) + 4, need, nullptr), "aligned"));
  CHECK(refused(matcha_block_colmax_normalise(mat, 2, e, 1, mat + 8, need - 1, nullptr), "too small"));
  CHECK(matcha_block_colmax_normalise(mat, 2, nullptr, 0, nullptr, 0, nullptr) == MATCHA_OK);                           // no blocks: a no-op
  // valid calls up to the launch: without a device it fails and is REPORTED
  if (matcha_device_count() == 0) {
    int64_t off[2] = {0, 2}, ptr[2] = {0, 1}, w[1] = {(int64_t)1 << 32}, acc[4] = {0, 0, 0, 0}, rng[2] = {0, 2};
    int32_t ids[2] = {1, 2}, n2c[3] = {-1, 0, 0}, st[4] = {0, 0, 0, 0};
    double ws[32];
    CHECK(matcha_cluster_adj_update(ids, off, w, ptr, 1, 2, acc, st, nullptr) == MATCHA_EHIP);
    CHECK(strstr(matcha_last_error(), "cluster_pairs_update_kernel") != nullptr);
    CHECK(matcha_cluster_adj_finish(acc, n2c, 2, mat, mat + 8, nullptr) == MATCHA_EHIP);
    CHECK(matcha_cluster_adj_finish(acc, nullptr, 2, mat, nullptr, nullptr) == MATCHA_EHIP);
    CHECK(matcha_block_colmax_normalise(mat, 2, rng, 1, ws, sizeof(ws), nullptr) == MATCHA_EHIP);
    CHECK(strstr(matcha_last_error(), "block_colmax_normalise_kernel") != nullptr);
    CHECK(acc[1] == 0 && st[0] == 0);
  }
}

int main() {
  unrank_checks();
  pair_count_checks();
  entry_checks();
  return finish("CLUSTER ADJACENCY HOST CHECKS");
}
