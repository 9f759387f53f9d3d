// The cluster file's text -> CSR (csrc/cluster_text.hip) under AddressSanitizer + UndefinedBehaviorSanitizer on the host, next to
// tests/host/cluster_adj_checks.hip: the two workspace queries (what they refuse, how they grow, that every count the entry accepts has a
// size), the argument validation of the two entries and every refusal of the chromosome table.  No kernel runs: every call below is refused
// before any device call, on device pointers that are never dereferenced (the chromosome table is HOST memory and is read); without a device
// the first device call of a valid request comes back as MATCHA_EHIP.
#include "host_driver.hpp"

static const int kName = MATCHA_CLUSTER_TEXT_NAME_MAX;

struct Table {
  std::vector<char> names;
  std::vector<int32_t> first, bins;
  void add(const char* name, int32_t f, int32_t b) {
    const size_t at = names.size();
    names.resize(at + kName, 0);
    memcpy(names.data() + at, name, strlen(name) < (size_t)kName ? strlen(name) : (size_t)kName);
    first.push_back(f);
    bins.push_back(b);
  }
  int32_t n() const { return (int32_t)first.size(); }
};

static void workspace_checks() {
  CHECK(matcha_cluster_text_count_workspace_bytes(-1) == 0 && matcha_cluster_text_count_workspace_bytes((int64_t)1 << 31) == 0);
  CHECK(matcha_cluster_text_count_workspace_bytes(0) == 8192 && matcha_cluster_text_count_workspace_bytes(((int64_t)1 << 31) - 1) == 8192);
  // counts that no text of n bytes has
  CHECK(matcha_cluster_text_workspace_bytes(-1, 1, 0) == 0 && matcha_cluster_text_workspace_bytes((int64_t)1 << 31, 1, 0) == 0);
  CHECK(matcha_cluster_text_workspace_bytes(10, 0, 0) == 0 && matcha_cluster_text_workspace_bytes(10, 12, 0) == 0);
  CHECK(matcha_cluster_text_workspace_bytes(10, 1, -1) == 0 && matcha_cluster_text_workspace_bytes(10, 1, 11) == 0);
  CHECK(matcha_cluster_text_workspace_bytes(10, 6, 6) == 0);               // 5 terminators + 6 tabs in 10 bytes
  // the carving: every region is 256-byte aligned, so the size is a multiple of 256; it grows with each of the three counts; the table and
  // the flag word alone take sizeof(names) + three int32 arrays + 256
  const size_t empty = matcha_cluster_text_workspace_bytes(0, 1, 0);
  CHECK(empty > 0 && empty % 256 == 0 && empty >= (size_t)MATCHA_CLUSTER_TEXT_CHROM_MAX * (kName + 12) + 256);
  size_t prev = empty;
  for (int64_t n = 1; n <= ((int64_t)1 << 30); n *= 4) {
    const size_t a = matcha_cluster_text_workspace_bytes(n, 1, 0);
    const size_t b = matcha_cluster_text_workspace_bytes(n, n / 4 + 1, 0);
    const size_t c = matcha_cluster_text_workspace_bytes(n, n / 4 + 1, n / 2);
    CHECK(a % 256 == 0 && b % 256 == 0 && c % 256 == 0 && a >= prev && b >= a && c >= b);
    CHECK(a >= (size_t)(n / 16 + 1) * 8);                                  // the span counts
    // (an empty region still takes its 256 bytes: four regions hold per-tab arrays, five per-line arrays)
    CHECK(c - b + 4 * 256 >= (size_t)(n / 2) * (4 + 8 + 8 + 4));           // tab positions, two key arrays, the unique flags
    CHECK(b - a + 5 * 256 >= (size_t)(n / 4) * (4 + 4 + 4 + 8 + 4));       // terminator positions, lo, hi, the packed counts, the unique starts
    prev = a;
  }
  CHECK(matcha_cluster_text_workspace_bytes(((int64_t)1 << 31) - 1, (int64_t)1 << 30, (int64_t)1 << 30) > ((size_t)1 << 35));
}

static void entry_checks() {
  alignas(256) static char dev[1024];                 // stands for device memory: never dereferenced
  uint8_t* const text = (uint8_t*)dev;
  int32_t* const i32 = (int32_t*)(dev + 256);
  int64_t* const i64 = (int64_t*)(dev + 512);
  void* const ws = dev;
  // count: text, n, counts, ws, ws_bytes
  const size_t cneed = matcha_cluster_text_count_workspace_bytes(100);
  CHECK(refused(matcha_cluster_text_count(text, -1, i64, ws, cneed, nullptr), "n=-1"));
  CHECK(refused(matcha_cluster_text_count(text, (int64_t)1 << 31, i64, ws, cneed, nullptr), "n="));
  CHECK(refused(matcha_cluster_text_count(text, 100, nullptr, ws, cneed, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_text_count(text, 100, i64, nullptr, cneed, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_text_count(nullptr, 100, i64, ws, cneed, nullptr), "null text"));
  CHECK(refused(matcha_cluster_text_count(text + 8, 100, i64, ws, cneed, nullptr), "aligned"));
  CHECK(refused(matcha_cluster_text_count(text, 100, (int64_t*)(dev + 516), ws, cneed, nullptr), "aligned"));
  CHECK(refused(matcha_cluster_text_count(text, 100, i64, ws, cneed - 1, nullptr), "too small"));

  Table t;
  t.add("chr1", 1, 14);
  t.add("chr10", 15, 9);
  t.add("chr1_random", 24, 7);
  const int32_t N = 30;
  const int64_t n = 100, nl = 5, nt = 12;
  const size_t need = matcha_cluster_text_workspace_bytes(n, nl, nt);
  CHECK(need > 0);
  auto parse = [&](const Table& tb, int64_t n_, int64_t nl_, int64_t nt_, int64_t res, int64_t max_size, int32_t nodes, size_t bytes) {
    return matcha_cluster_text_parse(text, n_, nl_, nt_, tb.names.data(), tb.first.data(), tb.bins.data(), tb.n(), res, max_size, nodes, i32, nt_, i64,
                                     nl_ + 1, i64 + 32, i64 + 33, i32 + 32, ws, bytes, nullptr);
  };
  CHECK(refused(parse(t, -1, nl, nt, 1000, 6, N, need), "n=-1"));
  CHECK(refused(parse(t, (int64_t)1 << 31, nl, nt, 1000, 6, N, need), "n="));
  CHECK(refused(parse(t, n, 0, nt, 1000, 6, N, need), "cannot be the counts"));
  CHECK(refused(parse(t, n, n + 2, 0, 1000, 6, N, need), "cannot be the counts"));
  CHECK(refused(parse(t, n, nl, -1, 1000, 6, N, need), "cannot be the counts"));
  CHECK(refused(parse(t, n, 60, 60, 1000, 6, N, need), "cannot be the counts"));
  CHECK(refused(parse(t, n, nl, nt, 0, 6, N, need), "res=0"));
  CHECK(refused(parse(t, n, nl, nt, (int64_t)1 << 31, 6, N, need), "res="));
  CHECK(refused(parse(t, n, nl, nt, 1000, 0, N, need), "max_cluster_size=0"));
  CHECK(refused(parse(t, n, nl, nt, 1000, ((int64_t)1 << 24) + 1, N, need), "max_cluster_size="));
  CHECK(refused(parse(t, n, nl, nt, 1000, 6, 0, need), "n_nodes=0"));
  CHECK(refused(parse(t, n, nl, nt, 1000, 6, N, need - 1), "too small"));
  CHECK(refused(parse(t, n, nl, nt, 1000, 6, N, 0), "too small"));
  // pointers and capacities
  const char* nm = t.names.data();
  const int32_t *fp = t.first.data(), *bp = t.bins.data();
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nullptr, fp, bp, 3, 1000, 6, N, i32, nt, i64, nl + 1, i64 + 32, i64 + 33, i32 + 32, ws, need, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, nullptr, bp, 3, 1000, 6, N, i32, nt, i64, nl + 1, i64 + 32, i64 + 33, i32 + 32, ws, need, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, nullptr, 3, 1000, 6, N, i32, nt, i64, nl + 1, i64 + 32, i64 + 33, i32 + 32, ws, need, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, bp, 0, 1000, 6, N, i32, nt, i64, nl + 1, i64 + 32, i64 + 33, i32 + 32, ws, need, nullptr), "n_chrom=0"));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, bp, 257, 1000, 6, N, i32, nt, i64, nl + 1, i64 + 32, i64 + 33, i32 + 32, ws, need, nullptr), "n_chrom=257"));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, bp, 3, 1000, 6, N, nullptr, nt, i64, nl + 1, i64 + 32, i64 + 33, i32 + 32, ws, need, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, bp, 3, 1000, 6, N, i32, nt, nullptr, nl + 1, i64 + 32, i64 + 33, i32 + 32, ws, need, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, bp, 3, 1000, 6, N, i32, nt, i64, nl + 1, nullptr, i64 + 33, i32 + 32, ws, need, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, bp, 3, 1000, 6, N, i32, nt, i64, nl + 1, i64 + 32, nullptr, i32 + 32, ws, need, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, bp, 3, 1000, 6, N, i32, nt, i64, nl + 1, i64 + 32, i64 + 33, nullptr, ws, need, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, bp, 3, 1000, 6, N, i32, nt, i64, nl + 1, i64 + 32, i64 + 33, i32 + 32, nullptr, need, nullptr), "null pointer"));
  CHECK(refused(matcha_cluster_text_parse(nullptr, n, nl, nt, nm, fp, bp, 3, 1000, 6, N, i32, nt, i64, nl + 1, i64 + 32, i64 + 33, i32 + 32, ws, need, nullptr), "null text"));
  CHECK(refused(matcha_cluster_text_parse(text + 4, n, nl, nt, nm, fp, bp, 3, 1000, 6, N, i32, nt, i64, nl + 1, i64 + 32, i64 + 33, i32 + 32, ws, need, nullptr), "aligned"));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, bp, 3, 1000, 6, N, i32, nt, i64, nl + 1, i64 + 32, i64 + 33, i32 + 32, dev + 64, need, nullptr), "aligned"));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, bp, 3, 1000, 6, N, i32, nt, (int64_t*)(dev + 516), nl + 1, i64 + 32, i64 + 33, i32 + 32, ws, need, nullptr), "aligned"));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, bp, 3, 1000, 6, N, i32, nt - 1, i64, nl + 1, i64 + 32, i64 + 33, i32 + 32, ws, need, nullptr), "ids_cap="));
  CHECK(refused(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, bp, 3, 1000, 6, N, i32, nt, i64, nl, i64 + 32, i64 + 33, i32 + 32, ws, need, nullptr), "offsets_cap="));
  // the table
  auto bad_table = [&](const Table& tb, int64_t res, const char* word) { return refused(parse(tb, n, nl, nt, res, 6, N, need), word); };
  { Table b = t; b.add("chr10", 1, 2); CHECK(bad_table(b, 1000, "duplicate name")); }
  { Table b = t; b.add("", 1, 2); CHECK(bad_table(b, 1000, "empty name")); }
  { Table b = t; b.add("chr 2", 1, 2); CHECK(bad_table(b, 1000, "chromosome 3: name")); }
  { Table b = t; b.add("chr\t2", 1, 2); CHECK(bad_table(b, 1000, "chromosome 3: name")); }
  { Table b = t; b.add("chr:2", 1, 2); CHECK(bad_table(b, 1000, "chromosome 3: name")); }
  { Table b = t; b.add("chr\xc3\xa9", 1, 2); CHECK(bad_table(b, 1000, "chromosome 3: name")); }
  { Table b = t; b.add("chr\x1c", 1, 2); CHECK(bad_table(b, 1000, "chromosome 3: name")); }
  { Table b = t; b.add("chr2", 1, 2); b.names[3 * kName + 10] = 'x'; CHECK(bad_table(b, 1000, "zero-padded")); }      // bytes behind the first NUL
  { Table b = t; b.add("chr2", 0, 2); CHECK(bad_table(b, 1000, "node range")); }
  { Table b = t; b.add("chr2", 1, 0); CHECK(bad_table(b, 1000, "node range")); }
  { Table b = t; b.add("chr2", 30, 2); CHECK(bad_table(b, 1000, "node range")); }
  { Table b = t; b.add("chr2", INT32_MAX, INT32_MAX); CHECK(bad_table(b, 1000, "node range")); }
  {                                                                          // 2^23 bins of 2^31 - 1: past 2^53, where float64 stops holding positions
    Table b;
    b.add("chr1", 1, 1 << 23);
    CHECK(refused(parse(b, n, nl, nt, ((int64_t)1 << 31) - 1, 6, 1 << 24, need), "2^53"));
    CHECK(refused(parse(b, n, nl, nt, (int64_t)1 << 30, 6, 1 << 24, need - 1), "too small"));      // 2^53 itself is accepted
  }
  {                                                                          // a name of exactly 32 bytes, no NUL behind it, is a name
    Table b = t;
    b.add("abcdefghijklmnopqrstuvwxyz012345", 25, 2);
    const int rc = parse(b, n, nl, nt, 1000, 6, N, need - 1);
    CHECK(refused(rc, "too small"));                                         // the table passed: the next refusal is the workspace's
  }
  // valid calls up to the first device call: without a device it fails and is REPORTED
  if (matcha_device_count() == 0) {
    CHECK(matcha_cluster_text_count(text, 100, i64, ws, cneed, nullptr) == MATCHA_EHIP);
    CHECK(strstr(matcha_last_error(), "cluster_text_count_kernel") != nullptr);
    std::vector<char> big(need + 512);
    char* aligned = (char*)(((uintptr_t)big.data() + 255) / 256 * 256);
    CHECK(matcha_cluster_text_parse(text, n, nl, nt, nm, fp, bp, 3, 1000, 6, N, i32, nt, i64, nl + 1, i64 + 32, i64 + 33, i32 + 32, aligned, need, nullptr) ==
          MATCHA_EHIP);
  }
}

int main() {
  workspace_checks();
  entry_checks();
  return finish("CLUSTER PARSE HOST CHECKS");
}
