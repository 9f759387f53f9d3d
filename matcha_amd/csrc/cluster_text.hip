// The cluster file's text -> clusters in CSR form, on the device: the reference's parse_file (Code/process.py:42-87) for one
// chunk of whole lines.  ids int32 / offsets int64 are what csrc/kmers.hip and csrc/cluster_adj.hip take.
//
// The contract (process.py line numbers; pinned by tests/golden/g9_process.npz and cluster_text_edge.npz):
//   lines     every '\r' and every '\n' ends a line (the empty line inside "\r\n" has no items); a last line without a terminator counts
//   strip     leading / trailing bytes of {0x09-0x0d, 0x1c-0x1f, 0x20} are removed (:52), the rest is split on '\t', the first field is dropped
//   pre-filter  a line with fewer than 2 or more than 50 max_cluster_size items is skipped UNPARSED (:54): nothing on it raises anything
//   items     exactly one ':' or MATCHA_CLUSTER_TEXT_ESPLIT (:60-63, the host's EOFError); a name that is not in the table drops the item
//             before its position is looked at (:64); node = first_node + floor(position / res), the quotient formed in float64 as :66
//             does; a bin past the chromosome's last is MATCHA_CLUSTER_TEXT_EBIN (:68, the host's KeyError)
//   cluster   node ids de-duplicated and sorted (:70, :77), kept when 2 <= nodes <= max_cluster_size (:73, :82), in file order
// Narrower than Python's int(): a position is 1 .. 18 ASCII digits, anything else MATCHA_CLUSTER_TEXT_EGRAMMAR; 19 or more digits are
// MATCHA_CLUSTER_TEXT_EBIN; a byte >= 0x80 anywhere in the text is MATCHA_CLUSTER_TEXT_ENONASCII.
//
//   cluster_text_count_kernel      per aligned 16-byte span: terminators and tabs, summed per block; cluster_text_count_sum_kernel adds the blocks
//   cluster_text_span_kernel       the same counts per span, packed (terminators << 32 | tabs) for ONE exclusive scan; flags bytes >= 0x80
//   cluster_text_verify_kernel     the scan's totals against the caller's counts: every later kernel leaves at once when they differ
//   cluster_text_scatter_kernel    the sorted byte positions of the terminators and of the tabs
//   cluster_text_lines_kernel      one lane per line: the stripped range [lo, hi), its tabs by two binary searches, the pre-filter
//   cluster_text_items_kernel      one lane per TAB: its line by a binary search in the terminators, the single colon, the name against the
//                                  table in LDS, the digits, the key line << nb | node (all ones: dropped)
//   (rocprim::radix_sort_keys over the used bits)
//   cluster_text_flag_kernel       1 at every first occurrence of a valid key; an exclusive scan numbers the unique (line, node) pairs
//   cluster_text_linecount_kernel  one lane per live line: its key range by two binary searches, its unique count, the size filter
//   (one exclusive scan of (kept << 32 | nodes) per line: the cluster index and the id offset of every kept line)
//   cluster_text_emit_kernel       ids; cluster_text_offsets_kernel: offsets, n_clusters, n_ids
// The only atomics are integer ones on the status words.  No kernel indexes memory with a value it has not bounded.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "kernels.hpp"

namespace matcha {
namespace {

constexpr int kBlock = 256;
constexpr int kSpan = 16;                               // bytes per lane in the scan kernels
constexpr int kNameMax = MATCHA_CLUSTER_TEXT_NAME_MAX;  // 32
constexpr int kChromMax = MATCHA_CLUSTER_TEXT_CHROM_MAX;  // 256
constexpr int kNameWords = kNameMax / 8;
constexpr int kCountBlocks = 1024;
constexpr int kMaxDigits = 18;
constexpr unsigned long long kDropped = ~0ull;

__device__ __forceinline__ unsigned long long shfl64_xor(unsigned long long v, int mask) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask, kWave), hi = (uint32_t)__shfl_xor((int)(v >> 32), mask, kWave);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ bool is_term(uint32_t b) { return b == 0x0au || b == 0x0du; }
__device__ __forceinline__ bool is_strip(uint32_t b) { return (b >= 0x09u && b <= 0x0du) || (b >= 0x1cu && b <= 0x20u); }

// the 16 bytes of span i as four words; bytes at or past n read as 0 (never loaded)
__device__ __forceinline__ uint4 load_span(const uint8_t* __restrict__ text, int64_t n, int64_t i) {
  const int64_t base = i * kSpan;
  if (base + kSpan <= n) return *reinterpret_cast<const uint4*>(text + base);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < kSpan; ++j)
    if (base + j < n) w[j >> 2] |= (uint32_t)text[base + j] << (8 * (j & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void count_word(uint32_t w, uint32_t& terms, uint32_t& tabs, uint32_t& high) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t b = (w >> (8 * j)) & 0xffu;
    terms += is_term(b) ? 1u : 0u;
    tabs += b == 0x09u ? 1u : 0u;
  }
  high |= w & 0x80808080u;
}

__global__ __launch_bounds__(kBlock) void cluster_text_count_kernel(const uint8_t* __restrict__ text, int64_t n, int64_t n_spans,
                                                                    unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long red[kBlock / kWave];
  uint32_t terms = 0, tabs = 0, high = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_spans; i += (int64_t)gridDim.x * kBlock) {
    const uint4 v = load_span(text, n, i);
    count_word(v.x, terms, tabs, high);
    count_word(v.y, terms, tabs, high);
    count_word(v.z, terms, tabs, high);
    count_word(v.w, terms, tabs, high);
  }
  unsigned long long pack = ((unsigned long long)terms << 32) | tabs;      // both sums stay below 2^31: n < 2^31
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) pack += shfl64_xor(pack, o);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = pack;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int w = 0; w < kBlock / kWave; ++w) s += red[w];
    partial[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kWave) void cluster_text_count_sum_kernel(const unsigned long long* __restrict__ partial, int blocks,
                                                                       int64_t* __restrict__ counts) {
  unsigned long long s = 0;
  for (int i = threadIdx.x; i < blocks; i += kWave) s += partial[i];
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) s += shfl64_xor(s, o);
  if (threadIdx.x == 0) {
    counts[0] = (int64_t)(s >> 32) + 1;                                    // lines: one more than terminators (the last may be empty)
    counts[1] = (int64_t)(s & 0xffffffffull);                              // tabs
  }
}

// status {0, max, max, max, max, 0, 0, 0}, the outputs' counts 0, ok = 0
__global__ void cluster_text_init_kernel(int32_t* __restrict__ status, int64_t* __restrict__ n_clusters, int64_t* __restrict__ n_ids,
                                         int64_t* __restrict__ offsets, int32_t* __restrict__ ok) {
  const int t = threadIdx.x;
  if (t < 8) status[t] = (t >= 1 && t <= 4) ? INT32_MAX : 0;
  if (t == 8) *n_clusters = 0;
  if (t == 9) *n_ids = 0;
  if (t == 10) offsets[0] = 0;
  if (t == 11) *ok = 0;
}

__global__ __launch_bounds__(kBlock) void cluster_text_span_kernel(const uint8_t* __restrict__ text, int64_t n, int64_t n_spans,
                                                                   unsigned long long* __restrict__ span_pack, int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i > n_spans) return;
  if (i == n_spans) {                                                      // the scan's last input: its output there is the totals
    span_pack[i] = 0;
    return;
  }
  const uint4 v = load_span(text, n, i);
  uint32_t terms = 0, tabs = 0, high = 0;
  count_word(v.x, terms, tabs, high);
  count_word(v.y, terms, tabs, high);
  count_word(v.z, terms, tabs, high);
  count_word(v.w, terms, tabs, high);
  span_pack[i] = ((unsigned long long)terms << 32) | tabs;
  if (high) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    int first = kSpan;
#pragma unroll
    for (int j = kSpan - 1; j >= 0; --j)
      if ((w[j >> 2] >> (8 * (j & 3))) & 0x80u) first = j;
    atomicOr(status, MATCHA_CLUSTER_TEXT_ENONASCII);
    atomicMin(status + 4, (int32_t)(i * kSpan + first));
  }
}

__global__ void cluster_text_verify_kernel(const unsigned long long* __restrict__ span_pack, int64_t n_spans, int64_t n_terms, int64_t n_tabs,
                                           int32_t* __restrict__ ok, int32_t* __restrict__ status) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned long long tot = span_pack[n_spans];
  const bool same = (int64_t)(tot >> 32) == n_terms && (int64_t)(tot & 0xffffffffull) == n_tabs;
  *ok = same ? 1 : 0;
  if (!same) atomicOr(status, MATCHA_CLUSTER_TEXT_ECOUNT);
}

__global__ __launch_bounds__(kBlock) void cluster_text_scatter_kernel(const uint8_t* __restrict__ text, int64_t n, int64_t n_spans,
                                                                      const unsigned long long* __restrict__ span_pack, const int32_t* __restrict__ ok,
                                                                      int64_t n_terms, int64_t n_tabs, int32_t* __restrict__ term_pos,
                                                                      int32_t* __restrict__ tab_pos) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_spans || !*ok) return;
  const uint4 v = load_span(text, n, i);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  const unsigned long long off = span_pack[i];
  int64_t t = (int64_t)(off >> 32), b = (int64_t)(off & 0xffffffffull);
#pragma unroll
  for (int j = 0; j < kSpan; ++j) {
    const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
    const int32_t pos = (int32_t)(i * kSpan + j);
    if (is_term(c)) {
      if (t < n_terms) term_pos[t] = pos;                                  // ok says the totals agree: the guards only restate it
      ++t;
    } else if (c == 0x09u) {
      if (b < n_tabs) tab_pos[b] = pos;
      ++b;
    }
  }
}

// the number of entries of the ascending a[0 .. count) that are < v
__device__ __forceinline__ int64_t count_below(const int32_t* __restrict__ a, int64_t count, int64_t v) {
  int64_t lo = 0, hi = count;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int64_t count_below_u64(const unsigned long long* __restrict__ a, int64_t count, unsigned long long v) {
  int64_t lo = 0, hi = count;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// line k is [k ? term_pos[k - 1] + 1 : 0, k < n_terms ? term_pos[k] : n); line_hi = -1 marks a line the pre-filter skips
__global__ __launch_bounds__(kBlock) void cluster_text_lines_kernel(const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ ok,
                                                                    const int32_t* __restrict__ term_pos, int64_t n_terms,
                                                                    const int32_t* __restrict__ tab_pos, int64_t n_tabs, int64_t max_items,
                                                                    int32_t* __restrict__ line_lo, int32_t* __restrict__ line_hi) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k > n_terms || !*ok) return;
  int64_t lo = k ? (int64_t)term_pos[k - 1] + 1 : 0;
  int64_t hi = k < n_terms ? (int64_t)term_pos[k] : n;
  lo = lo < 0 ? 0 : lo;
  hi = hi > n ? n : hi;
  while (lo < hi && is_strip(text[lo])) ++lo;
  while (hi > lo && is_strip(text[hi - 1])) --hi;
  int64_t items = 0;
  if (lo < hi) items = count_below(tab_pos, n_tabs, hi) - count_below(tab_pos, n_tabs, lo);
  const bool live = items >= 2 && items <= max_items;
  line_lo[k] = (int32_t)lo;
  line_hi[k] = live ? (int32_t)hi : -1;
}

struct ChromTable {                        // in the workspace, copied from the host by the entry; staged in LDS by the items kernel
  unsigned long long name[kChromMax][kNameWords];      // zero-padded, little-endian words
  int32_t len[kChromMax];
  int32_t first[kChromMax];
  int32_t bins[kChromMax];
};

__global__ __launch_bounds__(kBlock) void cluster_text_items_kernel(const uint8_t* __restrict__ text, int64_t n, const int32_t* __restrict__ ok,
                                                                    const int32_t* __restrict__ term_pos, int64_t n_terms,
                                                                    const int32_t* __restrict__ tab_pos, int64_t n_tabs,
                                                                    const int32_t* __restrict__ line_lo, const int32_t* __restrict__ line_hi,
                                                                    const ChromTable* __restrict__ table, int32_t n_chrom, double res, int nb,
                                                                    unsigned long long* __restrict__ keys, int32_t* __restrict__ status) {
  __shared__ unsigned long long s_name[kChromMax][kNameWords];
  __shared__ int32_t s_len[kChromMax], s_first[kChromMax], s_bins[kChromMax];
  for (int c = threadIdx.x; c < n_chrom; c += kBlock) {
#pragma unroll
    for (int w = 0; w < kNameWords; ++w) s_name[c][w] = table->name[c][w];
    s_len[c] = table->len[c];
    s_first[c] = table->first[c];
    s_bins[c] = table->bins[c];
  }
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= n_tabs || !*ok) return;
  unsigned long long key = kDropped;
  int err = 0;
  const int64_t p = tab_pos[t];
  int64_t b = 0;
  if (p >= 0 && p < n) {
    const int64_t k = count_below(term_pos, n_terms, p);                    // terminators in front of the tab: its line
    const int64_t hi = line_hi[k], lo = line_lo[k];
    if (hi >= 0 && hi <= n && p >= lo && p < hi) {                          // a live line, and a tab the strip left in
      b = p + 1;
      int64_t e = hi;
      if (t + 1 < n_tabs) {
        const int64_t nx = tab_pos[t + 1];
        if (nx > p && nx < hi) e = nx;
      }
      int colons = 0;
      int64_t colon = e;
      for (int64_t i = b; i < e; ++i)
        if (text[i] == (uint8_t)':') {
          if (colons == 0) colon = i;
          ++colons;
        }
      if (colons != 1) {
        err = MATCHA_CLUSTER_TEXT_ESPLIT;
      } else {
        const int64_t len = colon - b;
        int chrom = -1;
        if (len >= 1 && len <= kNameMax) {
          unsigned long long w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (j < len) w0 |= (unsigned long long)text[b + j] << (8 * j);
            if (j + 8 < len) w1 |= (unsigned long long)text[b + 8 + j] << (8 * j);
            if (j + 16 < len) w2 |= (unsigned long long)text[b + 16 + j] << (8 * j);
            if (j + 24 < len) w3 |= (unsigned long long)text[b + 24 + j] << (8 * j);
          }
          for (int c = 0; c < n_chrom; ++c) {
            if (s_name[c][0] == w0 && s_len[c] == (int32_t)len && s_name[c][1] == w1 && s_name[c][2] == w2 && s_name[c][3] == w3) chrom = c;
          }
        }
        if (chrom >= 0) {                                                   // an unlisted name drops the item before its position is read
          const int64_t d0 = colon + 1, nd = e - d0;
          bool digits = nd >= 1;
          unsigned long long v = 0;
          for (int64_t i = d0; i < e; ++i) {
            const uint32_t c = text[i];
            if (c < (uint32_t)'0' || c > (uint32_t)'9') {
              digits = false;
              break;
            }
            if (i - d0 < kMaxDigits) v = v * 10ull + (c - (uint32_t)'0');
          }
          if (!digits) {
            err = MATCHA_CLUSTER_TEXT_EGRAMMAR;
          } else if (nd > kMaxDigits || v >= (1ull << 53)) {
            err = MATCHA_CLUSTER_TEXT_EBIN;                                 // the table keeps bins * res <= 2^53: such a position lies past every chromosome
          } else {
            const double q = floor((double)v / res);                        // process.py:66 divides in float64; v < 2^53 and res < 2^31 are exact
            if (q >= (double)s_bins[chrom]) {
              err = MATCHA_CLUSTER_TEXT_EBIN;
            } else {
              key = ((unsigned long long)k << nb) | (unsigned long long)(uint32_t)(s_first[chrom] + (int32_t)q);
            }
          }
        }
      }
    }
  }
  keys[t] = key;
  if (err) {
    atomicOr(status, err);
    atomicMin(status + (err == MATCHA_CLUSTER_TEXT_ESPLIT ? 1 : err == MATCHA_CLUSTER_TEXT_EBIN ? 2 : 3), (int32_t)b);
  }
}

// flags [n_tabs + 1]: 1 where a valid key differs from the one in front of it; the entry behind the last key is 0 (the scan's total lands there)
__global__ __launch_bounds__(kBlock) void cluster_text_flag_kernel(const unsigned long long* __restrict__ sorted, int64_t n_tabs,
                                                                   const int32_t* __restrict__ ok, uint32_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i > n_tabs) return;
  uint32_t f = 0;
  if (i < n_tabs && *ok) {
    const unsigned long long key = sorted[i];
    f = key != kDropped && (i == 0 || sorted[i - 1] != key) ? 1u : 0u;
  }
  flags[i] = f;
}

// line_pack [n_lines + 1]: (1 << 32 | nodes) for a kept line, 0 for any other and for the entry behind the last line; line_ustart: the number
// of unique pairs in front of the line's own
__global__ __launch_bounds__(kBlock) void cluster_text_linecount_kernel(const unsigned long long* __restrict__ sorted, int64_t n_tabs,
                                                                        const uint32_t* __restrict__ upos, const int32_t* __restrict__ ok,
                                                                        const int32_t* __restrict__ line_hi, int64_t n_lines, int nb,
                                                                        int64_t max_nodes, unsigned long long* __restrict__ line_pack,
                                                                        uint32_t* __restrict__ line_ustart) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k > n_lines) return;
  unsigned long long pack = 0;
  uint32_t ustart = 0;
  if (k < n_lines && *ok && line_hi[k] >= 0) {
    const int64_t r0 = count_below_u64(sorted, n_tabs, (unsigned long long)k << nb);
    const int64_t r1 = count_below_u64(sorted, n_tabs, (unsigned long long)(k + 1) << nb);
    ustart = upos[r0];
    const int64_t nodes = (int64_t)upos[r1] - (int64_t)ustart;            // upos has n_tabs + 1 entries
    if (nodes >= 2 && nodes <= max_nodes) pack = (1ull << 32) | (unsigned long long)nodes;
  }
  line_pack[k] = pack;
  if (k < n_lines) line_ustart[k] = ustart;
}

// after the exclusive scan line_pack[k] = (kept lines in front << 32 | ids in front); a line is kept when the next entry counts one more
__global__ __launch_bounds__(kBlock) void cluster_text_emit_kernel(const unsigned long long* __restrict__ sorted, int64_t n_tabs,
                                                                   const uint32_t* __restrict__ flags_scanned, const int32_t* __restrict__ ok,
                                                                   const unsigned long long* __restrict__ line_pack,
                                                                   const uint32_t* __restrict__ line_ustart, int64_t n_lines, int nb,
                                                                   int32_t* __restrict__ ids, int64_t ids_cap) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_tabs || !*ok) return;
  const unsigned long long key = sorted[i];
  if (key == kDropped || (i > 0 && sorted[i - 1] == key)) return;
  const int64_t k = (int64_t)(key >> nb);
  if (k >= n_lines) return;
  const unsigned long long here = line_pack[k], next = line_pack[k + 1];
  if ((next >> 32) == (here >> 32)) return;                                // the line was not kept
  const int64_t pos = (int64_t)(here & 0xffffffffull) + ((int64_t)flags_scanned[i] - (int64_t)line_ustart[k]);
  if (pos >= 0 && pos < ids_cap) ids[pos] = (int32_t)(key & ((1ull << nb) - 1ull));
}

__global__ __launch_bounds__(kBlock) void cluster_text_offsets_kernel(const unsigned long long* __restrict__ line_pack, int64_t n_lines,
                                                                      const int32_t* __restrict__ ok, int64_t* __restrict__ offsets,
                                                                      int64_t offsets_cap, int64_t* __restrict__ n_clusters,
                                                                      int64_t* __restrict__ n_ids) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k > n_lines || !*ok) return;
  const unsigned long long here = line_pack[k];
  const int64_t c = (int64_t)(here >> 32), o = (int64_t)(here & 0xffffffffull);
  if (k == n_lines) {                                                      // the totals
    if (c < offsets_cap) offsets[c] = o;
    *n_clusters = c;
    *n_ids = o;
    return;
  }
  if ((line_pack[k + 1] >> 32) != (here >> 32) && c < offsets_cap) offsets[c] = o;
}

inline int bit_width(int64_t v) {                                          // the smallest b with 2^b > v
  int b = 1;
  while (((int64_t)1 << b) <= v) ++b;
  return b;
}

struct Plan {
  size_t off_table, off_ok, off_span, off_term, off_tab, off_lo, off_hi, off_keys_a, off_keys_b, off_flags, off_pack, off_ustart, off_tmp, tmp_bytes,
      total_bytes;
};

void make_plan(int64_t n, int64_t n_lines, int64_t n_tabs, Plan& pl) {
  const int64_t n_spans = cdiv(n, kSpan);
  // rocPRIM's scratch.  Its own queries pick a configuration from the current device and fail where there is none, and the size has to be the
  // same on the machine that sizes and on the one that runs: reserve a bound no configuration exceeds -- the sort's second key buffer plus
  // its histograms, the scans' one look-back state per block of at least 64 items -- and let the entry hold every query to it.
  size_t longest = (size_t)n_spans + 1;
  if ((size_t)n_lines + 1 > longest) longest = (size_t)n_lines + 1;
  if ((size_t)n_tabs + 1 > longest) longest = (size_t)n_tabs + 1;
  size_t tmp = (size_t)n_tabs * 2 * sizeof(unsigned long long);
  if (longest > tmp) tmp = longest;
  tmp += (size_t)2 << 20;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes ? bytes : 1, 256); return o; };
  pl.off_table = take(sizeof(ChromTable));
  pl.off_ok = take(sizeof(int32_t));
  pl.off_span = take(((size_t)n_spans + 1) * sizeof(unsigned long long));
  pl.off_term = take((size_t)n_lines * sizeof(int32_t));                   // n_lines - 1 terminators
  pl.off_tab = take((size_t)n_tabs * sizeof(int32_t));
  pl.off_lo = take((size_t)n_lines * sizeof(int32_t));
  pl.off_hi = take((size_t)n_lines * sizeof(int32_t));
  pl.off_keys_a = take((size_t)n_tabs * sizeof(unsigned long long));
  pl.off_keys_b = take((size_t)n_tabs * sizeof(unsigned long long));
  pl.off_flags = take(((size_t)n_tabs + 1) * sizeof(uint32_t));
  pl.off_pack = take(((size_t)n_lines + 1) * sizeof(unsigned long long));
  pl.off_ustart = take((size_t)n_lines * sizeof(uint32_t));
  pl.off_tmp = take(tmp);
  pl.tmp_bytes = tmp;
  pl.total_bytes = off;
}

bool sizes_ok(int64_t n, int64_t n_lines, int64_t n_tabs) {
  return n >= 0 && n < ((int64_t)1 << 31) && n_lines >= 1 && n_lines <= n + 1 && n_tabs >= 0 && n_tabs <= n && n_lines - 1 + n_tabs <= n;
}

bool name_byte_ok(unsigned char c) { return c > 0x20 && c < 0x80 && c != ':'; }      // no control byte, blank, colon or non-ASCII byte

unsigned grid_of(int64_t count) { return (unsigned)cdiv(count > 0 ? count : 1, kBlock); }

}  // namespace
}  // namespace matcha

using namespace matcha;

extern "C" size_t matcha_cluster_text_count_workspace_bytes(int64_t n) {
  if (n < 0 || n >= ((int64_t)1 << 31)) return 0;
  return align_up((size_t)kCountBlocks * sizeof(unsigned long long), 256);
}

extern "C" int matcha_cluster_text_count(const uint8_t* text, int64_t n, int64_t* counts, void* ws, size_t ws_bytes, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "matcha_cluster_text_count: n=%lld must be in [0, 2^31)", (long long)n);
  MATCHA_CHECK_ARG(counts && ws, "matcha_cluster_text_count: null pointer (counts or ws)");
  MATCHA_CHECK_ARG(n == 0 || text, "matcha_cluster_text_count: null text");
  MATCHA_CHECK_ARG(((uintptr_t)text) % 16 == 0 && ((uintptr_t)ws) % 8 == 0 && ((uintptr_t)counts) % 8 == 0,
                   "matcha_cluster_text_count: text must be 16-byte aligned, ws and counts 8-byte aligned");
  const size_t need = matcha_cluster_text_count_workspace_bytes(n);
  MATCHA_CHECK_ARG(ws_bytes >= need, "matcha_cluster_text_count: workspace too small (%zu bytes, matcha_cluster_text_count_workspace_bytes says %zu)",
                   ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_spans = cdiv(n, kSpan);
  int64_t blocks = cdiv(n_spans, kBlock);
  blocks = blocks < 1 ? 1 : blocks > kCountBlocks ? kCountBlocks : blocks;
  unsigned long long* partial = (unsigned long long*)ws;
  hipLaunchKernelGGL(cluster_text_count_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, text, n, n_spans, partial);
  MATCHA_CHECK_LAUNCH("cluster_text_count_kernel");
  hipLaunchKernelGGL(cluster_text_count_sum_kernel, dim3(1), dim3(kWave), 0, st, partial, (int)blocks, counts);
  MATCHA_CHECK_LAUNCH("cluster_text_count_sum_kernel");
  return MATCHA_OK;
}

extern "C" size_t matcha_cluster_text_workspace_bytes(int64_t n, int64_t n_lines, int64_t n_tabs) {
  if (!sizes_ok(n, n_lines, n_tabs)) return 0;
  Plan pl;
  make_plan(n, n_lines, n_tabs, pl);
  return pl.total_bytes;
}

extern "C" int matcha_cluster_text_parse(const uint8_t* text, int64_t n, int64_t n_lines, int64_t n_tabs, const char* names, const int32_t* first_node,
                                         const int32_t* n_bins, int32_t n_chrom, int64_t res, int64_t max_cluster_size, int32_t n_nodes, int32_t* ids,
                                         int64_t ids_cap, int64_t* offsets, int64_t offsets_cap, int64_t* n_clusters, int64_t* n_ids, int32_t* status,
                                         void* ws, size_t ws_bytes, matcha_stream_t stream) {
  const char* const me = "matcha_cluster_text_parse";
  MATCHA_CHECK_ARG(n >= 0 && n < ((int64_t)1 << 31), "%s: n=%lld must be in [0, 2^31)", me, (long long)n);
  MATCHA_CHECK_ARG(sizes_ok(n, n_lines, n_tabs), "%s: n_lines=%lld, n_tabs=%lld cannot be the counts of %lld bytes", me, (long long)n_lines,
                   (long long)n_tabs, (long long)n);
  MATCHA_CHECK_ARG(n_chrom >= 1 && n_chrom <= kChromMax, "%s: n_chrom=%d outside 1..%d", me, n_chrom, kChromMax);
  MATCHA_CHECK_ARG(res >= 1 && res < ((int64_t)1 << 31), "%s: res=%lld must be in [1, 2^31)", me, (long long)res);
  MATCHA_CHECK_ARG(max_cluster_size >= 1 && max_cluster_size <= ((int64_t)1 << 24), "%s: max_cluster_size=%lld must be in [1, 2^24]", me,
                   (long long)max_cluster_size);
  MATCHA_CHECK_ARG(n_nodes >= 1, "%s: n_nodes=%d must be >= 1", me, n_nodes);
  MATCHA_CHECK_ARG(names && first_node && n_bins, "%s: null pointer (names, first_node or n_bins)", me);
  MATCHA_CHECK_ARG(ids && offsets && n_clusters && n_ids && status && ws, "%s: null pointer (ids, offsets, n_clusters, n_ids, status or ws)", me);
  MATCHA_CHECK_ARG(n == 0 || text, "%s: null text", me);
  MATCHA_CHECK_ARG(((uintptr_t)text) % 16 == 0, "%s: text must be 16-byte aligned", me);
  MATCHA_CHECK_ARG(((uintptr_t)ws) % 256 == 0 && ((uintptr_t)offsets) % 8 == 0 && ((uintptr_t)n_clusters) % 8 == 0 && ((uintptr_t)n_ids) % 8 == 0 &&
                       ((uintptr_t)ids) % 4 == 0 && ((uintptr_t)status) % 4 == 0,
                   "%s: ws must be 256-byte aligned, offsets / n_clusters / n_ids 8-byte, ids and status 4-byte aligned", me);
  MATCHA_CHECK_ARG(ids_cap >= n_tabs && offsets_cap >= n_lines + 1, "%s: ids_cap=%lld must be >= n_tabs=%lld and offsets_cap=%lld >= n_lines + 1=%lld", me,
                   (long long)ids_cap, (long long)n_tabs, (long long)offsets_cap, (long long)(n_lines + 1));
  // the table: names of 1 .. 32 bytes without blanks, control bytes, colons or non-ASCII bytes, zero-padded, no two alike; node ranges inside
  // 1 .. n_nodes; bins * res <= 2^53, so that a position of 2^53 or more lies past every chromosome
  ChromTable* tab = new ChromTable;
  memset(tab, 0, sizeof(ChromTable));
  int bad = -1;
  const char* why = "";
  for (int c = 0; c < n_chrom && bad < 0; ++c) {
    const unsigned char* nm = (const unsigned char*)names + (size_t)c * kNameMax;
    int len = 0;
    while (len < kNameMax && nm[len]) ++len;
    for (int j = 0; j < kNameMax; ++j)
      if (j < len ? !name_byte_ok(nm[j]) : nm[j] != 0) { bad = c; why = "name must be 1..32 bytes above 0x20 and below 0x80 without ':', zero-padded"; }
    if (len == 0) { bad = c; why = "empty name"; }
    if (bad >= 0) break;
    memcpy(tab->name[c], nm, kNameMax);
    tab->len[c] = len;
    tab->first[c] = first_node[c];
    tab->bins[c] = n_bins[c];
    if (first_node[c] < 1 || n_bins[c] < 1 || (int64_t)first_node[c] + n_bins[c] - 1 > n_nodes) { bad = c; why = "node range leaves 1 .. n_nodes"; }
    else if ((int64_t)n_bins[c] > ((int64_t)1 << 53) / res) { bad = c; why = "n_bins * res exceeds 2^53"; }
    for (int o = 0; o < c && bad < 0; ++o)
      if (!memcmp(tab->name[o], tab->name[c], kNameMax)) { bad = c; why = "duplicate name"; }
  }
  if (bad >= 0) {
    delete tab;
    set_error("%s: chromosome %d: %s", me, bad, why);
    return MATCHA_EINVAL;
  }
  Plan pl;
  make_plan(n, n_lines, n_tabs, pl);
  if (ws_bytes < pl.total_bytes) {
    delete tab;
    set_error("%s: workspace too small (%zu bytes, matcha_cluster_text_workspace_bytes says %zu)", me, ws_bytes, pl.total_bytes);
    return MATCHA_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)ws;
  int32_t* ok = (int32_t*)(base + pl.off_ok);
  const hipError_t ce = hipMemcpyAsync(base + pl.off_table, tab, sizeof(ChromTable), hipMemcpyHostToDevice, st);      // pageable: staged before it returns
  delete tab;
  if (ce != hipSuccess) {
    set_error("%s: copying the chromosome table failed: %s", me, hipGetErrorString(ce));
    return MATCHA_EHIP;
  }
  hipLaunchKernelGGL(cluster_text_init_kernel, dim3(1), dim3(kWave), 0, st, status, n_clusters, n_ids, offsets, ok);
  MATCHA_CHECK_LAUNCH("cluster_text_init_kernel");
  if (n == 0) return MATCHA_OK;                                            // the empty CSR: offsets = [0]
  const int64_t n_spans = cdiv(n, kSpan), n_terms = n_lines - 1;
  unsigned long long* span_pack = (unsigned long long*)(base + pl.off_span);
  int32_t* term_pos = (int32_t*)(base + pl.off_term);
  int32_t* tab_pos = (int32_t*)(base + pl.off_tab);
  int32_t* line_lo = (int32_t*)(base + pl.off_lo);
  int32_t* line_hi = (int32_t*)(base + pl.off_hi);
  unsigned long long* keys_a = (unsigned long long*)(base + pl.off_keys_a);
  unsigned long long* keys_b = (unsigned long long*)(base + pl.off_keys_b);
  uint32_t* flags = (uint32_t*)(base + pl.off_flags);
  unsigned long long* line_pack = (unsigned long long*)(base + pl.off_pack);
  uint32_t* line_ustart = (uint32_t*)(base + pl.off_ustart);
  void* tmp = base + pl.off_tmp;
  size_t tb = pl.tmp_bytes;
  hipLaunchKernelGGL(cluster_text_span_kernel, dim3(grid_of(n_spans + 1)), dim3(kBlock), 0, st, text, n, n_spans, span_pack, status);
  MATCHA_CHECK_LAUNCH("cluster_text_span_kernel");
  tb = 0;
  if (rocprim::exclusive_scan(nullptr, tb, span_pack, span_pack, 0ull, (size_t)n_spans + 1, rocprim::plus<unsigned long long>(), st) != hipSuccess || tb > pl.tmp_bytes) {
    set_error("%s: the scan of the span counts asks for %zu bytes of scratch, %zu are reserved", me, tb, pl.tmp_bytes);
    return MATCHA_EHIP;
  }
  tb = pl.tmp_bytes;
  if (rocprim::exclusive_scan(tmp, tb, span_pack, span_pack, 0ull, (size_t)n_spans + 1, rocprim::plus<unsigned long long>(), st) != hipSuccess) {
    set_error("%s: the scan of the span counts failed", me);
    return MATCHA_EHIP;
  }
  hipLaunchKernelGGL(cluster_text_verify_kernel, dim3(1), dim3(kWave), 0, st, span_pack, n_spans, n_terms, n_tabs, ok, status);
  MATCHA_CHECK_LAUNCH("cluster_text_verify_kernel");
  if (n_tabs == 0) return MATCHA_OK;                                       // no items anywhere: the empty CSR the init kernel wrote
  hipLaunchKernelGGL(cluster_text_scatter_kernel, dim3(grid_of(n_spans)), dim3(kBlock), 0, st, text, n, n_spans, span_pack, ok, n_terms, n_tabs, term_pos,
                     tab_pos);
  MATCHA_CHECK_LAUNCH("cluster_text_scatter_kernel");
  hipLaunchKernelGGL(cluster_text_lines_kernel, dim3(grid_of(n_lines)), dim3(kBlock), 0, st, text, n, ok, term_pos, n_terms, tab_pos, n_tabs,
                     50 * max_cluster_size, line_lo, line_hi);
  MATCHA_CHECK_LAUNCH("cluster_text_lines_kernel");
  const int nb = bit_width(n_nodes), lb = bit_width(n_lines);
  hipLaunchKernelGGL(cluster_text_items_kernel, dim3(grid_of(n_tabs)), dim3(kBlock), 0, st, text, n, ok, term_pos, n_terms, tab_pos, n_tabs, line_lo, line_hi,
                     (const ChromTable*)(base + pl.off_table), n_chrom, (double)res, nb, keys_a, status);
  MATCHA_CHECK_LAUNCH("cluster_text_items_kernel");
  const int end_bit = nb + lb + 1 < 64 ? nb + lb + 1 : 64;                 // + 1: the dropped key's bit above every valid key
  tb = 0;
  if (rocprim::radix_sort_keys(nullptr, tb, keys_a, keys_b, (size_t)n_tabs, 0, end_bit, st) != hipSuccess || tb > pl.tmp_bytes) {
    set_error("%s: the radix sort asks for %zu bytes of scratch, %zu are reserved", me, tb, pl.tmp_bytes);
    return MATCHA_EHIP;
  }
  tb = pl.tmp_bytes;
  if (rocprim::radix_sort_keys(tmp, tb, keys_a, keys_b, (size_t)n_tabs, 0, end_bit, st) != hipSuccess) {
    set_error("%s: the radix sort failed", me);
    return MATCHA_EHIP;
  }
  hipLaunchKernelGGL(cluster_text_flag_kernel, dim3(grid_of(n_tabs + 1)), dim3(kBlock), 0, st, keys_b, n_tabs, ok, flags);
  MATCHA_CHECK_LAUNCH("cluster_text_flag_kernel");
  tb = 0;
  if (rocprim::exclusive_scan(nullptr, tb, flags, flags, 0u, (size_t)n_tabs + 1, rocprim::plus<uint32_t>(), st) != hipSuccess || tb > pl.tmp_bytes) {
    set_error("%s: the scan of the unique flags asks for %zu bytes of scratch, %zu are reserved", me, tb, pl.tmp_bytes);
    return MATCHA_EHIP;
  }
  tb = pl.tmp_bytes;
  if (rocprim::exclusive_scan(tmp, tb, flags, flags, 0u, (size_t)n_tabs + 1, rocprim::plus<uint32_t>(), st) != hipSuccess) {
    set_error("%s: the scan of the unique flags failed", me);
    return MATCHA_EHIP;
  }
  hipLaunchKernelGGL(cluster_text_linecount_kernel, dim3(grid_of(n_lines + 1)), dim3(kBlock), 0, st, keys_b, n_tabs, flags, ok, line_hi, n_lines, nb,
                     max_cluster_size, line_pack, line_ustart);
  MATCHA_CHECK_LAUNCH("cluster_text_linecount_kernel");
  tb = 0;
  if (rocprim::exclusive_scan(nullptr, tb, line_pack, line_pack, 0ull, (size_t)n_lines + 1, rocprim::plus<unsigned long long>(), st) != hipSuccess || tb > pl.tmp_bytes) {
    set_error("%s: the scan of the kept lines asks for %zu bytes of scratch, %zu are reserved", me, tb, pl.tmp_bytes);
    return MATCHA_EHIP;
  }
  tb = pl.tmp_bytes;
  if (rocprim::exclusive_scan(tmp, tb, line_pack, line_pack, 0ull, (size_t)n_lines + 1, rocprim::plus<unsigned long long>(), st) != hipSuccess) {
    set_error("%s: the scan of the kept lines failed", me);
    return MATCHA_EHIP;
  }
  hipLaunchKernelGGL(cluster_text_emit_kernel, dim3(grid_of(n_tabs)), dim3(kBlock), 0, st, keys_b, n_tabs, flags, ok, line_pack, line_ustart, n_lines, nb, ids,
                     ids_cap);
  MATCHA_CHECK_LAUNCH("cluster_text_emit_kernel");
  hipLaunchKernelGGL(cluster_text_offsets_kernel, dim3(grid_of(n_lines + 1)), dim3(kBlock), 0, st, line_pack, n_lines, ok, offsets, offsets_cap, n_clusters,
                     n_ids);
  MATCHA_CHECK_LAUNCH("cluster_text_offsets_kernel");
  return MATCHA_OK;
}
