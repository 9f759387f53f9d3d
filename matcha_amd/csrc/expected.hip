// Distance-matched expectation of k-way sweeps: statistics of a candidate's value per STRATUM of its gaps, accumulated on the
// device, and the observed-over-expected score of a candidate against the table made from them.
//
// A candidate of size k is a strictly ascending k-tuple of positive node ids x_0 < ... < x_{k-1}, zero-padded to the row width L (k <= L <= 8).
// Its gaps g_j = x_{j+1} - x_j fall into classes: class(g) = the number of edges <= g, for a strictly ascending list of 0 .. 15 positive edges,
// G = n_edges + 1 classes.  The stratum is the mixed radix of the classes, s = ((c_0 G + c_1) G + ...) + c_{k-2} < G^(k-1) <= 2^20; gap tuples stay
// ordered (mirror images are not merged).  A row whose leading non-zero run is not exactly k ids, is not strictly ascending, starts with a
// negative id or holds a non-zero id behind a zero has stratum -1.
//
//   gap_stats_init_kernel    zeroes the header (the two counters) and every plane (no memset).
//   gap_stats_update_kernel  one thread per row, L a template parameter (2 .. 8), the edges in the kernel arguments (padded to 15 with INT64_MAX, so
//                            the class is 15 compares with constant indices: nothing is indexed at run time, nothing goes to scratch).  An accepted
//                            row (skip == 0, stratum >= 0, 0 <= v <= vmax; -0.0 counts as 0) adds 1 to COUNT, rint(double(v) 2^shift) to SUM and
//                            rint(double(v) double(v) 2^shift) to SUMSQ of its stratum: int64 fixed point, integer adds commute, so the planes do
//                            not depend on arrival order or on how the stream is cut.  Sweep rows arrive in lexicographic order and the last gap
//                            changes class O(log n) times per prefix, so adjacent lanes mostly share a stratum: pairmap.hip's device -- compare
//                            with the lane below, one ballot for the run heads, one inclusive wavefront prefix of (q, q2, count), the LAST lane
//                            of a run issues the run's adds.  Rows in any order give the same planes, just more adds.  Where the planes fit the
//                            LDS budget (kLdsBudget: two workgroups per CU stay resident) the adds go to a block-level copy in LDS (64-bit LDS
//                            integer adds) and only its non-zero entries are flushed with global integer atomics after the block's grid-stride
//                            loop; above the budget (or with MATCHA_GAP_DIRECT in the mask) the run's adds are global atomics.  Integer atomics
//                            only.  The counters take one atomicAdd per wavefront.
//   gap_stats_read_kernel    the raw int64 planes and the two counters out.
//   gap_enrich_kernel        per row: the stratum (optionally written), and out = (score - offset[s]) * scale[s] as two separately rounded float32
//                            operations (no FMA contraction), NaN for stratum -1.  With null score only the strata are written.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "kernels.hpp"

namespace matcha {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxEdges = 15;
constexpr int64_t kMaxStrata = (int64_t)1 << 20;
constexpr int32_t kNoStratum = -1;
constexpr size_t kHeaderBytes = 256;           // int64 n_rows, int64 n_rejected, padding
constexpr size_t kLdsBudget = 64 * 1024;       // per workgroup: two of them fit a CU's 160 KiB
constexpr int kPlaneMask = MATCHA_GAP_COUNT | MATCHA_GAP_SUM | MATCHA_GAP_SUMSQ;

struct GapEdges {
  int64_t e[kMaxEdges];                        // the edges, then INT64_MAX (a gap of positive ids is at most INT64_MAX - 1)
  int32_t G, k;
};

struct GapPlan {
  size_t off_count, off_sum, off_sumsq, total; // an absent plane has offset 0
  int64_t n_strata;
  int n_planes;
};

// G^(k-1), or -1 beyond kMaxStrata / for arguments out of range
int64_t strata_count(int32_t k, int32_t n_edges) {
  if (k < 2 || k > MATCHA_MAX_L || n_edges < 0 || n_edges > kMaxEdges) return -1;
  int64_t s = 1;
  for (int j = 0; j < k - 1; ++j) {
    s *= n_edges + 1;
    if (s > kMaxStrata) return -1;
  }
  return s;
}

bool edges_ok(const int64_t* edges, int32_t n_edges) {
  if (n_edges < 0 || n_edges > kMaxEdges || (n_edges > 0 && !edges)) return false;
  for (int j = 0; j < n_edges; ++j)
    if (edges[j] < 1 || edges[j] == INT64_MAX || (j > 0 && edges[j] <= edges[j - 1])) return false;
  return true;
}

GapEdges make_edges(int32_t k, const int64_t* edges, int32_t n_edges) {
  GapEdges g;
  for (int j = 0; j < kMaxEdges; ++j) g.e[j] = j < n_edges ? edges[j] : INT64_MAX;
  g.G = n_edges + 1;
  g.k = k;
  return g;
}

bool planes_ok(int32_t planes) { return (planes & kPlaneMask) != 0 && (planes & ~(kPlaneMask | MATCHA_GAP_DIRECT)) == 0; }

GapPlan make_gplan(int64_t n_strata, int32_t planes) {
  GapPlan pl{};
  pl.n_strata = n_strata;
  size_t off = kHeaderBytes;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); ++pl.n_planes; return o; };
  if (planes & MATCHA_GAP_COUNT) pl.off_count = take((size_t)n_strata * 8);
  if (planes & MATCHA_GAP_SUM) pl.off_sum = take((size_t)n_strata * 8);
  if (planes & MATCHA_GAP_SUMSQ) pl.off_sumsq = take((size_t)n_strata * 8);
  pl.total = off;
  return pl;
}

struct GapView {
  unsigned long long* counters;                // {n_rows, n_rejected}
  unsigned long long *count, *sum, *sumsq;     // null = plane absent
};

GapView view_at(void* state, const GapPlan& pl) {
  char* w = (char*)state;
  GapView v;
  v.counters = (unsigned long long*)w;
  v.count = pl.off_count ? (unsigned long long*)(w + pl.off_count) : nullptr;
  v.sum = pl.off_sum ? (unsigned long long*)(w + pl.off_sum) : nullptr;
  v.sumsq = pl.off_sumsq ? (unsigned long long*)(w + pl.off_sumsq) : nullptr;
  return v;
}

__device__ __forceinline__ int32_t gap_class(const GapEdges& ge, int64_t gap) {
  int32_t c = 0;
#pragma unroll
  for (int j = 0; j < kMaxEdges; ++j) c += gap >= ge.e[j] ? 1 : 0;
  return c;
}

// the stratum of the row at x (L ids), kNoStratum for an invalid row
template <int L>
__device__ __forceinline__ int32_t stratum_of(const GapEdges& ge, const int64_t* __restrict__ x) {
  int64_t prev = x[0];
  bool ok = prev > 0, zero = false;
  int32_t run = ok ? 1 : 0, s = 0;
#pragma unroll
  for (int c = 1; c < L; ++c) {
    const int64_t id = x[c];
    if (id == 0) {
      zero = true;
    } else if (zero || id <= prev) {
      ok = false;                              // a hole, a repeated id or a descent
    } else {
      s = s * ge.G + gap_class(ge, (int64_t)((uint64_t)id - (uint64_t)prev));      // a valid row has prev > 0: the difference is exact
      ++run;
      prev = id;
    }
  }
  return ok && run == ge.k ? s : kNoStratum;
}

__global__ __launch_bounds__(kBlock) void gap_stats_init_kernel(unsigned long long* __restrict__ p, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n8; i += (int64_t)gridDim.x * kBlock) p[i] = 0ull;
}

// Every lane of a wavefront runs the whole body (lanes past n carry a dead row): the shuffles and ballots below read all 64 lanes.
// LDS: the block's copy of the planes, [plane present][n_strata] in the order COUNT, SUM, SUMSQ (dynamic shared memory).
template <int L, bool LDS>
__global__ __launch_bounds__(kBlock) void gap_stats_update_kernel(GapView gv, GapEdges ge, int32_t n_strata, double scale, float vmax,
                                                                  const int64_t* __restrict__ x, const float* __restrict__ value,
                                                                  const int32_t* __restrict__ skip, int64_t n) {
  extern __shared__ unsigned long long gap_lds[];
  unsigned long long* const l_count = gap_lds;
  unsigned long long* const l_sum = l_count + (gv.count ? n_strata : 0);
  unsigned long long* const l_sumsq = l_sum + (gv.sum ? n_strata : 0);
  const int n_lds = n_strata * ((gv.count ? 1 : 0) + (gv.sum ? 1 : 0) + (gv.sumsq ? 1 : 0));
  if (LDS) {
    for (int j = threadIdx.x; j < n_lds; j += kBlock) gap_lds[j] = 0ull;
    __syncthreads();
  }
  const int lane = threadIdx.x & (kWave - 1);
  uint32_t n_rows = 0, n_rej = 0;                                        // this wavefront's totals (identical in every lane)
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {
    const int64_t i = base + threadIdx.x;
    float v = 0.f;
    int32_t s = kNoStratum;
    bool live = false, rejected = false;
    if (i < n) {
      const bool skipped = skip && skip[i] != 0;
      v = value[i];
      s = stratum_of<L>(ge, x + i * L);
      const bool ok = s >= 0 && v >= 0.f && v <= vmax;                   // false for NaN
      live = !skipped && ok;
      rejected = !skipped && !ok;
    }
    const uint64_t live_mask = __ballot(live);
    n_rows += (uint32_t)__popcll(live_mask);
    n_rej += (uint32_t)__popcll(__ballot(rejected));
    if (live_mask == 0) continue;                                        // uniform within the wavefront
    v = live ? v + 0.f : 0.f;                                            // -0.0 -> +0.0
    s = live ? s : kNoStratum;
    // inclusive prefix over the lanes of (q, q2, count): at most 64 rows; unsigned arithmetic wraps like the planes do
    const double dv = (double)v;
    unsigned long long pq = live ? (unsigned long long)__double2ll_rn(dv * scale) : 0ull;
    unsigned long long p2 = live && gv.sumsq ? (unsigned long long)__double2ll_rn(dv * dv * scale) : 0ull;
    uint32_t pc = live ? 1u : 0u;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const unsigned long long tq = __shfl_up(pq, d, kWave);
      const unsigned long long t2 = __shfl_up(p2, d, kWave);
      const uint32_t tc = __shfl_up(pc, d, kWave);
      if (lane >= d) { pq += tq; p2 += t2; pc += tc; }
    }
    const int32_t below = __shfl_up(s, 1, kWave);
    const bool head = lane == 0 || s != below || s == kNoStratum;
    const uint64_t heads = __ballot(head);                               // bit 0 is always set
    const int first = 63 - __clzll(heads & (~0ull >> (63 - lane)));      // the head of this lane's run
    const bool last = lane == kWave - 1 || ((heads >> (lane + 1)) & 1ull);
    const int src = first > 0 ? first - 1 : 0;
    unsigned long long rq = __shfl(pq, src, kWave);
    unsigned long long r2 = __shfl(p2, src, kWave);
    uint32_t rc = __shfl(pc, src, kWave);
    rq = first > 0 ? pq - rq : pq;
    r2 = first > 0 ? p2 - r2 : p2;
    rc = first > 0 ? pc - rc : pc;
    if (last && s != kNoStratum) {                                       // a live row has exactly k - 1 gaps: 0 <= s < G^(k-1) = n_strata
      if (LDS) {
        if (gv.count) atomicAdd(l_count + s, (unsigned long long)rc);
        if (gv.sum) atomicAdd(l_sum + s, rq);
        if (gv.sumsq) atomicAdd(l_sumsq + s, r2);
      } else {
        if (gv.count) atomicAdd(gv.count + s, (unsigned long long)rc);
        if (gv.sum) atomicAdd(gv.sum + s, rq);
        if (gv.sumsq) atomicAdd(gv.sumsq + s, r2);
      }
    }
  }
  if (lane == 0) {
    if (n_rows) atomicAdd(gv.counters, (unsigned long long)n_rows);
    if (n_rej) atomicAdd(gv.counters + 1, (unsigned long long)n_rej);
  }
  if (LDS) {
    __syncthreads();
    for (int j = threadIdx.x; j < n_strata; j += kBlock) {
      if (gv.count) { const unsigned long long t = l_count[j]; if (t) atomicAdd(gv.count + j, t); }
      if (gv.sum) { const unsigned long long t = l_sum[j]; if (t) atomicAdd(gv.sum + j, t); }
      if (gv.sumsq) { const unsigned long long t = l_sumsq[j]; if (t) atomicAdd(gv.sumsq + j, t); }
    }
  }
}

__global__ __launch_bounds__(kBlock) void gap_stats_read_kernel(GapView gv, int64_t n_strata, int64_t* __restrict__ count_out, int64_t* __restrict__ sum_out,
                                                                int64_t* __restrict__ sumsq_out, int64_t* __restrict__ counters_out) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n_strata; p += (int64_t)gridDim.x * kBlock) {
    if (count_out) count_out[p] = (int64_t)gv.count[p];
    if (sum_out) sum_out[p] = (int64_t)gv.sum[p];
    if (sumsq_out) sumsq_out[p] = (int64_t)gv.sumsq[p];
  }
  if (counters_out && blockIdx.x == 0 && threadIdx.x < 2) counters_out[threadIdx.x] = (int64_t)gv.counters[threadIdx.x];
}

template <int L>
__global__ __launch_bounds__(kBlock) void gap_enrich_kernel(GapEdges ge, const int64_t* __restrict__ x, int64_t n, const float* __restrict__ score,
                                                            const float* __restrict__ offset, const float* __restrict__ scale,
                                                            int32_t* __restrict__ stratum_out, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const int32_t s = stratum_of<L>(ge, x + i * L);
    if (stratum_out) stratum_out[i] = s;
    if (score) out[i] = s >= 0 ? __fmul_rn(__fsub_rn(score[i], offset[s]), scale[s]) : __builtin_nanf("");
  }
}

template <int L>
void launch_stats(bool lds, unsigned blocks, size_t lds_bytes, hipStream_t st, const GapView& gv, const GapEdges& ge, int32_t n_strata, double scale,
                  float vmax, const int64_t* x, const float* value, const int32_t* skip, int64_t n) {
  if (lds)
    hipLaunchKernelGGL((gap_stats_update_kernel<L, true>), dim3(blocks), dim3(kBlock), lds_bytes, st, gv, ge, n_strata, scale, vmax, x, value, skip, n);
  else
    hipLaunchKernelGGL((gap_stats_update_kernel<L, false>), dim3(blocks), dim3(kBlock), 0, st, gv, ge, n_strata, scale, vmax, x, value, skip, n);
}

template <int L>
void launch_enrich(unsigned blocks, hipStream_t st, const GapEdges& ge, const int64_t* x, int64_t n, const float* score, const float* offset,
                   const float* scale, int32_t* stratum_out, float* out) {
  hipLaunchKernelGGL(gap_enrich_kernel<L>, dim3(blocks), dim3(kBlock), 0, st, ge, x, n, score, offset, scale, stratum_out, out);
}

unsigned grid_for(int64_t n, int64_t cap) {
  int64_t nb = cdiv(n, kBlock);
  return (unsigned)(nb > cap ? cap : nb);
}

}  // namespace
}  // namespace matcha

using namespace matcha;

extern "C" int64_t matcha_gap_strata_count(int32_t k, int32_t n_edges) { return strata_count(k, n_edges); }

extern "C" size_t matcha_gap_stats_bytes(int32_t k, int32_t n_edges, int32_t planes) {
  const int64_t ns = strata_count(k, n_edges);
  if (ns < 0 || !planes_ok(planes)) return 0;
  return make_gplan(ns, planes).total;
}

#define GAP_SHAPE_ARGS(fn)                                                                                                               \
  MATCHA_CHECK_ARG(k >= 2 && k <= MATCHA_MAX_L, fn ": k=%d must be in [2, %d]", k, MATCHA_MAX_L);                                         \
  MATCHA_CHECK_ARG(n_edges >= 0 && n_edges <= kMaxEdges, fn ": n_edges=%d must be in [0, %d]", n_edges, kMaxEdges);                       \
  const int64_t n_strata = strata_count(k, n_edges);                                                                                     \
  MATCHA_CHECK_ARG(n_strata >= 1, fn ": (n_edges + 1)^(k - 1) strata exceed 2^20 (k=%d n_edges=%d)", k, n_edges)

#define GAP_STATE_ARGS(fn)                                                                                                               \
  GAP_SHAPE_ARGS(fn);                                                                                                                    \
  MATCHA_CHECK_ARG(planes_ok(planes), fn ": planes=%d is not a mask of COUNT 1, SUM 2, SUMSQ 4 (and DIRECT 8)", planes);                 \
  MATCHA_CHECK_ARG(state, fn ": null state");                                                                                            \
  MATCHA_CHECK_ARG(((uintptr_t)state) % 8 == 0, fn ": state must be 8-byte aligned");                                                    \
  const GapPlan pl = make_gplan(n_strata, planes);                                                                                       \
  MATCHA_CHECK_ARG(bytes == pl.total, fn ": state of %zu bytes, matcha_gap_stats_bytes says %zu", bytes, pl.total)

#define GAP_EDGE_ARGS(fn)                                                                                                                \
  MATCHA_CHECK_ARG(edges_ok(edges, n_edges), fn ": the %d edges must be positive and strictly ascending", n_edges);                      \
  MATCHA_CHECK_ARG(L >= k && L <= MATCHA_MAX_L, fn ": row width L=%d must be in [k=%d, %d]", L, k, MATCHA_MAX_L);                         \
  MATCHA_CHECK_ARG(n >= 0 && n <= ((int64_t)1 << 40), fn ": n=%lld out of range", (long long)n)

extern "C" int matcha_gap_stats_init(void* state, size_t bytes, int32_t k, int32_t n_edges, int32_t planes, matcha_stream_t stream) {
  GAP_STATE_ARGS("matcha_gap_stats_init");
  const int64_t n8 = (int64_t)(pl.total / 8);                            // every offset is a multiple of 256
  hipLaunchKernelGGL(gap_stats_init_kernel, dim3(grid_for(n8, 1 << 14)), dim3(kBlock), 0, (hipStream_t)stream, (unsigned long long*)state, n8);
  MATCHA_CHECK_LAUNCH("gap_stats_init_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_gap_stats_update(void* state, size_t bytes, int32_t k, const int64_t* edges, int32_t n_edges, int32_t planes, int32_t shift,
                                       float vmax, const int64_t* x, int32_t L, const float* value, const int32_t* skip, int64_t n,
                                       matcha_stream_t stream) {
  GAP_STATE_ARGS("matcha_gap_stats_update");
  GAP_EDGE_ARGS("matcha_gap_stats_update");
  MATCHA_CHECK_ARG(shift >= 16 && shift <= 32, "matcha_gap_stats_update: shift=%d must be in [16, 32]", shift);
  MATCHA_CHECK_ARG(vmax > 0.f && vmax <= 1048576.f, "matcha_gap_stats_update: vmax=%g must be in (0, 2^20]", (double)vmax);      // NaN fails both
  const double scale = std::ldexp(1.0, shift);
  MATCHA_CHECK_ARG(!(planes & MATCHA_GAP_SUMSQ) || (double)vmax * (double)vmax * scale <= 4611686018427387904.0,
                   "matcha_gap_stats_update: with SUMSQ one row's vmax^2 2^shift must stay within 2^62 (vmax=%g shift=%d)", (double)vmax, shift);
  if (n == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(x && value, "matcha_gap_stats_update: null x or value");
  const GapView gv = view_at(state, pl);
  const GapEdges ge = make_edges(k, edges, n_edges);
  const size_t lds_bytes = (size_t)n_strata * 8 * pl.n_planes;
  const bool lds = !(planes & MATCHA_GAP_DIRECT) && lds_bytes <= kLdsBudget;
  const unsigned blocks = grid_for(n, lds ? 512 : 1 << 14);              // a block flushes its LDS copy once: no more blocks than stay resident
  hipStream_t st = (hipStream_t)stream;
  const int32_t ns = (int32_t)n_strata;
  switch (L) {
    case 2: launch_stats<2>(lds, blocks, lds_bytes, st, gv, ge, ns, scale, vmax, x, value, skip, n); break;
    case 3: launch_stats<3>(lds, blocks, lds_bytes, st, gv, ge, ns, scale, vmax, x, value, skip, n); break;
    case 4: launch_stats<4>(lds, blocks, lds_bytes, st, gv, ge, ns, scale, vmax, x, value, skip, n); break;
    case 5: launch_stats<5>(lds, blocks, lds_bytes, st, gv, ge, ns, scale, vmax, x, value, skip, n); break;
    case 6: launch_stats<6>(lds, blocks, lds_bytes, st, gv, ge, ns, scale, vmax, x, value, skip, n); break;
    case 7: launch_stats<7>(lds, blocks, lds_bytes, st, gv, ge, ns, scale, vmax, x, value, skip, n); break;
    default: launch_stats<8>(lds, blocks, lds_bytes, st, gv, ge, ns, scale, vmax, x, value, skip, n); break;
  }
  MATCHA_CHECK_LAUNCH(lds ? "gap_stats_update_kernel" : "gap_stats_update_direct_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_gap_stats_read(const void* state, size_t bytes, int32_t k, int32_t n_edges, int32_t planes, int64_t* count_out, int64_t* sum_out,
                                     int64_t* sumsq_out, int64_t* counters_out, matcha_stream_t stream) {
  GAP_STATE_ARGS("matcha_gap_stats_read");
  MATCHA_CHECK_ARG((!count_out || (planes & MATCHA_GAP_COUNT)) && (!sum_out || (planes & MATCHA_GAP_SUM)) && (!sumsq_out || (planes & MATCHA_GAP_SUMSQ)),
                   "matcha_gap_stats_read: an output for a plane that the mask %d does not hold", planes);
  MATCHA_CHECK_ARG(count_out || sum_out || sumsq_out || counters_out, "matcha_gap_stats_read: null outputs");
  hipLaunchKernelGGL(gap_stats_read_kernel, dim3(grid_for(n_strata, 1 << 12)), dim3(kBlock), 0, (hipStream_t)stream, view_at((void*)state, pl), n_strata,
                     count_out, sum_out, sumsq_out, counters_out);
  MATCHA_CHECK_LAUNCH("gap_stats_read_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_gap_enrich(int32_t k, const int64_t* edges, int32_t n_edges, const int64_t* x, int64_t n, int32_t L, const float* score,
                                 const float* offset, const float* scale, int32_t* stratum_out, float* out, matcha_stream_t stream) {
  GAP_SHAPE_ARGS("matcha_gap_enrich");
  GAP_EDGE_ARGS("matcha_gap_enrich");
  MATCHA_CHECK_ARG(score ? (offset && scale && out) : (!offset && !scale && !out && stratum_out),
                   "matcha_gap_enrich: score, offset, scale and out go together; without them stratum_out is required");
  if (n == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(x, "matcha_gap_enrich: null x");
  const GapEdges ge = make_edges(k, edges, n_edges);
  const unsigned blocks = grid_for(n, 1 << 14);
  hipStream_t st = (hipStream_t)stream;
  switch (L) {
    case 2: launch_enrich<2>(blocks, st, ge, x, n, score, offset, scale, stratum_out, out); break;
    case 3: launch_enrich<3>(blocks, st, ge, x, n, score, offset, scale, stratum_out, out); break;
    case 4: launch_enrich<4>(blocks, st, ge, x, n, score, offset, scale, stratum_out, out); break;
    case 5: launch_enrich<5>(blocks, st, ge, x, n, score, offset, scale, stratum_out, out); break;
    case 6: launch_enrich<6>(blocks, st, ge, x, n, score, offset, scale, stratum_out, out); break;
    case 7: launch_enrich<7>(blocks, st, ge, x, n, score, offset, scale, stratum_out, out); break;
    default: launch_enrich<8>(blocks, st, ge, x, n, score, offset, scale, stratum_out, out); break;
  }
  MATCHA_CHECK_LAUNCH("gap_enrich_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_gap_strata_ids(int32_t k, const int64_t* edges, int32_t n_edges, const int64_t* x, int64_t n, int32_t L, int32_t* stratum_out,
                                     matcha_stream_t stream) {
  MATCHA_CHECK_ARG(stratum_out, "matcha_gap_strata_ids: null stratum_out");
  return matcha_gap_enrich(k, edges, n_edges, x, n, L, nullptr, nullptr, nullptr, stratum_out, nullptr, stream);
}
