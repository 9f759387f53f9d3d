// The support of cluster decomposition's choices (the choices and their ranks are sweep_rows.hip's
// cluster_subset_rows_kernel's): two planes of uint64 cells -- fixed-point sums (rint(double(v) 2^32), PairMap's) and counts of the accepted
// rows -- per cluster and position (matcha_subset_support_*, S cells per cluster) or per cluster and pair of positions
// (matcha_subset_pair_*, P = S (S - 1) / 2 cells).  Both states are a header of two counters (rows accepted, rows rejected) and the two
// planes; init zeroes, read copies, and the two update kernels share their row intake, run arithmetic and epilogues.  A row is accepted
// when it is not skipped and 0 <= v <= vmax; it is rejected (counted, not added) when it is not skipped and v is outside or NaN.
//
//   subset_support_update_kernel  per cluster and position, the fixed-point sum (rint(double(v) 2^32), PairMap's) and the number of the
//                                 accepted rows whose choice contains the position; it unranks the choice itself and never reads a row.
//                                 A block serves runs of kSupRun consecutive ranks, hence of consecutive clusters: it accumulates into
//                                 an LDS tile of (clusters of the run) x S cells per plane with LDS integer atomics and issues one global
//                                 atomic per touched cell; clusters of the run beyond the tile go to global atomics directly.  Integer
//                                 atomics only: the state does not depend on arrival order or on how the stream is cut.
//
// Per-pair support.  Per cluster and PAIR of positions i < j, the same two quantities over the accepted rows whose choice
// contains both: two planes of A P cells, the upper triangle packed row-major: cell a P + i (2 S - i - 1) / 2 + (j - i - 1).
//
//   subset_pair_update_kernel  the support kernel's structure and row handling; an accepted row adds to the C(m, 2) <= 28 cells of its
//                              choice.  m = 2: the choice IS one pair and its lexicographic rank is the packed index, so the row's
//                              cell is its global rank g -- no unranking, no tile, one coalesced global atomic per plane.  m >= 3: a
//                              block's run of kPairRun consecutive ranks accumulates into an LDS tile of kPairTile cells per plane
//                              (uint64 sums; uint32 counts, a run adds at most kPairRun to a cell) and flushes one global atomic per
//                              touched cell; clusters of the run beyond the tile (only where C(S, m) <= P: m >= S - 2) go to global
//                              atomics directly.  Sizes: 2 048 cells are 16 KB + 8 KB = 24 KB of LDS per block, six blocks (24 of
//                              32 wavefronts) per CU of 160 KB, and hold 4 clusters of 32 loci (496 cells), 56 of 9; a run of 2 048
//                              ranks is 8 rows per thread, as in the support kernel.  Integer atomics only.
#include <hip/hip_runtime.h>

#include "sweep_rank.hpp"

namespace matcha {
namespace {

constexpr int kSupRun = 2048;                  // consecutive ranks per block run: 8 rows per thread
constexpr int kSupTile = 1024;                 // cells per LDS plane (2 planes x 8 KB): 32 clusters of 32 ids, 341 of 3
constexpr size_t kSupHeader = 256;             // int64 n_rows, int64 n_rejected, padding
constexpr int kPairRun = 2048;
constexpr int kPairTile = 2048;

typedef unsigned long long u64;

struct PlanePlan {
  size_t off_sum, off_count, total;
  int64_t cells;
};

bool support_args_ok(int64_t A, int32_t S, int32_t m, int32_t m_min, float vmax) {
  return A >= 1 && A <= ((int64_t)1 << 40) && S >= 2 && S <= kMaxWide && m >= m_min && m <= kMaxK && vmax > 0.f && vmax <= 1048576.f;   // NaN fails
}

int32_t pair_cells(int32_t S) { return S * (S - 1) / 2; }              // P <= 496, so A P < 2^49

PlanePlan make_plan(int64_t cells) {
  PlanePlan pl{};
  pl.cells = cells;
  pl.off_sum = kSupHeader;
  pl.off_count = pl.off_sum + align_up((size_t)pl.cells * 8, 256);
  pl.total = pl.off_count + align_up((size_t)pl.cells * 8, 256);
  return pl;
}

__global__ __launch_bounds__(256) void subset_plane_init_kernel(u64* __restrict__ p, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) p[i] = 0ull;
}

// Row i of the stream (in_run: it lies in the block's run): true when the row is accepted, q = its value in fixed point.  Counts the
// wavefront's accepted and rejected rows: the ballots read all 64 lanes, so every lane calls this, the ones behind the run too.
__device__ __forceinline__ bool plane_intake(const float* __restrict__ value, const int32_t* __restrict__ skip, int64_t i, bool in_run, float vmax,
                                             uint32_t& n_rows, uint32_t& n_rej, u64& q) {
  float v = 0.f;
  bool live = false, rejected = false;
  if (in_run) {
    const bool skipped = skip && skip[i] != 0;
    v = value[i];
    const bool okv = v >= 0.f && v <= vmax;                             // false for NaN
    live = !skipped && okv;
    rejected = !skipped && !okv;
  }
  n_rows += (uint32_t)__popcll(__ballot(live));
  n_rej += (uint32_t)__popcll(__ballot(rejected));
  if (live) {
    v = v + 0.f;                                                        // -0.0 -> +0.0
    q = (u64)__double2ll_rn((double)v * 4294967296.0);
  }
  return live;
}

// The clusters of a run of len ranks from g: the first one, and how many of them the tile holds
__device__ __forceinline__ uint64_t run_span(uint64_t g, int len, uint64_t cm, uint64_t tile_clusters, uint64_t& a_first) {
  a_first = g / cm;
  const uint64_t a_last = (g + (uint64_t)len - 1) / cm;
  return a_last - a_first + 1 < tile_clusters ? a_last - a_first + 1 : tile_clusters;
}

// One global atomic per touched cell of the tile; sum / cnt point at the run's first cluster
template <class CountT>
__device__ __forceinline__ void flush_plane_tile(const u64* tsum, const CountT* tcnt, int cells, u64* __restrict__ sum, u64* __restrict__ cnt) {
  __syncthreads();
  for (int e = threadIdx.x; e < cells; e += 256) {
    const CountT c = tcnt[e];
    if (c) {
      atomicAdd(sum + e, tsum[e]);
      atomicAdd(cnt + e, (u64)c);
    }
  }
  __syncthreads();                                                      // the tile is reused by the next run
}

// the wavefront's totals are identical in every lane
__device__ __forceinline__ void add_counters(u64* __restrict__ counters, uint32_t n_rows, uint32_t n_rej) {
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (n_rows) atomicAdd(counters, (u64)n_rows);
    if (n_rej) atomicAdd(counters + 1, (u64)n_rej);
  }
}

// Every lane of a wavefront runs the whole body: the trip counts depend on the block's run only, the ballots read all 64 lanes.
__global__ __launch_bounds__(256) void subset_support_update_kernel(u64* __restrict__ counters, u64* __restrict__ sum, u64* __restrict__ cnt, int32_t S,
                                                                    int32_t m, uint64_t cm, float vmax, const float* __restrict__ value,
                                                                    const int32_t* __restrict__ skip, int64_t n, int64_t g0) {
  __shared__ u64 tsum[kSupTile], tcnt[kSupTile];
  const uint64_t tile_clusters = (uint64_t)(kSupTile / S);              // >= 32
  uint32_t n_rows = 0, n_rej = 0;                                       // this wavefront's totals (identical in every lane)
  const int64_t runs = (n + kSupRun - 1) / kSupRun;
  for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
    const int64_t i0 = run * kSupRun;
    const int len = n - i0 < kSupRun ? (int)(n - i0) : kSupRun;
    uint64_t a_first;
    const uint64_t span = run_span((uint64_t)(g0 + i0), len, cm, tile_clusters, a_first);
    const int cells = (int)span * S;                                    // <= kSupTile
    for (int e = threadIdx.x; e < cells; e += 256) { tsum[e] = 0ull; tcnt[e] = 0ull; }
    __syncthreads();
    for (int off = 0; off < len; off += 256) {
      const int at = off + (int)threadIdx.x;
      u64 q = 0;
      if (plane_intake(value, skip, i0 + at, at < len, vmax, n_rows, n_rej, q)) {
        uint64_t a, r;
        split_rank((uint64_t)(g0 + i0 + at), cm, a, r);
        int32_t y[kMaxK] = {0, 0, 0, 0, 0, 0, 0, 0};
        unrank(r, cm, S, m, y);
        const uint64_t rel = a - a_first;
        const bool tiled = rel < span;
#pragma unroll
        for (int c = 0; c < kMaxK; ++c) {
          if (c < m) {
            if (tiled) {
              const int e = (int)rel * S + y[c];                        // < span S
              atomicAdd(&tsum[e], q);
              atomicAdd(&tcnt[e], 1ull);
            } else {
              const uint64_t e = a * (uint64_t)S + (uint64_t)y[c];      // a < A: the host checked g0 + n <= A cm
              atomicAdd(sum + e, q);
              atomicAdd(cnt + e, 1ull);
            }
          }
        }
      }
    }
    flush_plane_tile(tsum, tcnt, cells, sum + a_first * (uint64_t)S, cnt + a_first * (uint64_t)S);
  }
  add_counters(counters, n_rows, n_rej);
}

// Every lane of a wavefront runs the whole body: the trip counts depend on the block's run only (m is the launch's), the ballots read
// all 64 lanes and every barrier is reached by all four wavefronts.
__global__ __launch_bounds__(256) void subset_pair_update_kernel(u64* __restrict__ counters, u64* __restrict__ sum, u64* __restrict__ cnt, int32_t S, int32_t P,
                                                                 int32_t m, uint64_t cm, float vmax, const float* __restrict__ value,
                                                                 const int32_t* __restrict__ skip, int64_t n, int64_t g0) {
  __shared__ u64 tsum[kPairTile];
  __shared__ unsigned int tcnt[kPairTile];
  const bool direct = m == 2;                                           // cm == P and the choice's rank is its cell
  const uint64_t tile_clusters = (uint64_t)(kPairTile / P);             // >= 4
  uint32_t n_rows = 0, n_rej = 0;                                       // this wavefront's totals (identical in every lane)
  const int64_t runs = (n + kPairRun - 1) / kPairRun;
  for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
    const int64_t i0 = run * kPairRun;
    const int len = n - i0 < kPairRun ? (int)(n - i0) : kPairRun;
    uint64_t a_first;
    const uint64_t span = run_span((uint64_t)(g0 + i0), len, cm, tile_clusters, a_first);
    const int cells = direct ? 0 : (int)span * P;                       // <= kPairTile
    for (int e = threadIdx.x; e < cells; e += 256) { tsum[e] = 0ull; tcnt[e] = 0u; }
    __syncthreads();
    for (int off = 0; off < len; off += 256) {
      const int at = off + (int)threadIdx.x;
      u64 q = 0;
      if (plane_intake(value, skip, i0 + at, at < len, vmax, n_rows, n_rej, q)) {
        if (direct) {
          const uint64_t e = (uint64_t)(g0 + i0 + at);                  // < A cm = A P: the host checked g0 + n <= A cm
          atomicAdd(sum + e, q);
          atomicAdd(cnt + e, 1ull);
        } else {
          uint64_t a, r;
          split_rank((uint64_t)(g0 + i0 + at), cm, a, r);
          int32_t y[kMaxK] = {0, 0, 0, 0, 0, 0, 0, 0};
          unrank(r, cm, S, m, y);                                       // ascending, every y[c] < S for c < m
          const uint64_t rel = a - a_first;
          const bool tiled = rel < span;
          const int tbase = tiled ? (int)rel * P : 0;
          const uint64_t gbase = a * (uint64_t)P;                       // a < A
#pragma unroll
          for (int c = 0; c < kMaxK - 1; ++c) {
            const int row = y[c] * (2 * S - y[c] - 1) / 2 - y[c] - 1;   // + j: the cell of (y[c], j), j > y[c]
#pragma unroll
            for (int d = c + 1; d < kMaxK; ++d) {
              if (d < m) {
                const int e = row + y[d];                               // in [0, P)
                if (tiled) {
                  atomicAdd(&tsum[tbase + e], q);                       // tbase + e < span P
                  atomicAdd(&tcnt[tbase + e], 1u);
                } else {
                  atomicAdd(sum + gbase + (uint64_t)e, q);
                  atomicAdd(cnt + gbase + (uint64_t)e, 1ull);
                }
              }
            }
          }
        }
      }
    }
    flush_plane_tile(tsum, tcnt, cells, sum + a_first * (uint64_t)P, cnt + a_first * (uint64_t)P);
  }
  add_counters(counters, n_rows, n_rej);
}

__global__ __launch_bounds__(256) void subset_plane_read_kernel(const u64* __restrict__ counters, const u64* __restrict__ sum, const u64* __restrict__ cnt,
                                                                int64_t cells, int64_t* __restrict__ sum_out, int64_t* __restrict__ count_out,
                                                                int64_t* __restrict__ counters_out) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < cells; p += (int64_t)gridDim.x * 256) {
    if (sum_out) sum_out[p] = (int64_t)sum[p];
    if (count_out) count_out[p] = (int64_t)cnt[p];
  }
  if (counters_out && blockIdx.x == 0 && threadIdx.x < 2) counters_out[threadIdx.x] = (int64_t)counters[threadIdx.x];
}

unsigned plane_grid(int64_t items, int per_block) {
  const int64_t blocks = cdiv(items, per_block);
  return (unsigned)(blocks > (1 << 14) ? 1 << 14 : blocks);
}

// The three bodies behind the eight state-taking entries: pair = 0 is matcha_subset_support_*, pair = 1 matcha_subset_pair_*.  The launch
// log keeps the entry's kernel names.
int plane_init(int pair, void* state, const PlanePlan& pl, matcha_stream_t stream) {
  const int64_t n8 = (int64_t)(pl.total / 8);                            // every offset is a multiple of 256
  hipLaunchKernelGGL(subset_plane_init_kernel, dim3(plane_grid(n8, 256)), dim3(256), 0, (hipStream_t)stream, (u64*)state, n8);
  MATCHA_CHECK_LAUNCH(pair ? "subset_pair_init_kernel" : "subset_support_init_kernel");
  return MATCHA_OK;
}

int plane_update(int pair, void* state, const PlanePlan& pl, int64_t A, int32_t S, int32_t m, float vmax, const float* value, const int32_t* skip, int64_t n,
                 int64_t g0, matcha_stream_t stream) {
  const char* fn = pair ? "matcha_subset_pair_update" : "matcha_subset_support_update";
  const int64_t cm = count_subsets(S, m);
  const int64_t total = A * cm;                                          // < 2^40 * 2^24
  MATCHA_CHECK_ARG(n >= 0 && n <= ((int64_t)1 << 40), "%s: n=%lld out of range", fn, (long long)n);
  MATCHA_CHECK_ARG(g0 >= 0 && g0 <= total && n <= total - g0, "%s: %lld ranks from %lld lie outside [0, %lld)", fn, (long long)n, (long long)g0,
                   (long long)total);
  if (n == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(value, "%s: null value", fn);
  char* w = (char*)state;
  u64 *counters = (u64*)w, *sum = (u64*)(w + pl.off_sum), *cnt = (u64*)(w + pl.off_count);
  if (pair) {
    hipLaunchKernelGGL(subset_pair_update_kernel, dim3(plane_grid(n, kPairRun)), dim3(256), 0, (hipStream_t)stream, counters, sum, cnt, S, pair_cells(S), m,
                       (uint64_t)cm, vmax, value, skip, n, g0);
    MATCHA_CHECK_LAUNCH("subset_pair_update_kernel");
  } else {
    hipLaunchKernelGGL(subset_support_update_kernel, dim3(plane_grid(n, kSupRun)), dim3(256), 0, (hipStream_t)stream, counters, sum, cnt, S, m, (uint64_t)cm,
                       vmax, value, skip, n, g0);
    MATCHA_CHECK_LAUNCH("subset_support_update_kernel");
  }
  return MATCHA_OK;
}

int plane_read(int pair, const void* state, const PlanePlan& pl, int64_t* sum_out, int64_t* count_out, int64_t* counters_out, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(sum_out || count_out || counters_out, "%s: null output", pair ? "matcha_subset_pair_read" : "matcha_subset_support_read");
  const char* w = (const char*)state;
  hipLaunchKernelGGL(subset_plane_read_kernel, dim3(plane_grid(pl.cells, 256)), dim3(256), 0, (hipStream_t)stream, (const u64*)w,
                     (const u64*)(w + pl.off_sum), (const u64*)(w + pl.off_count), pl.cells, sum_out, count_out, counters_out);
  MATCHA_CHECK_LAUNCH(pair ? "subset_pair_read_kernel" : "subset_support_read_kernel");
  return MATCHA_OK;
}

}  // namespace
}  // namespace matcha

using namespace matcha;

// What every state-taking entry checks first; declares the plan `pl`.  m_min: 1 for the per-locus planes, 2 for the per-pair ones.
#define PLANE_COMMON_ARGS(fn, bytes_fn, m_min, cells)                                                                               \
  MATCHA_CHECK_ARG(state, fn ": null state");                                                                                       \
  MATCHA_CHECK_ARG(support_args_ok(A, S, m, m_min, vmax), fn ": need 1 <= A <= 2^40, 2 <= S <= %d, %d <= m <= %d, 0 < vmax <= 2^20 " \
                                                             "(A=%lld S=%d m=%d vmax=%g)",                                          \
                   kMaxWide, m_min, kMaxK, (long long)A, S, m, (double)vmax);                                                       \
  MATCHA_CHECK_ARG(((uintptr_t)state) % 8 == 0, fn ": state must be 8-byte aligned");                                               \
  const PlanePlan pl = make_plan(cells);                                                                                            \
  MATCHA_CHECK_ARG(bytes >= pl.total, fn ": state too small (%zu bytes, " bytes_fn " says %zu)", bytes, pl.total)
#define SUPPORT_COMMON_ARGS(fn) PLANE_COMMON_ARGS(fn, "matcha_subset_support_bytes", 1, A * S)
#define PAIR_COMMON_ARGS(fn) PLANE_COMMON_ARGS(fn, "matcha_subset_pair_bytes", 2, A * pair_cells(S))

extern "C" size_t matcha_subset_support_bytes(int64_t A, int32_t S, int32_t m, float vmax) {
  return support_args_ok(A, S, m, 1, vmax) ? make_plan(A * S).total : 0;
}

extern "C" int matcha_subset_support_init(void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, matcha_stream_t stream) {
  SUPPORT_COMMON_ARGS("matcha_subset_support_init");
  return plane_init(0, state, pl, stream);
}

extern "C" int matcha_subset_support_update(void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, const float* value,
                                            const int32_t* skip, int64_t n, int64_t g0, matcha_stream_t stream) {
  SUPPORT_COMMON_ARGS("matcha_subset_support_update");
  return plane_update(0, state, pl, A, S, m, vmax, value, skip, n, g0, stream);
}

extern "C" int matcha_subset_support_read(const void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, int64_t* sum_out,
                                          int64_t* count_out, int64_t* counters_out, matcha_stream_t stream) {
  SUPPORT_COMMON_ARGS("matcha_subset_support_read");
  return plane_read(0, state, pl, sum_out, count_out, counters_out, stream);
}

extern "C" size_t matcha_subset_pair_bytes(int64_t A, int32_t S, int32_t m, float vmax) {
  return support_args_ok(A, S, m, 2, vmax) ? make_plan(A * pair_cells(S)).total : 0;
}

extern "C" int matcha_subset_pair_init(void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, matcha_stream_t stream) {
  PAIR_COMMON_ARGS("matcha_subset_pair_init");
  return plane_init(1, state, pl, stream);
}

extern "C" int matcha_subset_pair_update(void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, const float* value,
                                         const int32_t* skip, int64_t n, int64_t g0, matcha_stream_t stream) {
  PAIR_COMMON_ARGS("matcha_subset_pair_update");
  return plane_update(1, state, pl, A, S, m, vmax, value, skip, n, g0, stream);
}

extern "C" int matcha_subset_pair_read(const void* state, size_t bytes, int64_t A, int32_t S, int32_t m, float vmax, int64_t* sum_out,
                                       int64_t* count_out, int64_t* counters_out, matcha_stream_t stream) {
  PAIR_COMMON_ARGS("matcha_subset_pair_read");
  return plane_read(1, state, pl, sum_out, count_out, counters_out, stream);
}
