// Contact matrices of the adj front end from the clusters themselves: the reference's edgelist2adj (Code/process.py:90-105)
// and the History version's get_adjacency (History_version/Code/main_drop.py:543-563), accumulated on the device.
//
// Clusters arrive as CSR (ids int32 [I], offsets int64 [M + 1]; ids 1 .. N strictly ascending inside a cluster), with one int64 fixed-point
// weight q[c] = rint(w_c 2^32) per cluster and the inclusive prefix pair_ptr [M + 1] over p_c = s_c (s_c - 1) / 2.  Every pair i < j of a
// cluster adds q[c] to acc[(id_i - 1) N + (id_j - 1)], an int64 [N, N] matrix of which only the upper triangle is ever written.  Integer adds
// commute: acc does not depend on arrival order, on the order of the clusters or on how a cluster list is cut into calls.
//
//   cluster_pairs_update_kernel   the unit of work is the GLOBAL pair rank g in [0, pair_ptr[M]): every wavefront takes one contiguous run of
//                                 ranks, 64 at a time, so a cluster of 10 000 nodes and ten thousand clusters of 3 cost the same per pair.
//                                 The run's first cluster comes from a binary search in pair_ptr; from then on the wavefront walks forward:
//                                 it loads the next 64 cluster ends and every lane finds its cluster among them with shuffles.  The local
//                                 rank becomes (i < j) by tri_unrank (cluster_unrank.hpp); ranks of one row address ascending cells of one
//                                 matrix row.  One no-return 64-bit integer atomicAdd per pair.
//                                 A cluster is accepted when 1 <= id_i < id_j <= N holds for ALL its pairs (which is: ids strictly ascending
//                                 and in range).  A cluster whose pairs all lie in the wavefront's 64 ranks is judged by a ballot over those
//                                 lanes; one that is cut by the 64-rank window (at most the first and the last of a step) is scanned whole by
//                                 the wavefront, and the verdict on the last one is carried into the next step, so a large cluster is scanned
//                                 once per run of ranks.  A rejected cluster adds nothing and sets status[0] |= MATCHA_STATUS_BAD_ID; so does a
//                                 cluster whose offsets and pair_ptr disagree.  No id is used as an index before it is checked.
//   cluster_adj_finish_kernel     per 64 x 64 tile of the upper triangle: acc -> double(v) 2^-32 through a padded LDS tile, so that the cell
//                                 and its mirror both leave as coalesced rows; split by node2chrom into intra / inter (the other matrix's cell
//                                 and the diagonal are written 0), or everything into one matrix.  Overwrites its outputs.
//   block_colmax_normalise_kernel get_adjacency(norm=True): per block of rows and column, max over the block's rows, then
//                                 A[rows, col] /= (max + 1e-10) in float64 (IEEE division).  Lanes run along columns in both passes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cluster_unrank.hpp"
#include "kernels.hpp"
#include "sweep_rank.hpp"

namespace matcha {
namespace {

constexpr int kBlock = 256;
constexpr int kUpdateBlocks = 2048;          // 8 blocks of 4 wavefronts per compute unit; every wavefront owns one run of ranks
constexpr int kMaxBlocks = 1 << 14;
constexpr int kTile = 64;
constexpr int kTileLd = kTile + 1;           // doubles per LDS row: the transposed read walks a column without bank conflicts

// first index e in [lo, hi] with ptr[e] > g (ptr is non-decreasing and ptr[hi] > g)
__device__ __forceinline__ int64_t first_above(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi, int64_t g) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ptr[mid] > g) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// are ids[off .. off + s) strictly ascending and inside 1 .. N?  The whole wavefront calls it with the same arguments.
__device__ __forceinline__ bool wave_cluster_ok(const int32_t* __restrict__ ids, int64_t off, int32_t s, int32_t N, int lane) {
  bool bad = false;
  for (int32_t k = lane; k < s; k += kWave) {
    const int32_t a = ids[off + k];
    const int32_t b = k + 1 < s ? ids[off + k + 1] : 0;          // the last id only has to lie in 1 .. N
    bad |= a < 1 || a > N || (k + 1 < s && a >= b);
  }
  return __ballot(bad) == 0;
}

__global__ __launch_bounds__(kBlock) void cluster_pairs_update_kernel(const int32_t* __restrict__ ids, const int64_t* __restrict__ offsets,
                                                                      const int64_t* __restrict__ q, const int64_t* __restrict__ pair_ptr, int64_t M,
                                                                      int32_t N, unsigned long long* __restrict__ acc, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t P = pair_ptr[M];
  const int64_t n_ids = offsets[M];
  if (P <= 0) return;
  const int64_t waves = (int64_t)gridDim.x * (kBlock / kWave);
  const int64_t per = (P / waves / kWave + 1) * kWave;                       // ranks per wavefront, a multiple of 64
  const int64_t wid = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  const int64_t g0 = wid * per;
  if (g0 >= P) return;
  const int64_t g1 = P - g0 < per ? P : g0 + per;
  // the cluster of the run's first rank (the same search in every lane) and its first rank
  int64_t win = first_above(pair_ptr, 0, M, g0) - 1;
  int64_t win_start = pair_ptr[win];
  int64_t carry_c = -1;                                                      // the verdict on a cluster cut by the previous step
  bool carry_ok = false;
  bool any_bad = false;
  for (int64_t base = g0; base < g1; base += kWave) {
    const int64_t g = base + lane;
    const bool active = g < g1;
    // ---- the lane's cluster is win + (the number of ends pair_ptr[win + 1 + k] <= g among the next 64 clusters); all 64: the next window
    int64_t c = -1, start = 0, end = 0;
    bool found = !active;
    while (true) {
      const int64_t idx = win + 1 + lane;
      const int64_t e = idx <= M ? pair_ptr[idx] : INT64_MAX;
      int cnt = 0;                                                           // binary search over the lanes' sorted ends
#pragma unroll
      for (int step = 32; step > 0; step >>= 1) {
        const int64_t probe = shfl64(e, cnt + step - 1);
        if (probe <= g) cnt += step;
      }
      const int64_t last = shfl64(e, kWave - 1);
      if (last <= g) cnt = kWave;                                            // cnt is 63 here: the search covers 63 ends
      const int64_t below = shfl64(e, cnt > 0 ? cnt - 1 : 0);
      const int64_t mine = shfl64(e, cnt < kWave ? cnt : 0);
      if (!found && cnt < kWave) {
        found = true;
        c = win + cnt;
        start = cnt > 0 ? below : win_start;
        end = mine;
      }
      if (__ballot(!found) == 0) break;
      win += kWave;
      win_start = last;
    }
    const int n_act = g1 - base < kWave ? (int)(g1 - base) : kWave;
    win = shfl64(c, n_act - 1);                                              // the next step starts in or behind the last lane's cluster
    win_start = shfl64(start, n_act - 1);
    // ---- the pair and the lane's own verdict on it
    int64_t off = 0;
    int32_t s = 0, a = 0, b = 0;
    bool shape_ok = false, pair_ok = false;
    if (active) {
      off = offsets[c];
      const int64_t s64 = offsets[c + 1] - off;
      shape_ok = off >= 0 && s64 >= 2 && s64 <= kMaxClusterNodes && off <= n_ids - s64 && end - start == s64 * (s64 - 1) / 2 && start <= g && g < end;
      if (shape_ok) {
        s = (int32_t)s64;
        int32_t i, j;
        tri_unrank(g - start, s, i, j);
        a = ids[off + i];
        b = ids[off + j];
        pair_ok = a >= 1 && a < b && b <= N;
      }
    }
    // ---- the verdict on the lane's cluster.  Lanes of one cluster are adjacent: heads marks the first lane of every run.
    const int64_t c_below = shfl64(c, lane > 0 ? lane - 1 : 0);
    const uint64_t heads = __ballot(lane == 0 || c != c_below);
    const uint64_t bad_lanes = __ballot(active && !pair_ok);
    const int first = 63 - __clzll(heads & (~0ull >> (63 - lane)));
    const uint64_t after = lane == kWave - 1 ? 0ull : heads >> (lane + 1);
    const int run_end = after ? lane + 1 + (__ffsll((unsigned long long)after) - 1) : kWave;          // one past the run's last lane
    const uint64_t run_mask = (run_end == kWave ? ~0ull : (1ull << run_end) - 1ull) & ~((1ull << first) - 1ull);
    const bool whole = start == base + first && end == base + run_end;       // every pair of the cluster lies in this step
    bool ok = shape_ok && (bad_lanes & run_mask) == 0;
    // clusters cut by the window: the first lane's and the last active lane's.  Uniform control flow: both are read from fixed lanes.
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const int src = side == 0 ? 0 : n_act - 1;
      const int64_t cc = shfl64(c, src);
      const bool cut = __shfl((int)(shape_ok && !whole), src) != 0;
      if (side == 1 && cc == shfl64(c, 0)) break;                            // one cluster fills the step
      if (!cut) continue;
      bool verdict;
      if (cc == carry_c) {
        verdict = carry_ok;
      } else {
        verdict = wave_cluster_ok(ids, shfl64(off, src), __shfl(s, src), N, lane);
        carry_c = cc;
        carry_ok = verdict;
      }
      if (c == cc) ok = verdict;
    }
    if (active) {
      if (ok) atomicAdd(acc + ((int64_t)(a - 1) * N + (b - 1)), (unsigned long long)q[c]);
      else any_bad = true;
    }
  }
  if (status && __ballot(any_bad) != 0 && lane == 0) atomicOr(status, MATCHA_STATUS_BAD_ID);
}

// the 64 x 64 tile pair (ti <= tj) of rank t: the strict pair (ti, tj + 1) of T + 1 items
__device__ __forceinline__ void tile_of(int64_t t, int32_t T, int32_t& ti, int32_t& tj) {
  int32_t i, j;
  tri_unrank(t, T + 1, i, j);
  ti = i;
  tj = j - 1;
}

__global__ __launch_bounds__(kBlock) void cluster_adj_finish_kernel(const int64_t* __restrict__ acc, const int32_t* __restrict__ node2chrom, int32_t N,
                                                                    int32_t T, int64_t n_tiles, double* __restrict__ intra, double* __restrict__ inter) {
  __shared__ double tile[kTile * kTileLd];
  __shared__ int32_t chrom_i[kTile], chrom_j[kTile];
  const int col = threadIdx.x & (kTile - 1), row0 = threadIdx.x >> 6;      // a wavefront per row: 64 lanes x 8 contiguous bytes
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    int32_t ti, tj;
    tile_of(t, T, ti, tj);
    const int64_t r0 = (int64_t)ti * kTile, c0 = (int64_t)tj * kTile;
    __syncthreads();                                                         // the previous tile has been read
    if (inter && threadIdx.x < kTile) chrom_i[threadIdx.x] = r0 + threadIdx.x < N ? node2chrom[r0 + threadIdx.x + 1] : -1;
    if (inter && threadIdx.x >= kTile && threadIdx.x < 2 * kTile) chrom_j[col] = c0 + col < N ? node2chrom[c0 + col + 1] : -1;
    for (int r = row0; r < kTile; r += kBlock / kTile) {
      const int64_t gr = r0 + r, gc = c0 + col;
      double v = 0.0;
      if (gr < gc && gc < N) v = (double)acc[gr * N + gc] * (1.0 / 4294967296.0);       // gr < gc < N: only the upper triangle is read
      tile[r * kTileLd + col] = v;
    }
    __syncthreads();
    for (int r = row0; r < kTile; r += kBlock / kTile) {
      if (ti != tj) {
        {                                                                    // the cell (r0 + r, c0 + col)
          const int64_t gr = r0 + r, gc = c0 + col;
          if (gr < N && gc < N) {
            const double v = tile[r * kTileLd + col];
            const bool same = !inter || chrom_i[r] == chrom_j[col];
            intra[gr * N + gc] = same ? v : 0.0;
            if (inter) inter[gr * N + gc] = same ? 0.0 : v;
          }
        }
        {                                                                    // its mirror's row: (c0 + r, r0 + col)
          const int64_t gr = c0 + r, gc = r0 + col;
          if (gr < N && gc < N) {
            const double v = tile[col * kTileLd + r];
            const bool same = !inter || chrom_j[r] == chrom_i[col];
            intra[gr * N + gc] = same ? v : 0.0;
            if (inter) inter[gr * N + gc] = same ? 0.0 : v;
          }
        }
      } else {                                                               // a diagonal tile holds both triangles
        const int64_t gr = r0 + r, gc = c0 + col;
        if (gr < N && gc < N) {
          const double v = r < col ? tile[r * kTileLd + col] : r > col ? tile[col * kTileLd + r] : 0.0;
          const bool same = !inter || chrom_i[r] == chrom_j[col];
          intra[gr * N + gc] = same ? v : 0.0;
          if (inter) inter[gr * N + gc] = same ? 0.0 : v;
        }
      }
    }
  }
}

// One thread per (block of rows, column); consecutive threads own consecutive columns, so every row step of a wavefront is 512 contiguous bytes.
// colmax [n_ranges, N] keeps the maxima.  A NaN in a column's block gives a NaN maximum, as np.max does.
__global__ __launch_bounds__(kBlock) void block_colmax_normalise_kernel(double* __restrict__ A, int32_t N, const int64_t* __restrict__ ranges,
                                                                        int32_t n_ranges, double* __restrict__ colmax) {
  const int64_t col_blocks = ((int64_t)N + kBlock - 1) / kBlock;
  const int64_t items = (int64_t)n_ranges * col_blocks;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t k = it / col_blocks;
    const int64_t col = (it - k * col_blocks) * kBlock + threadIdx.x;
    int64_t lo = ranges[2 * k], hi = ranges[2 * k + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > N ? N : hi;
    if (col >= N || lo >= hi) continue;
    double m = A[lo * N + col];
    for (int64_t r = lo + 1; r < hi; ++r) {
      const double v = A[r * N + col];
      m = (v > m || v != v) ? v : m;
    }
    colmax[k * N + col] = m;
    const double d = m + 1e-10;
    for (int64_t r = lo; r < hi; ++r) A[r * N + col] = A[r * N + col] / d;
  }
}

}  // namespace
}  // namespace matcha

using namespace matcha;

extern "C" int64_t matcha_cluster_pairs_count(const int64_t* offsets_host, int64_t M) {
  if (!offsets_host || M < 0) return -1;
  unsigned __int128 total = 0;
  const unsigned __int128 lim = (unsigned __int128)1 << 63;
  for (int64_t c = 0; c < M; ++c) {
    const int64_t s = offsets_host[c + 1] - offsets_host[c];
    if (s < 0 || s > kMaxClusterNodes) return -1;
    total += (unsigned __int128)(s * (s - 1) / 2);
    if (total >= lim) return -1;
  }
  return (int64_t)total;
}

extern "C" int matcha_cluster_adj_update(const int32_t* ids, const int64_t* offsets, const int64_t* q, const int64_t* pair_ptr, int64_t M, int32_t n_nodes,
                                         int64_t* acc, int32_t* status, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(M >= 0 && M <= ((int64_t)1 << 40), "matcha_cluster_adj_update: M=%lld out of range", (long long)M);
  MATCHA_CHECK_ARG(n_nodes >= 1, "matcha_cluster_adj_update: n_nodes=%d must be >= 1", n_nodes);
  MATCHA_CHECK_ARG(acc, "matcha_cluster_adj_update: null acc");
  MATCHA_CHECK_ARG(((uintptr_t)acc) % 8 == 0, "matcha_cluster_adj_update: acc must be 8-byte aligned");
  if (M == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(ids && offsets && q && pair_ptr, "matcha_cluster_adj_update: null pointer (ids, offsets, q or pair_ptr)");
  hipLaunchKernelGGL(cluster_pairs_update_kernel, dim3(kUpdateBlocks), dim3(kBlock), 0, (hipStream_t)stream, ids, offsets, q, pair_ptr, M, n_nodes,
                     (unsigned long long*)acc, status);
  MATCHA_CHECK_LAUNCH("cluster_pairs_update_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_cluster_adj_finish(const int64_t* acc, const int32_t* node2chrom, int32_t n_nodes, double* intra, double* inter_or_null,
                                         matcha_stream_t stream) {
  MATCHA_CHECK_ARG(n_nodes >= 1, "matcha_cluster_adj_finish: n_nodes=%d must be >= 1", n_nodes);
  MATCHA_CHECK_ARG(acc && intra, "matcha_cluster_adj_finish: null pointer (acc or intra)");
  MATCHA_CHECK_ARG(!inter_or_null || node2chrom, "matcha_cluster_adj_finish: the split into intra / inter needs node2chrom");
  MATCHA_CHECK_ARG(inter_or_null != intra, "matcha_cluster_adj_finish: intra and inter must not alias");
  const int32_t T = (int32_t)cdiv(n_nodes, kTile);
  const int64_t n_tiles = (int64_t)T * (T + 1) / 2;
  const int64_t blocks = n_tiles > kMaxBlocks ? kMaxBlocks : n_tiles;
  hipLaunchKernelGGL(cluster_adj_finish_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, acc, node2chrom, n_nodes, T, n_tiles, intra,
                     inter_or_null);
  MATCHA_CHECK_LAUNCH("cluster_adj_finish_kernel");
  return MATCHA_OK;
}

extern "C" size_t matcha_block_colmax_workspace_bytes(int32_t n_nodes, int32_t n_ranges) {
  if (n_nodes < 1 || n_ranges < 1) return 0;
  return align_up((size_t)n_nodes * (size_t)n_ranges * sizeof(double), 256);
}

extern "C" int matcha_block_colmax_normalise(double* A, int32_t n_nodes, const int64_t* ranges, int32_t n_ranges, void* ws, size_t ws_bytes,
                                             matcha_stream_t stream) {
  MATCHA_CHECK_ARG(n_nodes >= 1, "matcha_block_colmax_normalise: n_nodes=%d must be >= 1", n_nodes);
  MATCHA_CHECK_ARG(n_ranges >= 0 && n_ranges <= (1 << 20), "matcha_block_colmax_normalise: n_ranges=%d out of range", n_ranges);
  if (n_ranges == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(A && ranges && ws, "matcha_block_colmax_normalise: null pointer (A, ranges or ws)");
  MATCHA_CHECK_ARG(((uintptr_t)ws) % 8 == 0, "matcha_block_colmax_normalise: ws must be 8-byte aligned");
  const size_t need = matcha_block_colmax_workspace_bytes(n_nodes, n_ranges);
  MATCHA_CHECK_ARG(ws_bytes >= need, "matcha_block_colmax_normalise: workspace too small (%zu bytes, matcha_block_colmax_workspace_bytes says %zu)", ws_bytes,
                   need);
  const int64_t items = (int64_t)n_ranges * cdiv(n_nodes, kBlock);
  const int64_t blocks = items > kMaxBlocks ? kMaxBlocks : items;
  hipLaunchKernelGGL(block_colmax_normalise_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, A, n_nodes, ranges, n_ranges, (double*)ws);
  MATCHA_CHECK_LAUNCH("block_colmax_normalise_kernel");
  return MATCHA_OK;
}
