// k-way pair maps: the scores of k-way rows projected onto pairs of bins, accumulated on the device.
//
// A map covers a row region R = [lo_r, lo_r + n_r) and a column region C = [lo_c, lo_c + n_c) of node ids: R == C (symmetric) or
// R and C disjoint (rectangular).  An accepted row (skip[i] == 0 and 0 <= value[i] <= vmax; -0.0 counts as 0, NaN / negative / too
// large values are counted in n_rejected) contributes its value once for every pair of positions ci < cj whose ids a = x[ci],
// b = x[cj] are both non-zero, differ and address a cell: rectangular (a - lo_r, b - lo_c) if a in R and b in C, else
// (b - lo_r, a - lo_c) if b in R and a in C; symmetric (min - lo, max - lo) -- only the upper triangle is ever written, the read
// mirrors it.  Planes, chosen by a bit mask: SUM int64 of rint(double(v) 2^32) (fixed point: integer adds commute, so the plane does
// not depend on arrival order or on how the stream is cut), COUNT int64, COUNT_GE int64 (v >= threshold, compared in float32), MAX
// (a 32-bit key: 0 = never hit, else the value's bits | 0x80000000, which orders the non-negative floats as unsigned integers).
//
//   pairmap_init_kernel    zeroes the header (the two counters) and every plane (no memset).
//   pairmap_update_kernel  one thread per row, L a template parameter (2 .. 8), so the ids stay in registers and the pair loop unrolls.
//                          Sweep rows arrive in lexicographic order: for every pair that does not involve the last position,
//                          consecutive lanes address the same cell.  Per pair the lanes compare their cell with the lane below, one
//                          ballot gives the heads of the runs of equal cells, and the LAST lane of a run issues the run's atomics.  A
//                          row's contribution (q, 1, v >= threshold) is the same for all its pairs, so ONE inclusive wavefront prefix
//                          sum per row serves every pair: a run's total is prefix[last] - prefix[first - 1] (two-dword q, count and
//                          count_ge packed in one dword).  The maximum is a segmented scan of the key (six steps, bounded by the run's
//                          first lane).  Merging only joins ADJACENT equal cells; rows in any order give the same planes, just more
//                          atomics.  Pairs with the last position hit consecutive cells of one matrix row: 64 lanes x 8 contiguous bytes.
//                          Integer atomics only: atomicAdd on unsigned long long, atomicMax on unsigned.  The counters take one
//                          atomicAdd per wavefront (ballot + popcount, accumulated over the grid-stride loop).
//   pairmap_read_kernel    one plane out (int64 raw, or float32 for MAX with -inf in cells never hit), mirrored with a zero diagonal
//                          for a symmetric map, and the two counters.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "kernels.hpp"

namespace matcha {
namespace {

constexpr int kBlock = 256;
constexpr uint32_t kNoCell = 0xFFFFFFFFu;      // cells are < 2^31
constexpr size_t kHeaderBytes = 256;           // int64 n_rows, int64 n_rejected, padding
constexpr int kPlaneMask = MATCHA_PAIRMAP_SUM | MATCHA_PAIRMAP_COUNT | MATCHA_PAIRMAP_COUNT_GE | MATCHA_PAIRMAP_MAX;

struct PairmapPlan {
  size_t off_sum, off_count, off_ge, off_max, total;      // an absent plane has offset 0
  int64_t cells;
  int symmetric;
};

bool pairmap_args_ok(int64_t lo_r, int32_t n_r, int64_t lo_c, int32_t n_c, int32_t planes, float vmax) {
  const int64_t lim = (int64_t)1 << 62;
  if (!(n_r >= 1 && n_c >= 1 && lo_r >= 0 && lo_c >= 0 && lo_r <= lim && lo_c <= lim)) return false;
  if ((int64_t)n_r * n_c > INT32_MAX) return false;
  if (planes < 1 || (planes & ~kPlaneMask)) return false;
  if (!(vmax > 0.f && vmax <= 1048576.f)) return false;                 // NaN fails both
  const bool same = lo_r == lo_c && n_r == n_c;
  const bool disjoint = lo_r + n_r <= lo_c || lo_c + n_c <= lo_r;
  return same || disjoint;
}

PairmapPlan make_pplan(int64_t lo_r, int32_t n_r, int64_t lo_c, int32_t n_c, int32_t planes) {
  PairmapPlan pl{};
  pl.cells = (int64_t)n_r * n_c;
  pl.symmetric = lo_r == lo_c && n_r == n_c;
  size_t off = kHeaderBytes;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  if (planes & MATCHA_PAIRMAP_SUM) pl.off_sum = take((size_t)pl.cells * 8);
  if (planes & MATCHA_PAIRMAP_COUNT) pl.off_count = take((size_t)pl.cells * 8);
  if (planes & MATCHA_PAIRMAP_COUNT_GE) pl.off_ge = take((size_t)pl.cells * 8);
  if (planes & MATCHA_PAIRMAP_MAX) pl.off_max = take((size_t)pl.cells * 4);
  pl.total = off;
  return pl;
}

struct PairmapView {
  unsigned long long* counters;                // {n_rows, n_rejected}
  unsigned long long *sum, *count, *ge;        // null = plane absent
  unsigned int* max;
};

PairmapView view_at(void* state, const PairmapPlan& pl) {
  char* w = (char*)state;
  PairmapView v;
  v.counters = (unsigned long long*)w;
  v.sum = pl.off_sum ? (unsigned long long*)(w + pl.off_sum) : nullptr;
  v.count = pl.off_count ? (unsigned long long*)(w + pl.off_count) : nullptr;
  v.ge = pl.off_ge ? (unsigned long long*)(w + pl.off_ge) : nullptr;
  v.max = pl.off_max ? (unsigned int*)(w + pl.off_max) : nullptr;
  return v;
}

__global__ __launch_bounds__(kBlock) void pairmap_init_kernel(unsigned long long* __restrict__ p, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n8; i += (int64_t)gridDim.x * kBlock) p[i] = 0ull;
}

struct PairmapRegion {
  uint64_t lo_r, lo_c;
  uint32_t n_r, n_c;
  int symmetric;
};

// the cell a pair of ids addresses, kNoCell for none (unsigned differences: an id below the region wraps past every n)
__device__ __forceinline__ uint32_t cell_of(const PairmapRegion& g, int64_t a, int64_t b) {
  if (a == 0 || b == 0 || a == b) return kNoCell;
  if (g.symmetric) {
    const uint64_t ra = (uint64_t)a - g.lo_r, rb = (uint64_t)b - g.lo_r;
    if (ra >= g.n_r || rb >= g.n_r) return kNoCell;
    const uint32_t lo = (uint32_t)(ra < rb ? ra : rb), hi = (uint32_t)(ra < rb ? rb : ra);
    return lo * g.n_c + hi;
  }
  const uint64_t ar = (uint64_t)a - g.lo_r, bc = (uint64_t)b - g.lo_c;
  if (ar < g.n_r && bc < g.n_c) return (uint32_t)ar * g.n_c + (uint32_t)bc;
  const uint64_t br = (uint64_t)b - g.lo_r, ac = (uint64_t)a - g.lo_c;
  if (br < g.n_r && ac < g.n_c) return (uint32_t)br * g.n_c + (uint32_t)ac;
  return kNoCell;
}

// Every lane of a wavefront runs the whole body (lanes past n carry an empty row): the shuffles and ballots below read all 64 lanes.
template <int L>
__global__ __launch_bounds__(kBlock) void pairmap_update_kernel(PairmapView pv, PairmapRegion g, float vmax, float threshold, const int64_t* __restrict__ x,
                                                                const float* __restrict__ value, const int32_t* __restrict__ skip, int64_t n) {
  const int lane = threadIdx.x & (kWave - 1);
  uint32_t n_rows = 0, n_rej = 0;                                        // this wavefront's totals (identical in every lane)
  for (int64_t base = (int64_t)blockIdx.x * kBlock; base < n; base += (int64_t)gridDim.x * kBlock) {
    const int64_t i = base + threadIdx.x;
    int64_t id[L];
    float v = 0.f;
    bool live = false, rejected = false;
    if (i < n) {
      const bool skipped = skip && skip[i] != 0;
      v = value[i];
      const bool ok = v >= 0.f && v <= vmax;                             // false for NaN
      live = !skipped && ok;
      rejected = !skipped && !ok;
#pragma unroll
      for (int c = 0; c < L; ++c) id[c] = x[i * L + c];
    } else {
#pragma unroll
      for (int c = 0; c < L; ++c) id[c] = 0;
    }
    const uint64_t live_mask = __ballot(live);
    n_rows += (uint32_t)__popcll(live_mask);
    n_rej += (uint32_t)__popcll(__ballot(rejected));
    if (live_mask == 0) continue;                                        // uniform within the wavefront
    v = live ? v + 0.f : 0.f;                                            // -0.0 -> +0.0
    // inclusive prefix over the lanes of (q, count | count_ge << 16): at most 64 rows, q <= 2^52
    unsigned long long pq = live ? (unsigned long long)__double2ll_rn((double)v * 4294967296.0) : 0ull;
    uint32_t pc = live ? (1u | (v >= threshold ? 0x10000u : 0u)) : 0u;
    const uint32_t key = live ? (__builtin_bit_cast(uint32_t, v) | 0x80000000u) : 0u;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const unsigned long long tq = __shfl_up(pq, d, kWave);
      const uint32_t tc = __shfl_up(pc, d, kWave);
      if (lane >= d) { pq += tq; pc += tc; }
    }
#pragma unroll
    for (int ci = 0; ci < L - 1; ++ci) {
#pragma unroll
      for (int cj = ci + 1; cj < L; ++cj) {
        const uint32_t cell = live ? cell_of(g, id[ci], id[cj]) : kNoCell;
        if (__ballot(cell != kNoCell) == 0) continue;                    // uniform: padding columns, ids outside the regions
        const uint32_t below = __shfl_up(cell, 1, kWave);
        const bool head = lane == 0 || cell != below || cell == kNoCell;
        const uint64_t heads = __ballot(head);                           // bit 0 is always set
        const int first = 63 - __clzll(heads & (~0ull >> (63 - lane)));  // the head of this lane's run
        const bool last = lane == kWave - 1 || ((heads >> (lane + 1)) & 1ull);
        const int src = first > 0 ? first - 1 : 0;
        unsigned long long rq = __shfl(pq, src, kWave);
        uint32_t rc = __shfl(pc, src, kWave);
        rq = first > 0 ? pq - rq : pq;
        rc = first > 0 ? pc - rc : pc;
        uint32_t mk = key;
        if (pv.max) {
#pragma unroll
          for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t t = __shfl_up(mk, d, kWave);
            if (lane - d >= first) mk = t > mk ? t : mk;
          }
        }
        if (last && cell != kNoCell) {
          if (pv.sum) atomicAdd(pv.sum + cell, rq);
          if (pv.count) atomicAdd(pv.count + cell, (unsigned long long)(rc & 0xFFFFu));
          if (pv.ge && (rc >> 16)) atomicAdd(pv.ge + cell, (unsigned long long)(rc >> 16));
          if (pv.max) atomicMax(pv.max + cell, mk);
        }
      }
    }
  }
  if (lane == 0) {
    if (n_rows) atomicAdd(pv.counters, (unsigned long long)n_rows);
    if (n_rej) atomicAdd(pv.counters + 1, (unsigned long long)n_rej);
  }
}

__global__ __launch_bounds__(kBlock) void pairmap_read_kernel(PairmapView pv, int32_t plane, uint32_t n_c, int symmetric, int64_t cells, void* __restrict__ out,
                                                              int64_t* __restrict__ counters_out) {
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < cells; p += (int64_t)gridDim.x * kBlock) {
    const uint32_t r = (uint32_t)p / n_c, c = (uint32_t)p - r * n_c;
    const bool diag = symmetric && r == c;
    const uint32_t src = symmetric && r > c ? c * n_c + r : (uint32_t)p;
    if (plane == MATCHA_PAIRMAP_MAX) {
      const uint32_t key = pv.max[src];
      ((float*)out)[p] = diag ? 0.f : key ? __builtin_bit_cast(float, key & 0x7FFFFFFFu) : -INFINITY;
    } else {
      const unsigned long long* from = plane == MATCHA_PAIRMAP_SUM ? pv.sum : plane == MATCHA_PAIRMAP_COUNT ? pv.count : pv.ge;
      ((int64_t*)out)[p] = diag ? 0 : (int64_t)from[src];
    }
  }
  if (counters_out && blockIdx.x == 0 && threadIdx.x < 2) counters_out[threadIdx.x] = (int64_t)pv.counters[threadIdx.x];
}

template <int L>
void launch_update(unsigned blocks, hipStream_t st, const PairmapView& pv, const PairmapRegion& g, float vmax, float threshold, const int64_t* x,
                   const float* value, const int32_t* skip, int64_t n) {
  hipLaunchKernelGGL(pairmap_update_kernel<L>, dim3(blocks), dim3(kBlock), 0, st, pv, g, vmax, threshold, x, value, skip, n);
}

}  // namespace
}  // namespace matcha

using namespace matcha;

extern "C" size_t matcha_pairmap_bytes(int64_t lo_r, int32_t n_r, int64_t lo_c, int32_t n_c, int32_t planes, float vmax, float threshold) {
  if (!pairmap_args_ok(lo_r, n_r, lo_c, n_c, planes, vmax)) return 0;
  return make_pplan(lo_r, n_r, lo_c, n_c, planes).total;
}

#define PAIRMAP_COMMON_ARGS(fn)                                                                                                       \
  MATCHA_CHECK_ARG(state, fn ": null state");                                                                                         \
  MATCHA_CHECK_ARG(pairmap_args_ok(lo_r, n_r, lo_c, n_c, planes, vmax),                                                               \
                   fn ": need n_r, n_c >= 1, n_r n_c < 2^31, lo >= 0, equal or disjoint regions, planes in [1, 15], 0 < vmax <= 2^20 " \
                      "(rows [%lld, +%d) cols [%lld, +%d) planes=%d vmax=%g)",                                                        \
                   (long long)lo_r, n_r, (long long)lo_c, n_c, planes, (double)vmax);                                                 \
  MATCHA_CHECK_ARG(((uintptr_t)state) % 8 == 0, fn ": state must be 8-byte aligned");                                                 \
  const PairmapPlan pl = make_pplan(lo_r, n_r, lo_c, n_c, planes);                                                                    \
  MATCHA_CHECK_ARG(bytes >= pl.total, fn ": state too small (%zu bytes, matcha_pairmap_bytes says %zu)", bytes, pl.total)

extern "C" int matcha_pairmap_init(void* state, size_t bytes, int64_t lo_r, int32_t n_r, int64_t lo_c, int32_t n_c, int32_t planes, float vmax,
                                   float threshold, matcha_stream_t stream) {
  PAIRMAP_COMMON_ARGS("matcha_pairmap_init");
  const int64_t n8 = (int64_t)(pl.total / 8);                            // every offset is a multiple of 256
  int64_t blocks = cdiv(n8, kBlock);
  if (blocks > (1 << 14)) blocks = 1 << 14;
  hipLaunchKernelGGL(pairmap_init_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, (unsigned long long*)state, n8);
  MATCHA_CHECK_LAUNCH("pairmap_init_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_pairmap_update(void* state, size_t bytes, int64_t lo_r, int32_t n_r, int64_t lo_c, int32_t n_c, int32_t planes, float vmax,
                                     float threshold, const int64_t* x, const float* value, const int32_t* skip, int64_t n, int32_t L,
                                     matcha_stream_t stream) {
  PAIRMAP_COMMON_ARGS("matcha_pairmap_update");
  MATCHA_CHECK_ARG(L >= 2 && L <= MATCHA_MAX_L, "matcha_pairmap_update: row width L=%d must be in [2, %d]", L, MATCHA_MAX_L);
  MATCHA_CHECK_ARG(n >= 0 && n <= ((int64_t)1 << 40), "matcha_pairmap_update: n=%lld out of range", (long long)n);
  if (n == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(x && value, "matcha_pairmap_update: null x or value");
  const PairmapView pv = view_at(state, pl);
  const PairmapRegion g{(uint64_t)lo_r, (uint64_t)lo_c, (uint32_t)n_r, (uint32_t)n_c, pl.symmetric};
  int64_t nb = cdiv(n, kBlock);
  if (nb > (1 << 14)) nb = 1 << 14;
  const unsigned blocks = (unsigned)nb;
  hipStream_t st = (hipStream_t)stream;
  switch (L) {
    case 2: launch_update<2>(blocks, st, pv, g, vmax, threshold, x, value, skip, n); break;
    case 3: launch_update<3>(blocks, st, pv, g, vmax, threshold, x, value, skip, n); break;
    case 4: launch_update<4>(blocks, st, pv, g, vmax, threshold, x, value, skip, n); break;
    case 5: launch_update<5>(blocks, st, pv, g, vmax, threshold, x, value, skip, n); break;
    case 6: launch_update<6>(blocks, st, pv, g, vmax, threshold, x, value, skip, n); break;
    case 7: launch_update<7>(blocks, st, pv, g, vmax, threshold, x, value, skip, n); break;
    default: launch_update<8>(blocks, st, pv, g, vmax, threshold, x, value, skip, n); break;
  }
  MATCHA_CHECK_LAUNCH("pairmap_update_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_pairmap_read(const void* state, size_t bytes, int64_t lo_r, int32_t n_r, int64_t lo_c, int32_t n_c, int32_t planes, float vmax,
                                   float threshold, int32_t plane, void* out, int64_t* counters_out, matcha_stream_t stream) {
  PAIRMAP_COMMON_ARGS("matcha_pairmap_read");
  MATCHA_CHECK_ARG((plane == MATCHA_PAIRMAP_SUM || plane == MATCHA_PAIRMAP_COUNT || plane == MATCHA_PAIRMAP_COUNT_GE || plane == MATCHA_PAIRMAP_MAX) &&
                       (plane & planes),
                   "matcha_pairmap_read: plane=%d is not one plane of the mask %d", plane, planes);
  MATCHA_CHECK_ARG(out, "matcha_pairmap_read: null output");
  int64_t blocks = cdiv(pl.cells, kBlock);
  if (blocks > (1 << 14)) blocks = 1 << 14;
  hipLaunchKernelGGL(pairmap_read_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, view_at((void*)state, pl), plane, (uint32_t)n_c,
                     pl.symmetric, pl.cells, out, counters_out);
  MATCHA_CHECK_LAUNCH("pairmap_read_kernel");
  return MATCHA_OK;
}
