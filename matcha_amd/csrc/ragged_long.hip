// The ragged plan for LONG rows: x [B, L] with L <= MATCHA_MAX_LONG_L = 32 (ragged.hip keeps a row's ids in MATCHA_MAX_L = 8 registers).
//
// It fills the fields of Ragged that the token-level kernels read -- row_off, tok_slot, tok_id, tok_key, tok_pos, count and the shared
// padding token at index Tr, exactly as ragged.hip documents them -- and no tile list (no fused kernel runs on long rows).  Pads may stand
// anywhere in a row; an all-padding row has k = 0 and an empty token range.
//
// A workgroup owns 256 consecutive rows and reads their 256 L ids as ONE contiguous, coalesced range (a thread per row would stride by
// 8 L bytes).  A row's real columns are a 32-bit set: the counting pass builds it with LDS atomics and leaves it in `mask` [B]; the fill
// pass reads it back, so a token's position is row_off[b] + popcount(mask[b] below column l).  Three launches: count, scan of the block
// sums, fill.
#include <string.h>

#include "kernels.hpp"

namespace matcha {

constexpr int kLongRows = 256;               // rows per workgroup of the counting / filling passes

// exclusive scan over the 256 threads of a workgroup (six shuffle steps per wavefront, then the four wave totals)
__device__ __forceinline__ int long_scan_256(int v, int* lds4, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) lds4[wave] = incl;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += lds4[w];
  if (total) *total = lds4[0] + lds4[1] + lds4[2] + lds4[3];
  return base + incl - v;
}

__global__ __launch_bounds__(256) void long_plan_count_kernel(const int64_t* __restrict__ x, int64_t B, int L, uint32_t* __restrict__ mask,
                                                              int32_t* __restrict__ blk_sum) {
  __shared__ uint32_t m[kLongRows];
  __shared__ int lds4[4];
  const int64_t b0 = (int64_t)blockIdx.x * kLongRows;
  const int rows = (int)(B - b0 < kLongRows ? B - b0 : kLongRows);
  m[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = b0 * L;
  const int n = rows * L;
  for (int e = threadIdx.x; e < n; e += 256)
    if (x[base + e] != 0) { const int r = e / L; atomicOr(&m[r], 1u << (e - r * L)); }
  __syncthreads();
  const uint32_t mine = (int)threadIdx.x < rows ? m[threadIdx.x] : 0u;
  if ((int)threadIdx.x < rows) mask[b0 + threadIdx.x] = mine;
  int total;
  (void)long_scan_256(__popc(mine), lds4, &total);
  if (threadIdx.x == 0) blk_sum[blockIdx.x] = total;
}

// exclusive scan of the block sums in place; count = {Tr + 1, Tr, 0 tiles, 0 half tiles}
__global__ __launch_bounds__(1024) void long_plan_scan_kernel(int32_t* __restrict__ blk_sum, int nblk, int32_t* __restrict__ count) {
  __shared__ int wtot[16];
  const int chunk = (nblk + 1023) / 1024;
  const int b0 = threadIdx.x * chunk, b1 = (b0 + chunk < nblk) ? b0 + chunk : nblk;
  int local = 0;
  for (int b = b0; b < b1; ++b) local += blk_sum[b];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  int wbase = 0, total = 0;
#pragma unroll
  for (int w2 = 0; w2 < 16; ++w2) { const int v = wtot[w2]; if (w2 < wave) wbase += v; total += v; }
  if (threadIdx.x == 0) { count[0] = total + 1; count[1] = total; count[2] = 0; count[3] = 0; }
  int run = wbase + incl - local;
  for (int b = b0; b < b1; ++b) { const int v = blk_sum[b]; blk_sum[b] = run; run += v; }
}

__global__ __launch_bounds__(256) void long_plan_fill_kernel(const int64_t* __restrict__ x, int64_t B, int L, const uint32_t* __restrict__ mask,
                                                             const int32_t* __restrict__ blk_base, const int32_t* __restrict__ count,
                                                             int32_t* __restrict__ row_off, int32_t* __restrict__ tok_slot, int64_t* __restrict__ tok_id,
                                                             int32_t* __restrict__ tok_pos, int32_t* __restrict__ tok_key, int64_t n_nodes,
                                                             int32_t* __restrict__ status) {
  __shared__ uint32_t m[kLongRows];
  __shared__ int first[kLongRows];
  __shared__ int lds4[4];
  const int64_t b0 = (int64_t)blockIdx.x * kLongRows;
  const int rows = (int)(B - b0 < kLongRows ? B - b0 : kLongRows);
  const uint32_t mine = (int)threadIdx.x < rows ? mask[b0 + threadIdx.x] : 0u;
  const int pos = blk_base[blockIdx.x] + long_scan_256(__popc(mine), lds4, nullptr);
  m[threadIdx.x] = mine;
  first[threadIdx.x] = pos;
  if ((int)threadIdx.x < rows) row_off[b0 + threadIdx.x] = pos;
  __syncthreads();
  const int64_t base = b0 * L;
  const int n = rows * L;
  for (int e = threadIdx.x; e < n; e += 256) {
    int64_t id = x[base + e];
    if (id == 0) continue;
    const int r = e / L, l = e - r * L;
    const uint32_t mk = m[r];
    if (((mk >> l) & 1u) == 0) continue;               // (x changed between the two passes: keep to the counted columns, stay in bounds)
    const int nth = __popc(mk & ((1u << l) - 1u));
    const int p = first[r] + nth;
    if (id < 0 || id > n_nodes) {                      // the reference raises IndexError here (nn.Embedding, Modules.py:34)
      if (status) atomicOr(status, MATCHA_STATUS_BAD_ID);
      id = 0;
    }
    tok_slot[p] = (int32_t)(base + e); tok_id[p] = id; tok_key[p] = (int32_t)id; tok_pos[p] = nth | (__popc(mk) << 8);
  }
  const int tr = count[1];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    row_off[B] = tr;
    tok_slot[tr] = (int32_t)(B * L);
    tok_id[tr] = 0;
    tok_pos[tr] = 0;
  }
  // tok_key of every slot behind the real tokens is 0 (the padding token's included), as in ragged.hip
  for (int64_t i = tr + (int64_t)blockIdx.x * 256 + threadIdx.x; i < B * L + 1; i += (int64_t)gridDim.x * 256) tok_key[i] = 0;
}

size_t long_plan_bytes(int64_t B, int L) {
  const int64_t T = B * L;
  size_t n = 0;
  n += align_up((size_t)(B + 1) * 4, 256);                      // row_off
  n += align_up((size_t)(T + 1) * 4, 256);                      // tok_slot
  n += align_up((size_t)(T + 1) * 8, 256);                      // tok_id
  n += 256;                                                     // count
  n += align_up((size_t)cdiv(B, kLongRows) * 4, 256);           // blk_sum
  n += align_up((size_t)(T + 1) * 4, 256);                      // tok_pos
  n += align_up((size_t)(T + 1) * 4, 256);                      // tok_key
  n += align_up((size_t)B * 4, 256);                            // mask
  return n;
}

void long_plan_carve(int64_t B, int L, char* base, Ragged& r, uint32_t** mask) {
  const int64_t T = B * L;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base + off; off += align_up(bytes, 256); return p; };
  memset(&r, 0, sizeof(r));
  r.row_off = (int32_t*)take((size_t)(B + 1) * 4);
  r.tok_slot = (int32_t*)take((size_t)(T + 1) * 4);
  r.tok_id = (int64_t*)take((size_t)(T + 1) * 8);
  r.count = (int32_t*)take(256);
  r.nblk = (int)cdiv(B, kLongRows);
  r.blk_sum = (int32_t*)take((size_t)r.nblk * 4);
  r.tok_pos = (int32_t*)take((size_t)(T + 1) * 4);
  r.tok_key = (int32_t*)take((size_t)(T + 1) * 4);
  *mask = (uint32_t*)take((size_t)B * 4);
}

int launch_long_plan(const int64_t* x, int64_t B, int L, int64_t n_nodes, int32_t* status, const Ragged& r, uint32_t* mask, hipStream_t st) {
  hipLaunchKernelGGL(long_plan_count_kernel, dim3(r.nblk), dim3(256), 0, st, x, B, L, mask, r.blk_sum);
  MATCHA_CHECK_LAUNCH("long_plan_count_kernel");
  hipLaunchKernelGGL(long_plan_scan_kernel, dim3(1), dim3(1024), 0, st, r.blk_sum, r.nblk, r.count);
  MATCHA_CHECK_LAUNCH("long_plan_scan_kernel");
  hipLaunchKernelGGL(long_plan_fill_kernel, dim3(r.nblk), dim3(256), 0, st, x, B, L, mask, r.blk_sum, r.count, r.row_off, r.tok_slot, r.tok_id, r.tok_pos,
                     r.tok_key, n_nodes, status);
  MATCHA_CHECK_LAUNCH("long_plan_fill_kernel");
  return MATCHA_OK;
}

}  // namespace matcha
