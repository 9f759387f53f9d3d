// The bookkeeping of one training step of the reference's epoch loop (main.py:155-188) as two launches, so that an epoch can replay ONE
// captured step with everything that changes from step to step living in device memory:
//   matcha_step_select   before the step: this step's positives out of the epoch's shuffled list (main.py:160-161: the slice
//                        [i * batch, (i + 1) * batch) of edges / edge_weight), their weights, the step's reconstruction chromosome;
//                        the counter-RNG seeds of the sampler and of the dropout masks + 1
//   matcha_step_record   after the step: sigmoid of the logits into the epoch's prediction buffer (main.py:58, :185-186), the size of
//                        every hyperedge (main.py:449-451), the running sums of the two losses (main.py:187-188), step counter + 1
//   matcha_step_record_pairs   the same for the regression objective (main.py:94-117): the step's rows as random pairs, one record per pair
// As torch ops this was fourteen tiny kernels per step (a fifth of the launches of a 384-row step); the arithmetic is index copies, a
// popcount per row and expf.
#include "kernels.hpp"

namespace matcha {

__global__ __launch_bounds__(256) void step_select_kernel(const int64_t* __restrict__ pos, const float* __restrict__ w, int64_t n_rows, int L,
                                                          const int64_t* __restrict__ it, int P, int64_t* __restrict__ x,
                                                          float* __restrict__ ww, const int32_t* __restrict__ chroms, int64_t n_chroms,
                                                          int32_t* __restrict__ cell, uint64_t* __restrict__ seed0, uint64_t* __restrict__ seed1) {
  const int64_t step = *it;
  const int i = blockIdx.x * 256 + threadIdx.x;             // one thread per (row, slot)
  if (i == 0) {
    if (cell) cell[0] = chroms[step < n_chroms ? step : n_chroms - 1];
    if (seed0) seed0[0] += 1;                               // the sampler's and the trainer's counter-RNG seeds: new draws every step
    if (seed1) seed1[0] += 1;
  }
  if (i >= P * L) return;
  const int row = i / L, l = i - row * L;
  const int64_t src = (step * P + row) % n_rows;            // (past the end of the list the selection wraps around: never out of bounds)
  x[(int64_t)row * L + l] = pos[src * L + l];
  if (l == 0) ww[row] = w[src];
}

// one workgroup (the driver's batch is 384 rows; a larger B just loops): every thread reads the counter, a barrier, then thread 0 advances it
__global__ __launch_bounds__(1024) void step_record_kernel(const float* __restrict__ logits, const float* __restrict__ losses,
                                                           const int64_t* __restrict__ x, int B, int L, int64_t* __restrict__ it,
                                                           int64_t n_steps, float* __restrict__ sums, float* __restrict__ preds,
                                                           int64_t* __restrict__ sizes) {
  int64_t step = *it;
  __syncthreads();                                          // every thread holds the counter before thread 0 advances it
  if (threadIdx.x == 0) {
    it[0] = step + 1;
    sums[0] += losses[0];
    sums[1] += losses[1];
  }
  if (step >= n_steps) step = n_steps - 1;                  // (a replay past the epoch's end overwrites the last row: never out of bounds)
  for (int b = threadIdx.x; b < B; b += 1024) {
    const float z = logits[b];
    preds[step * B + b] = 1.0f / (1.0f + expf(-z));         // torch.sigmoid's expression (main.py:58)
    int k = 0;
    for (int l = 0; l < L; ++l) k += x[(int64_t)b * L + l] != 0 ? 1 : 0;
    sizes[step * B + b] = k;
  }
}

// ---- the regression objective's pairs (main.py:94-117): a random perfect matching of the step's rows, fresh every step ----------------
// pi = a balanced Feistel network on [0, 2^m) (m even, 2^m >= B) walked in cycles until it lands in [0, B): a bijection of [0, B) keyed
// by (seed, step) with no sort and no table.  tests/test_cpu_regress.py restates the same arithmetic in numpy.
__device__ __forceinline__ uint64_t pair_mix(uint64_t v) {            // murmur3's 64-bit finaliser
  v ^= v >> 33; v *= 0xff51afd7ed558ccdull;
  v ^= v >> 33; v *= 0xc4ceb9fe1a85ec53ull;
  v ^= v >> 33;
  return v;
}
__device__ __forceinline__ uint32_t pair_perm(uint32_t i, uint64_t key, int hb, uint32_t n) {
  const uint32_t mask = (1u << hb) - 1u;
  uint32_t v = i;
  do {
    uint32_t lo = v >> hb, hi = v & mask;
    for (int r = 0; r < 6; ++r) {
      const uint32_t f = (uint32_t)pair_mix(key ^ ((uint64_t)r << 32) ^ hi) & mask;
      const uint32_t t = lo ^ f;
      lo = hi; hi = t;
    }
    v = (lo << hb) | hi;
  } while (v >= n);
  return v;
}
__device__ __forceinline__ float softplus_t(float z) { return z > 20.f ? z : log1pf(expf(z)); }   // torch's F.softplus (threshold 20)

// one thread per pair.  A single workgroup (the driver's steps: up to 2 048 rows) also advances the counter and the sums, behind a barrier
// that every thread has read the counter before; a larger batch runs on a grid, and step_advance_kernel, enqueued behind it, advances them
// (blocks of one grid cannot wait for each other's read of the counter).
__global__ __launch_bounds__(1024) void step_record_pairs_kernel(const float* __restrict__ logits, const float* __restrict__ losses,
                                                                 const float* __restrict__ y, const int64_t* __restrict__ x, int B, int L,
                                                                 int hb, int64_t* __restrict__ it, int64_t n_steps,
                                                                 const uint64_t* __restrict__ seed, float* __restrict__ sums,
                                                                 float* __restrict__ preds, int32_t* __restrict__ labels,
                                                                 int64_t* __restrict__ sizes) {
  int64_t step = *it;
  const uint64_t key = pair_mix(seed[0] ^ pair_mix((uint64_t)step + 0x9E3779B97F4A7C15ull));
  if (gridDim.x == 1) {
    __syncthreads();                                        // every thread holds the counter before thread 0 advances it
    if (threadIdx.x == 0) {
      it[0] = step + 1;
      sums[0] += losses[0];
      sums[1] += losses[1];
    }
  }
  if (step >= n_steps) step = n_steps - 1;                  // (a replay past the epoch's end overwrites the last row: never out of bounds)
  const int H = B / 2;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < H; j += gridDim.x * blockDim.x) {
    const uint32_t r0 = pair_perm(2u * j, key, hb, (uint32_t)B), r1 = pair_perm(2u * j + 1u, key, hb, (uint32_t)B);
    const float y0 = y[r0], y1 = y[r1];
    const float dz = softplus_t(logits[r0]) - softplus_t(logits[r1]);
    preds[step * H + j] = 1.0f / (1.0f + expf(-dz));
    labels[step * H + j] = y0 == y1 ? -1 : (y1 < y0 ? 1 : 0);
    int k = 0;
    for (int l = 0; l < L; ++l) k += x[(int64_t)r0 * L + l] != 0 ? 1 : 0;
    sizes[step * H + j] = k;
  }
}

__global__ void step_advance_kernel(const float* __restrict__ losses, int64_t* __restrict__ it, float* __restrict__ sums) {
  if (threadIdx.x == 0) {
    it[0] += 1;
    sums[0] += losses[0];
    sums[1] += losses[1];
  }
}

}  // namespace matcha

using namespace matcha;

extern "C" int matcha_step_record_pairs(const float* logits, const float* losses, const float* y, const int64_t* x, int64_t B, int32_t L,
                                        int64_t* it, int64_t n_steps, const uint64_t* seed, float* sums, float* preds, int32_t* labels,
                                        int64_t* sizes, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(logits && losses && y && x && it && seed && sums && preds && labels && sizes && B >= 2 && B <= (int64_t)1 << 30 &&
                       n_steps >= 1 && L >= 1 && L <= MATCHA_MAX_L,
                   "matcha_step_record_pairs: bad argument");
  int m = 2;                                                // even bit count of the Feistel domain, 2^m >= B
  while (((int64_t)1 << m) < B) m += 2;
  hipStream_t st = (hipStream_t)stream;
  const int64_t H = B / 2;
  const unsigned grid = H <= 1024 ? 1u : (unsigned)cdiv(H, 256);
  hipLaunchKernelGGL(step_record_pairs_kernel, dim3(grid), dim3(grid == 1 ? 1024 : 256), 0, st, logits, losses, y, x, (int)B, (int)L, m / 2, it,
                     n_steps, seed, sums, preds, labels, sizes);
  MATCHA_CHECK_LAUNCH("step_record_pairs_kernel");
  if (grid > 1) {
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(64), 0, st, losses, it, sums);
    MATCHA_CHECK_LAUNCH("step_advance_kernel");
  }
  return MATCHA_OK;
}

extern "C" int matcha_step_select(const int64_t* pos, const float* w, int64_t n_rows, int32_t L, const int64_t* it, int32_t P, int64_t* x,
                                  float* ww, const int32_t* chroms, int64_t n_chroms, int32_t* cell, uint64_t* seed0, uint64_t* seed1,
                                  matcha_stream_t stream) {
  MATCHA_CHECK_ARG(pos && w && it && x && ww && n_rows > 0 && L >= 1 && L <= MATCHA_MAX_L && P >= 1, "matcha_step_select: bad argument");
  MATCHA_CHECK_ARG(!cell || (chroms && n_chroms > 0), "matcha_step_select: cell without chroms");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(step_select_kernel, dim3((unsigned)cdiv((int64_t)P * L, 256)), dim3(256), 0, st, pos, w, n_rows, (int)L, it, (int)P, x, ww, chroms,
                     n_chroms, cell, seed0, seed1);
  MATCHA_CHECK_LAUNCH("step_select_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_step_record(const float* logits, const float* losses, const int64_t* x, int64_t B, int32_t L, int64_t* it, int64_t n_steps,
                                  float* sums, float* preds, int64_t* sizes, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(logits && losses && x && it && sums && preds && sizes && B >= 1 && n_steps >= 1 && L >= 1 && L <= MATCHA_MAX_L,
                   "matcha_step_record: bad argument");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(step_record_kernel, dim3(1), dim3(1024), 0, st, logits, losses, x, (int)B, (int)L, it, n_steps, sums, preds, sizes);
  MATCHA_CHECK_LAUNCH("step_record_kernel");
  return MATCHA_OK;
}
