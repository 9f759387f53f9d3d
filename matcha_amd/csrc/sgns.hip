// Skip-gram with negative sampling over a walk corpus (word2vec's published algorithm; the reference calls gensim's
// Word2Vec(walks, size=d, window=10, min_count=0, sg=1, iter=1), History_version/Code/main_SPRITE.py:637-765).
//
// One WAVEFRONT per corpus position (walk w, index i), lane = column: d = 64 C, lane l holds columns l, 64 + l, ...  A dot product is C
// multiply-adds per lane and one 64-lane butterfly; a row update is C atomic instructions that each cover one contiguous 256-byte segment
// of a row, the shape at which global float atomics run at their chip-wide rate (one lane per row is an order of magnitude slower).
// All positions of a launch run concurrently and meet in the tables through float atomics (word2vec's own threads update without locks
// too): the result depends on arrival order in its last bits and is not reproducible from run to run.
//
// Position (w, i), global position g = g_base + w Lw + i, random stream kStreamSgns with hi = g:
//   lr = max(lr1, lr0 - (lr0 - lr1) g / g_total) (in double, rounded to float);  b = window - rand(g, 0) % window;  u = syn1[walk[i]]
//   for every j in [i - b, i + b], j != i, inside the walk, ascending, jj = j - (i - window):
//     v = syn0[walk[j]], neu = 0
//     target u (label 1), then `negative` draws k: id = the inverse-CDF draw of rand64(g, 1 + 2 (jj negative + k)) over the noise table, label 0,
//     skipped when it equals walk[i]:   g_t = (label - sigmoid(v . t)) lr;  neu += g_t t;  t += g_t v  (a negative's row: one atomic add)
//     syn0[walk[j]] += neu (atomic)
//   syn1[walk[i]] += u_final - u_initial (atomic)
#include "kernels.hpp"

namespace matcha {

constexpr int kSgnsMaxNegative = 32, kSgnsMaxWindow = 1024;

template <int C>
__global__ __launch_bounds__(256) void sgns_kernel(const int32_t* __restrict__ walks, int64_t w0, int64_t w1, int Lw, int n_nodes,
                                                   float* __restrict__ syn0, float* __restrict__ syn1,
                                                   const uint64_t* __restrict__ noise_cum, int window, int negative, double lr0, double lr1,
                                                   int64_t g_base, int64_t g_total, const uint64_t* __restrict__ seed,
                                                   int32_t* __restrict__ status) {
  constexpr int D = 64 * C;
  const int lane = (int)threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
  const int64_t p = (int64_t)blockIdx.x * (256 / kWave) + wave;            // wave-uniform
  if (p >= (w1 - w0) * (int64_t)Lw) return;
  const int64_t w = w0 + p / Lw;
  const int i = (int)(p % Lw);
  const int32_t* __restrict__ walk = walks + w * (int64_t)Lw;
  const int center = walk[i];
  if (center < 1 || center > n_nodes) {                 // not a node: the position trains nothing and the call is flagged
    if (lane == 0 && status) atomicOr(status, MATCHA_STATUS_BAD_ID);
    return;
  }
  const int64_t g = g_base + w * (int64_t)Lw + i;
  const double lrd = lr0 - (lr0 - lr1) * (double)g / (double)g_total;
  const float lr = (float)(lrd > lr1 ? lrd : lr1);
  const uint32_t key = rng_key(*seed, kStreamSgns);
  const int b = window - (int)(rng_u32(key, (uint32_t)g, 0u) % (uint32_t)window);
  float u[C], u0[C];
#pragma unroll
  for (int k = 0; k < C; ++k) u0[k] = u[k] = syn1[(int64_t)center * D + k * kWave + lane];
  const int j0 = i - b < 0 ? 0 : i - b, j1 = i + b > Lw - 1 ? Lw - 1 : i + b;
  for (int j = j0; j <= j1; ++j) {
    if (j == i) continue;
    const int ctx = walk[j];
    if (ctx < 1 || ctx > n_nodes) {
      if (lane == 0 && status) atomicOr(status, MATCHA_STATUS_BAD_ID);
      continue;
    }
    // the context's negatives, one draw per lane: their binary searches run side by side
    const int jj = j - (i - window);
    int drawn = 0;
    if (lane < negative) drawn = 1 + (int)cum_draw(noise_cum + 1, n_nodes, rng_u64(key, (uint32_t)g, 1u + 2u * (uint32_t)(jj * negative + lane)));
    float* __restrict__ vrow = syn0 + (int64_t)ctx * D;
    float v[C], neu[C];
#pragma unroll
    for (int k = 0; k < C; ++k) v[k] = vrow[k * kWave + lane];
    {                                                   // the positive: the centre's own output row, kept in registers
      float f = 0.f;
#pragma unroll
      for (int k = 0; k < C; ++k) f = fmaf(v[k], u[k], f);
      f = group_sum<kWave>(f);
      const float gt = (1.f - 1.f / (1.f + expf(-f))) * lr;
#pragma unroll
      for (int k = 0; k < C; ++k) { neu[k] = gt * u[k]; u[k] = fmaf(gt, v[k], u[k]); }
    }
    for (int k2 = 0; k2 < negative; ++k2) {
      const int t_id = __shfl(drawn, k2, kWave);
      if (t_id == center) continue;                     // skipped, not redrawn (word2vec.c)
      float* __restrict__ trow = syn1 + (int64_t)t_id * D;
      float t[C];
#pragma unroll
      for (int k = 0; k < C; ++k) t[k] = trow[k * kWave + lane];
      float f = 0.f;
#pragma unroll
      for (int k = 0; k < C; ++k) f = fmaf(v[k], t[k], f);
      f = group_sum<kWave>(f);
      const float gt = (0.f - 1.f / (1.f + expf(-f))) * lr;
#pragma unroll
      for (int k = 0; k < C; ++k) {
        neu[k] = fmaf(gt, t[k], neu[k]);
        atomicAdd(trow + k * kWave + lane, gt * v[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < C; ++k) atomicAdd(vrow + k * kWave + lane, neu[k]);
  }
#pragma unroll
  for (int k = 0; k < C; ++k) atomicAdd(syn1 + (int64_t)center * D + k * kWave + lane, u[k] - u0[k]);
}

}  // namespace matcha

using namespace matcha;

extern "C" int matcha_sgns_epoch(const int32_t* walks, int64_t n_walks, int32_t walk_length, int64_t w0, int64_t w1, int32_t n_nodes,
                                 int32_t d, float* syn0, float* syn1, const uint64_t* noise_cum, int32_t window, int32_t negative,
                                 double lr0, double lr1, int64_t g_base, int64_t g_total, const uint64_t* seed, int32_t* status,
                                 matcha_stream_t stream) {
  MATCHA_CHECK_ARG(walks && syn0 && syn1 && noise_cum && seed, "matcha_sgns_epoch: null pointer");
  MATCHA_CHECK_ARG(d == 64 || d == 128 || d == 256, "matcha_sgns_epoch: d=%d (64, 128 or 256)", d);
  MATCHA_CHECK_ARG(n_nodes >= 1, "matcha_sgns_epoch: n_nodes=%d", n_nodes);
  MATCHA_CHECK_ARG(walk_length >= 1, "matcha_sgns_epoch: walk_length=%d", walk_length);
  MATCHA_CHECK_ARG(window >= 1 && window <= kSgnsMaxWindow, "matcha_sgns_epoch: window=%d outside 1..%d", window, kSgnsMaxWindow);
  MATCHA_CHECK_ARG(negative >= 0 && negative <= kSgnsMaxNegative, "matcha_sgns_epoch: negative=%d outside 0..%d", negative, kSgnsMaxNegative);
  MATCHA_CHECK_ARG(lr0 >= lr1 && lr1 >= 0.0 && lr0 < 1e30, "matcha_sgns_epoch: learning rates lr0=%g lr1=%g (lr0 >= lr1 >= 0)", lr0, lr1);
  MATCHA_CHECK_ARG(n_walks >= 0 && w0 >= 0 && w1 <= n_walks, "matcha_sgns_epoch: walks [%lld, %lld) outside 0..%lld", (long long)w0, (long long)w1, (long long)n_walks);
  // the global position is the random stream's 32-bit hi counter
  MATCHA_CHECK_ARG(g_total >= 1 && g_total <= (1ll << 32), "matcha_sgns_epoch: g_total=%lld outside 1..2^32", (long long)g_total);
  MATCHA_CHECK_ARG(g_base >= 0 && g_base <= g_total && n_walks <= (g_total - g_base) / walk_length,
                   "matcha_sgns_epoch: g_base=%lld + %lld walks of %d positions pass g_total=%lld", (long long)g_base, (long long)n_walks, walk_length, (long long)g_total);
  if (w1 <= w0) return MATCHA_OK;
  const int64_t positions = (w1 - w0) * (int64_t)walk_length;
  const dim3 grid((unsigned)cdiv(positions, 256 / kWave)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define SGNS_LAUNCH(C_)                                                                                                              \
  hipLaunchKernelGGL(sgns_kernel<C_>, grid, block, 0, st, walks, w0, w1, walk_length, n_nodes, syn0, syn1, noise_cum, window, negative, lr0, \
                     lr1, g_base, g_total, seed, status)
  if (d == 64) SGNS_LAUNCH(1);
  else if (d == 128) SGNS_LAUNCH(2);
  else SGNS_LAUNCH(4);
#undef SGNS_LAUNCH
  MATCHA_CHECK_LAUNCH("sgns_kernel");
  return MATCHA_OK;
}
