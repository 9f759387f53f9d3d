// Biased second-order random walks over the hypergraph (the reference's History_version/Code/random_walk_hyper.py).
//
// The reference tabulates one alias table per ordered pair of neighbours (src, dst).  Here a step is a proposal from the FIRST-order
// distribution of the current node -- one inverse-CDF draw over the node's incidence list, whose integer weights sum, per neighbour, to
// f(dst, c) deg(c)^-1/2 -- followed by an acceptance test with the second-order factor alpha(src, dst, c) / alpha_max, decided by two
// membership probes.  Memory is one entry per incidence; every quantity is an integer, so tests/walk_ref.py reproduces a walk bit for bit.
//
// One LANE per walker.  A step is a chain of dependent random loads (the binary search, then up to two probe chains) and a walker cannot
// start step s + 1 before step s is known: there is no parallelism inside a walker worth a second lane, and the latency is hidden by
// the walkers in flight (DESIGN.md 7.17 weighs the alternatives).
#include "kernels.hpp"
#include "set_probe.hpp"

namespace matcha {

// counter of the walk's random stream: hi = the walk's global id, lo = step << 18 | trial << 2 | draw (0, 1: the proposal's 64 bits, 2: acceptance)
constexpr int kWalkMaxLength = 1 << 14, kWalkMaxTrials = 1 << 16;

__global__ __launch_bounds__(256) void hyper_walk_kernel(const int64_t* __restrict__ inc_ptr, const int32_t* __restrict__ inc_nb,
                                                         const uint64_t* __restrict__ inc_cum, int n_nodes,
                                                         const int32_t* __restrict__ pair_set, const int64_t* __restrict__ pair_edges,
                                                         int64_t n_pair, int L_pair, const int32_t* __restrict__ triple_set,
                                                         const int64_t* __restrict__ triple_edges, int64_t n_triple, int L_triple,
                                                         uint64_t t_back, uint64_t t_pair, uint64_t t_far,
                                                         const int32_t* __restrict__ nodes, int64_t n_start, int64_t w0, int64_t w1,
                                                         int walk_length, int max_trials, const uint64_t* __restrict__ seed,
                                                         int32_t* __restrict__ out, int32_t* __restrict__ status) {
  const int64_t w = w0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= w1) return;
  int32_t* row = out + (w - w0) * (int64_t)walk_length;
  int cur = nodes[w % n_start];
  if (cur < 0 || cur > n_nodes) {                       // a start outside the tables: flagged, an all-zero walk
    if (status) atomicOr(status, MATCHA_STATUS_BAD_ID);
    for (int s = 0; s < walk_length; ++s) row[s] = 0;
    return;
  }
  const uint32_t key = rng_key(*seed, kStreamWalk);
  int prev = cur;
  int capped = 0;
  row[0] = cur;
  for (int s = 1; s < walk_length; ++s) {
    const int64_t b = inc_ptr[cur], n = inc_ptr[cur + 1] - b;
    if (n <= 0) { row[s] = cur; continue; }             // a node without a neighbour repeats itself
    int c = cur;
    bool accepted = false;
    for (int t = 0; t < max_trials && !accepted; ++t) {
      const uint32_t ctr = ((uint32_t)s << 18) | ((uint32_t)t << 2);
      c = inc_nb[b + cum_draw(inc_cum + b, n, rng_u64(key, (uint32_t)w, ctr))];
      if (s == 1) { accepted = true; break; }           // the proposal distribution IS the first-order distribution
      uint64_t thr = t_far;
      if (c == prev) {
        thr = t_back;
      } else {
        // sorted (prev, cur, c): three distinct nodes
        const int lo2 = prev < cur ? prev : cur, hi2 = prev < cur ? cur : prev;
        const int64_t x0 = c < lo2 ? c : lo2, x2 = c > hi2 ? c : hi2, x1 = (int64_t)prev + cur + c - x0 - x2;
        if (n_triple > 0 && triple_contains(triple_set, triple_edges, L_triple, x0, x1, x2)) thr = t_back;
        else if (n_pair > 0 && pair_contains(pair_set, pair_edges, L_pair, prev < c ? prev : c, prev < c ? c : prev)) thr = t_pair;
      }
      accepted = (uint64_t)rng_u32(key, (uint32_t)w, ctr | 2u) < thr;
    }
    if (!accepted) ++capped;                            // trials exhausted: the last proposal is kept and the step counted
    row[s] = c;
    prev = cur;
    cur = c;
  }
  if (capped && status) atomicAdd(status + 1, capped);
}

}  // namespace matcha

using namespace matcha;

extern "C" int matcha_hyper_walk(const int64_t* inc_ptr, const int32_t* inc_nb, const uint64_t* inc_cum, int32_t n_nodes,
                                 const void* pair_set, const int64_t* pair_edges, int64_t n_pair_edges, int32_t L_pair,
                                 const void* triple_set, const int64_t* triple_edges, int64_t n_triple_edges, int32_t L_triple,
                                 const int64_t* thresholds, const int32_t* nodes, int64_t n_start, int64_t w0, int64_t w1,
                                 int32_t walk_length, int32_t max_trials, const uint64_t* seed, int32_t* out, int32_t* status,
                                 matcha_stream_t stream) {
  MATCHA_CHECK_ARG(inc_ptr && inc_nb && inc_cum && thresholds && nodes && seed && out, "matcha_hyper_walk: null pointer");
  MATCHA_CHECK_ARG(n_nodes >= 1, "matcha_hyper_walk: n_nodes=%d", n_nodes);
  MATCHA_CHECK_ARG(n_pair_edges == 0 || (pair_set && pair_edges), "matcha_hyper_walk: non-empty pair set without buffers");
  MATCHA_CHECK_ARG(n_triple_edges == 0 || (triple_set && triple_edges), "matcha_hyper_walk: non-empty triple set without buffers");
  MATCHA_CHECK_ARG(n_pair_edges >= 0 && n_pair_edges < (1ll << 31), "matcha_hyper_walk: n_pair_edges=%lld", (long long)n_pair_edges);
  MATCHA_CHECK_ARG(n_triple_edges >= 0 && n_triple_edges < (1ll << 31), "matcha_hyper_walk: n_triple_edges=%lld", (long long)n_triple_edges);
  MATCHA_CHECK_ARG(n_pair_edges == 0 || (L_pair >= 2 && L_pair <= MATCHA_MAX_LONG_L), "matcha_hyper_walk: L_pair=%d (a pair set holds rows of two nodes)", L_pair);
  MATCHA_CHECK_ARG(n_triple_edges == 0 || (L_triple >= 3 && L_triple <= MATCHA_MAX_LONG_L), "matcha_hyper_walk: L_triple=%d (a triple set holds rows of three nodes)", L_triple);
  for (int i = 0; i < 3; ++i)
    MATCHA_CHECK_ARG(thresholds[i] >= 0 && thresholds[i] <= (1ll << 32), "matcha_hyper_walk: thresholds[%d]=%lld outside 0..2^32", i, (long long)thresholds[i]);
  MATCHA_CHECK_ARG(thresholds[0] == (1ll << 32) || thresholds[1] == (1ll << 32) || thresholds[2] == (1ll << 32),
                   "matcha_hyper_walk: no class accepts always (one threshold must be 2^32)");
  MATCHA_CHECK_ARG(n_start >= 1, "matcha_hyper_walk: n_start=%lld", (long long)n_start);
  MATCHA_CHECK_ARG(walk_length >= 1 && walk_length <= kWalkMaxLength, "matcha_hyper_walk: walk_length=%d outside 1..%d", walk_length, kWalkMaxLength);
  MATCHA_CHECK_ARG(max_trials >= 1 && max_trials <= kWalkMaxTrials, "matcha_hyper_walk: max_trials=%d outside 1..%d", max_trials, kWalkMaxTrials);
  // the walk's global id is the random stream's 32-bit hi counter
  MATCHA_CHECK_ARG(w0 >= 0 && w1 <= (1ll << 31) - 1, "matcha_hyper_walk: walk ids [%lld, %lld) outside 0..2^31-1", (long long)w0, (long long)w1);
  if (w1 <= w0) return MATCHA_OK;
  hipLaunchKernelGGL(hyper_walk_kernel, dim3((unsigned)cdiv(w1 - w0, 256)), dim3(256), 0, (hipStream_t)stream, inc_ptr, inc_nb, inc_cum,
                     n_nodes, (const int32_t*)pair_set, pair_edges, n_pair_edges, L_pair, (const int32_t*)triple_set, triple_edges,
                     n_triple_edges, L_triple, (uint64_t)thresholds[0], (uint64_t)thresholds[1], (uint64_t)thresholds[2], nodes, n_start, w0,
                     w1, walk_length, max_trials, seed, out, status);
  MATCHA_CHECK_LAUNCH("hyper_walk_kernel");
  return MATCHA_OK;
}
