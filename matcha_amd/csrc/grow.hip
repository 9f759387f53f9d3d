// ==== cluster growth =================================================================================================
// A beam search that grows hubs of up to 32 loci from seed clusters, one bin of a region per step.  The beam table is int64 [A, B, S]:
// A seeds, B slots per seed (1 <= B <= 64), every slot a cluster row of 7.10 (1 <= S <= 31; the leading non-zero run is the slot, an
// all-zero slot is empty).  Entry e = a B + j; the candidate of (e, r) is 7.10's candidate of cluster e with one free id lo + r, its
// global rank g = e n + r.  The rows, their validity and flag bit 1 are csrc/sweep_rows.hip's kway_complete_rows_kernel, unchanged.  What is
// new is the duplicate rule: the same sorted row is reached from several slots of a seed ({a, b} + c and {a, c} + b).
//
// Twins.  Candidate (a, j, r) is a twin iff a LOWER slot j' < j of the same seed is strictly ascending, non-empty, holds as many ids as
// slot j (which must be strictly ascending too) and slot_j' is a subset of slot_j + {lo + r}: slot_j' \ slot_j is {lo + r}, or empty
// (the two slots are identical: every candidate of slot j is a twin).  Of all candidates of a seed that give the same sorted row
// exactly one is not a twin, the one of the lowest slot (DESIGN.md 7.13 has the proof): no hashing, no atomics.
//
//   grow_twins_kernel       one wavefront per entry, lane i < S holds id i of slot j.  For every lower slot j' (a wave-uniform trip
//                           count) lane i reads id i of slot j' and a constant number of ballots decides the relation: the two zero
//                           masks (sizes), the two descent masks, the mismatch mask d and the two shift tests.  Two strictly ascending
//                           rows u (slot j') and v (slot j) of equal length with |u \ v| = 1 differ in one window [p, q] = [first, last
//                           set bit of d], inside which one row is the other shifted by one: u_i = v_(i-1) on (p, q] and u \ v = {u_p},
//                           or u_i = v_(i+1) on [p, q) and u \ v = {u_q} (p = q: both).  Column j' of row e of twin int64 [A B, B] gets
//                           that id, -1 for identical slots, 0 for no relation; lane j' keeps the column, and the row leaves as one
//                           coalesced store, columns j' >= j zero.  Every shuffle and ballot is executed by all 64 lanes: a lane without
//                           an id, a slot without a relation and a wavefront behind the last entry are predicated, never branched
//                           around.
//   grow_twin_flags_kernel  one thread per rank of [rank0, rank0 + count): ORs 2 into flag[i] when lo + r stands in columns [0, j) of
//                           its entry's twin row, or a -1 does.  Consecutive ranks share the entry: the row is a broadcast read.
// No LDS, no scratch, plain C++ and vector stores.
#include "sweep_rank.hpp"

namespace matcha {
namespace {

constexpr int kGrowBlock = 256;                // 4 wavefronts: 4 entries per block (twins), 256 ranks per block (flags)
constexpr int kMaxBeam = 64;                   // slots per seed: one lane per column of a twin row
constexpr int kMaxSlot = MATCHA_MAX_LONG_L - 1;

__global__ __launch_bounds__(kGrowBlock) void grow_twins_kernel(const int64_t* __restrict__ beam, int64_t entries, int32_t B, int32_t S,
                                                                int64_t* __restrict__ twin) {
  const int lane = threadIdx.x & 63;
  const int64_t per_pass = (int64_t)gridDim.x * (kGrowBlock / 64);
  for (int64_t e0 = (int64_t)blockIdx.x * (kGrowBlock / 64); e0 < entries; e0 += per_pass) {
    const int64_t e = e0 + (threadIdx.x >> 6);                           // the same in all lanes of a wavefront
    const bool live = e < entries;
    const int j = live ? (int)(e % B) : 0;                               // no lower slot behind the last entry: the loop is empty
    const int64_t seed0 = e - j;                                         // entry of the seed's slot 0
    int64_t v = 0;
    if (live && lane < S) v = beam[e * S + lane];
    const uint64_t zv = __ballot(v == 0);                                // lanes >= S hold 0 and S <= 31: bit 31 at the latest is set
    const int s = __builtin_ctzll(zv);
    const int64_t v_prev = shfl64(v, lane ? lane - 1 : 0), v_next = shfl64(v, lane < 63 ? lane + 1 : 63);
    const bool v_ok = s >= 1 && __ballot(lane >= 1 && lane < s && v <= v_prev) == 0;      // non-empty and strictly ascending
    int64_t mine = 0;                                                    // lane c: column c of the twin row
    for (int jp = 0; jp < j; ++jp) {
      int64_t u = 0;
      if (lane < S) u = beam[(seed0 + jp) * S + lane];
      const uint64_t zu = __ballot(u == 0);
      const int su = __builtin_ctzll(zu);
      const int64_t u_prev = shfl64(u, lane ? lane - 1 : 0);
      const bool u_ok = su >= 1 && __ballot(lane >= 1 && lane < su && u <= u_prev) == 0;
      const bool pair = v_ok && u_ok && su == s;
      const uint64_t d = __ballot(lane < s && u != v);
      const int p = __builtin_ctzll(d | (1ull << 63)), q = 63 - __builtin_clzll(d | 1ull);      // defined for d = 0 too (not used then)
      const uint64_t up = __ballot(lane > p && lane <= q && u != v_prev);                        // u is v shifted up on (p, q]?
      const uint64_t down = __ballot(lane >= p && lane < q && u != v_next);                      // ... or shifted down on [p, q)?
      const int64_t x_up = shfl64(u, p), x_down = shfl64(u, q);
      int64_t t = 0;
      if (pair) t = d == 0 ? -1 : up == 0 ? x_up : down == 0 ? x_down : 0;
      if (lane == jp) mine = t;
    }
    if (live && lane < B) twin[e * B + lane] = mine;
  }
}

__global__ __launch_bounds__(kGrowBlock) void grow_twin_flags_kernel(const int64_t* __restrict__ twin, int32_t B, int64_t lo, uint64_t n, int64_t rank0,
                                                                     int64_t count, int32_t* __restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * kGrowBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kGrowBlock) {
    uint64_t e, r;
    split_rank((uint64_t)(rank0 + i), n, e, r);
    const int j = (int)(e % (uint64_t)B);
    const int64_t id = lo + (int64_t)r;
    const int64_t* __restrict__ row = twin + e * (uint64_t)B;
    bool hit = false;
    for (int c = 0; c < j; ++c) {
      const int64_t t = row[c];
      hit |= t != 0 && (t == id || t == -1);
    }
    if (hit) flag[i] |= 2;
  }
}

// A B n, -1 when it does not fit 63 bits
int64_t grow_total(int64_t A, int32_t B, int32_t n) {
  const unsigned __int128 total = (unsigned __int128)(uint64_t)A * (uint64_t)B * (uint64_t)n;
  return total >= ((unsigned __int128)1 << 63) ? -1 : (int64_t)total;
}

}  // namespace
}  // namespace matcha

using namespace matcha;

extern "C" int matcha_grow_twins(const int64_t* beam, int64_t A, int32_t B, int32_t S, int64_t* twin, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(B >= 1 && B <= kMaxBeam, "matcha_grow_twins: B=%d slots per seed must be in [1, %d]", B, kMaxBeam);
  MATCHA_CHECK_ARG(S >= 1 && S <= kMaxSlot, "matcha_grow_twins: S=%d ids per slot must be in [1, %d]", S, kMaxSlot);
  MATCHA_CHECK_ARG(A >= 0 && A <= ((int64_t)1 << 40), "matcha_grow_twins: A=%lld seeds out of range", (long long)A);
  if (A == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(beam, "matcha_grow_twins: null beam");
  MATCHA_CHECK_ARG(twin, "matcha_grow_twins: null output");
  const int64_t entries = A * B;
  int64_t blocks = cdiv(entries, kGrowBlock / 64);
  if (blocks > (1 << 20)) blocks = 1 << 20;
  hipLaunchKernelGGL(grow_twins_kernel, dim3((unsigned)blocks), dim3(kGrowBlock), 0, (hipStream_t)stream, beam, entries, B, S, twin);
  MATCHA_CHECK_LAUNCH("grow_twins_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_grow_twin_flags(const int64_t* twin, int64_t A, int32_t B, int64_t lo, int32_t n, int64_t rank0, int64_t count, int32_t* flag,
                                      matcha_stream_t stream) {
  MATCHA_CHECK_ARG(B >= 1 && B <= kMaxBeam, "matcha_grow_twin_flags: B=%d slots per seed must be in [1, %d]", B, kMaxBeam);
  MATCHA_CHECK_ARG(n >= 1, "matcha_grow_twin_flags: n=%d bins, need n >= 1", n);
  MATCHA_CHECK_ARG(A >= 0, "matcha_grow_twin_flags: A=%lld seeds out of range", (long long)A);
  MATCHA_CHECK_ARG(lo >= 0 && lo <= ((int64_t)1 << 62), "matcha_grow_twin_flags: lo out of range");
  const int64_t total = grow_total(A, B, n);
  MATCHA_CHECK_ARG(total >= 0, "matcha_grow_twin_flags: A B n does not fit 63 bits (A=%lld B=%d n=%d)", (long long)A, B, n);
  MATCHA_ROWS_RANGE("matcha_grow_twin_flags", false, kGrowBlock);
  if (count == 0 || A == 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(twin, "matcha_grow_twin_flags: null twin table");
  MATCHA_CHECK_ARG(flag, "matcha_grow_twin_flags: null flag");
  hipLaunchKernelGGL(grow_twin_flags_kernel, dim3(blocks), dim3(kGrowBlock), 0, (hipStream_t)stream, twin, B, lo, (uint64_t)n, rank0, count, flag);
  MATCHA_CHECK_LAUNCH("grow_twin_flags_kernel");
  return MATCHA_OK;
}
