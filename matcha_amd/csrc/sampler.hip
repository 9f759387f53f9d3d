// K16: negative sampling (main.py:361-459) on the GPU against an EXACT hash set of the known hyperedges.
//
// The reference keeps one Bloom filter per hyperedge size (utils.py:75-97, pybloom_live) and rejects a
// candidate when `tuple(temp) in filter`.  Here membership is exact: an open-addressing table of int32
// indices into the (immutable) edge list; a probe compares the candidate with the stored row itself.
// A zero-padded ascending row [a,b,c,0,...] identifies (k, tuple) uniquely because node ids are >= 1.
//
// Randomness is the counter RNG of oracle/rng.py, stream STREAM_NEG; negative n = neg_num*j + i of positive j
// draws   mask bits   : rand(key, n, 0xFFFF0000 + attempt)  -> low k bits, redrawn while zero
//                       (each position chosen with prob 1/2, conditioned on >= 1 chosen  ==  the reference's
//                        Binomial(k, 1/2) != 0 count (main.py:371-372) + uniform choice of positions (:389))
//         replacement : rand(key, n, 8*trial + position)     -> start + floor(u * (end - start))    (:405-407)
//                       (rows of more than 8 columns, neg_sample_long_kernel: 32*trial + position)
#include "kernels.hpp"
#include "set_probe.hpp"

namespace matcha {

// The set's layout and its one-lane probes for rows of two and three nodes: set_probe.hpp.
constexpr int kMaxTrials = 1 << 16;

__device__ __forceinline__ uint64_t row_hash(const int64_t* __restrict__ row, int L) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < L; ++i) {
    const uint64_t v = (uint64_t)row[i];
    if (v == 0) break;
    h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 31;
  }
  return h;
}
// rows equal as zero-padded tuples of possibly different widths
__device__ __forceinline__ bool rows_equal(const int64_t* __restrict__ a, int La, const int64_t* __restrict__ b, int Lb) {
  const int L = La > Lb ? La : Lb;
  for (int i = 0; i < L; ++i) {
    const int64_t va = i < La ? a[i] : 0, vb = i < Lb ? b[i] : 0;
    if (va != vb) return false;
    if (va == 0) return true;
  }
  return true;
}

// The same two functions on a row held in REGISTERS (neg_sample_kernel's candidate): every index is a compile-time constant after
// unrolling, so the array never becomes a scratch-memory object (dynamic indices cost 144 B of scratch per lane and 94 scratch
// instructions in the first version); the early exits are flags.
__device__ __forceinline__ uint64_t row_hash_reg(const int64_t (&row)[MATCHA_MAX_L], int L) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
  bool live = true;
#pragma unroll
  for (int i = 0; i < MATCHA_MAX_L; ++i) {
    const uint64_t v = (uint64_t)row[i];
    live = live && i < L && v != 0;
    uint64_t t = h ^ (v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2));
    t *= 0xBF58476D1CE4E5B9ull;
    t ^= t >> 31;
    h = live ? t : h;
  }
  return h;
}
__device__ __forceinline__ bool rows_equal_reg(const int64_t* __restrict__ a, int La, const int64_t (&b)[MATCHA_MAX_L], int Lb) {
  const int L = La > Lb ? La : Lb;
  bool decided = false, equal = true;
#pragma unroll
  for (int i = 0; i < MATCHA_MAX_L; ++i) {
    const int64_t va = (i < La) ? a[i < La ? i : 0] : 0, vb = i < Lb ? b[i] : 0;
    const bool on = !decided && i < L;
    if (on && va != vb) { decided = true; equal = false; }
    if (on && va == vb && va == 0) decided = true;
  }
  return equal;
}
__device__ __forceinline__ bool set_contains_reg(const int32_t* __restrict__ set, const int64_t* __restrict__ edges, int L_set,
                                                 const int64_t (&row)[MATCHA_MAX_L], int L) {
  const int64_t cap = reinterpret_cast<const int64_t*>(set)[0];
  const unsigned long long* slots = reinterpret_cast<const unsigned long long*>(set + kSetHeader);
  const uint64_t h = row_hash_reg(row, L);
  const uint32_t tag = row_tag(h);
  uint64_t pos = h & (uint64_t)(cap - 1);
  for (int64_t probe = 0; probe < cap; probe += kSetWindow) {
    unsigned long long w[kSetWindow];
#pragma unroll
    for (int i = 0; i < kSetWindow; ++i) w[i] = slots[(pos + (uint64_t)i) & (uint64_t)(cap - 1)];      // eight loads in flight: one round trip
    bool open = true;                                    // no empty slot met yet
#pragma unroll
    for (int i = 0; i < kSetWindow; ++i) {
      const int32_t idx = (int32_t)(uint32_t)(w[i] & 0xFFFFFFFFull);
      const uint32_t t = (uint32_t)(w[i] >> 32);
      if (open && idx < 0) open = false;
      if (open && t == tag && rows_equal_reg(edges + (int64_t)idx * L_set, L_set, row, L)) return true;
    }
    if (!open) return false;
    pos = (pos + kSetWindow) & (uint64_t)(cap - 1);
  }
  return false;
}

__global__ void hashset_clear_kernel(int32_t* set, int64_t cap) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { reinterpret_cast<int64_t*>(set)[0] = cap; }
  if (i < cap) reinterpret_cast<unsigned long long*>(set + kSetHeader)[i] = ~0ull;        // idx = -1, tag = all ones
}

__global__ void hashset_insert_kernel(int32_t* set, const int64_t* __restrict__ edges, int64_t n, int L) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t cap = reinterpret_cast<const int64_t*>(set)[0];
  unsigned long long* slots = reinterpret_cast<unsigned long long*>(set + kSetHeader);
  const int64_t* row = edges + i * L;
  const uint64_t h = row_hash(row, L);
  const unsigned long long mine = ((unsigned long long)row_tag(h) << 32) | (unsigned long long)(uint32_t)(int32_t)i;
  uint64_t pos = h & (uint64_t)(cap - 1);
  for (int64_t probe = 0; probe < cap; ++probe) {
    const unsigned long long old = atomicCAS(&slots[pos], ~0ull, mine);
    if (old == ~0ull) return;                                      // inserted
    const int32_t oidx = (int32_t)(uint32_t)(old & 0xFFFFFFFFull);
    if ((uint32_t)(old >> 32) == row_tag(h) && rows_equal(edges + (int64_t)oidx * L, L, row, L)) return;   // duplicate row already present
    pos = (pos + 1) & (uint64_t)(cap - 1);
  }
}

__device__ __forceinline__ bool set_contains(const int32_t* __restrict__ set, const int64_t* __restrict__ edges, int L_set,
                                             const int64_t* row, int L) {
  const int64_t cap = reinterpret_cast<const int64_t*>(set)[0];
  const unsigned long long* slots = reinterpret_cast<const unsigned long long*>(set + kSetHeader);
  const uint64_t h = row_hash(row, L);
  const uint32_t tag = row_tag(h);
  uint64_t pos = h & (uint64_t)(cap - 1);
  for (int64_t probe = 0; probe < cap; ++probe) {
    const unsigned long long w = slots[pos];
    const int32_t idx = (int32_t)(uint32_t)(w & 0xFFFFFFFFull);
    if (idx < 0) return false;
    if ((uint32_t)(w >> 32) == tag && rows_equal(edges + (int64_t)idx * L_set, L_set, row, L)) return true;
    pos = (pos + 1) & (uint64_t)(cap - 1);
  }
  return false;
}

__global__ void hashset_contains_kernel(const int32_t* __restrict__ set, const int64_t* __restrict__ edges, int L_set,
                                        const int64_t* __restrict__ rows, int64_t n, int L, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = set_contains(set, edges, L_set, rows + i * L, L) ? 1 : 0;
}

// one thread per negative
__global__ __launch_bounds__(256) void neg_sample_kernel(const int32_t* __restrict__ set, const int64_t* __restrict__ set_edges,
                                                         int64_t n_set, int L_set, const int64_t* __restrict__ pos, int64_t P,
                                                         int L, int neg_num, int min_dis, const int32_t* __restrict__ node2chrom, int n_nodes,
                                                         const int32_t* __restrict__ chrom_range, int n_chrom,
                                                         const uint64_t* __restrict__ seed, int64_t* __restrict__ neg, int32_t* __restrict__ status) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= P * neg_num) return;
  const int64_t j = n / neg_num;
  int64_t orig[MATCHA_MAX_L], cand[MATCHA_MAX_L];
  int k = 0;
#pragma unroll
  for (int i = 0; i < MATCHA_MAX_L; ++i) {
    orig[i] = (i < L) ? pos[j * L + i] : 0;
    if (orig[i] != 0) k = i + 1;
  }
  int64_t* out = neg + n * L;
  // The chromosome range of EVERY position is looked up before the membership test of the positive, not after it and only for the
  // positions drawn: node -> chromosome -> range is a chain of two dependent loads that then runs next to the hash probe's two
  // instead of behind them (this kernel is a chain of global-memory round trips; at the reference's 288 negatives per step it is
  // nothing else).  Clamped indices, no branch around the loads.
  const uint64_t seed_v = *seed;
  int cidx[MATCHA_MAX_L];
#pragma unroll
  for (int i = 0; i < MATCHA_MAX_L; ++i) {
    const bool in = i < k && orig[i] >= 1 && orig[i] <= n_nodes;
    const int c = node2chrom[in ? orig[i] : 0];
    cidx[i] = (in && c >= 0 && c < n_chrom) ? c : -1;
  }
  int2 crange[MATCHA_MAX_L];
#pragma unroll
  for (int i = 0; i < MATCHA_MAX_L; ++i) crange[i] = reinterpret_cast<const int2*>(chrom_range)[cidx[i] >= 0 ? cidx[i] : 0];
  // `while neighbor_check(temp, dict)` with temp == the positive on entry (main.py:390-392): if the positive is
  // not a member (in particular: empty set, the reference's phase 1, main.py:589) the loop never runs.
  bool resample = (n_set > 0) && (k > 0) && set_contains_reg(set, set_edges, L_set, orig, L);
  bool done = false;
  if (resample) {
    const uint32_t key = rng_key(seed_v, kStreamNeg);
    uint32_t mask = 0;
    for (uint32_t a = 0; mask == 0; ++a) mask = rng_u32(key, (uint32_t)n, 0xFFFF0000u + a) & ((1u << k) - 1u);
    // the chromosome ranges of the positions that may be redrawn do not change between trials
    int64_t cstart[MATCHA_MAX_L], clen[MATCHA_MAX_L];
#pragma unroll
    for (int i = 0; i < MATCHA_MAX_L; ++i) {
      cstart[i] = 0; clen[i] = -1;
      if (i < k && ((mask >> i) & 1u)) {
        // a node outside [1, n_nodes] or without a chromosome (node2chrom = -1, the default fill of train.run) cannot be
        // redrawn: it is kept and the call is flagged (the reference raises KeyError / IndexError at main.py:401-403)
        if (cidx[i] >= 0) {
          cstart[i] = crange[i].x;
          clen[i] = (int64_t)crange[i].y - cstart[i];
        } else if (status) {
          atomicOr(status, MATCHA_STATUS_BAD_CHROM);
        }
      }
    }
    for (int trial = 0; trial < kMaxTrials && !done; ++trial) {
      // unused slots (i >= k) sort behind every node id and are put back to 0 afterwards
      constexpr int64_t kBig = 0x7FFFFFFFFFFFFFFFll;
#pragma unroll
      for (int i = 0; i < MATCHA_MAX_L; ++i) {
        cand[i] = i < k ? orig[i] : kBig;
        if (clen[i] >= 0) {
          const uint32_t r = rng_u32(key, (uint32_t)n, (uint32_t)(8 * trial + i));
          cand[i] = cstart[i] + (int64_t)(((uint64_t)r * (uint64_t)clen[i]) >> 32);
        }
      }
      // sort ascending (k <= 8): Batcher's odd-even merge network, 19 compare-exchanges on registers (an insertion sort indexes the array
      // with run-time values); then reject duplicates / close neighbours / known hyperedges (main.py:410-421, :392)
#define NS_CE(A, B) do { const int64_t lo__ = cand[A] < cand[B] ? cand[A] : cand[B], hi__ = cand[A] < cand[B] ? cand[B] : cand[A]; cand[A] = lo__; cand[B] = hi__; } while (0)
      static_assert(MATCHA_MAX_L == 8, "the sorting network below is for 8 slots");
      NS_CE(0, 1); NS_CE(2, 3); NS_CE(4, 5); NS_CE(6, 7);
      NS_CE(0, 2); NS_CE(1, 3); NS_CE(4, 6); NS_CE(5, 7);
      NS_CE(1, 2); NS_CE(5, 6);
      NS_CE(0, 4); NS_CE(1, 5); NS_CE(2, 6); NS_CE(3, 7);
      NS_CE(2, 4); NS_CE(3, 5);
      NS_CE(1, 2); NS_CE(3, 4); NS_CE(5, 6);
#undef NS_CE
      bool ok = true;
#pragma unroll
      for (int a = 0; a + 1 < MATCHA_MAX_L; ++a) {
        const int64_t gap = cand[a + 1] - cand[a];
        if (a + 1 < k && (gap == 0 || gap <= min_dis)) ok = false;
      }
#pragma unroll
      for (int i = 0; i < MATCHA_MAX_L; ++i) cand[i] = i < k ? cand[i] : 0;
      if (ok && !set_contains_reg(set, set_edges, L_set, cand, L)) done = true;
    }
    // trials exhausted (tiny chromosome, large min_dis, dense known set): the row is returned equal to its positive and counted;
    // the reference would loop forever (main.py:392)
    if (!done && status) atomicAdd(status + 1, 1);
  }
#pragma unroll
  for (int i = 0; i < MATCHA_MAX_L; ++i)
    if (i < L) out[i] = done ? cand[i] : orig[i];
}

// ---- rows of up to MATCHA_MAX_LONG_L = 32 columns: one LANE per position ---------------------------------------------------------------------
// neg_sample_kernel keeps a row in 8 int64 registers per lane and sorts it with an 8-slot network; at 32 slots that is ~200 live VGPRs.  Here a
// GROUP of 32 adjacent lanes owns one negative and lane i holds position i: two negatives per wavefront, eight per 256-thread block.  The row
// is one register pair per lane; sorting, the gap test, the hash chain and the comparison with a stored row are cross-lane exchanges and
// ballots.  No LDS, no scratch.  The table format (hash, tag, slots, linear probing) is the one above: either build serves either sampler.
//
// Every cross-lane operation below is executed by ALL 64 lanes of the wavefront: the two groups of a wavefront run the same wave-uniform
// loops (their conditions are __any over the wavefront) and a group that has nothing left to do is predicated off (`want`, `active`), never
// branched around a shuffle or a ballot.  Only loads, stores and atomics sit inside divergent ifs.
constexpr int kGroup = 32;             // lanes per negative
static_assert(MATCHA_MAX_LONG_L == kGroup && kWave == 2 * kGroup, "one lane per position, two negatives per wavefront");

__device__ __forceinline__ uint32_t group_ballot(bool p, int half) { return (uint32_t)(__ballot(p) >> (kGroup * half)); }
__device__ __forceinline__ int first_bit(uint32_t m) { return m ? __ffs((int)m) - 1 : kGroup; }      // kGroup when no bit is set

// Membership of the group's row (`val` = this lane's id, 0 at and behind the row's end and at lanes >= L) -- row_hash / set_contains above,
// one lane per position.  `want` is group-uniform; a group with want == false loads nothing and gets false.
__device__ __forceinline__ bool group_contains(const int32_t* __restrict__ set, const int64_t* __restrict__ edges, int L_set, int64_t val, int L,
                                               int lane, int half, bool want) {
  const int64_t cap = reinterpret_cast<const int64_t*>(set)[0];
  const unsigned long long* slots = reinterpret_cast<const unsigned long long*>(set + kSetHeader);
  // the hash chain is sequential in the position: every lane runs it on values broadcast from their owners
  uint64_t h = 0x9E3779B97F4A7C15ull;
  bool live = want;
  for (int i = 0; i < L; ++i) {
    if (!__any(live)) break;
    const uint64_t v = (uint64_t)__shfl((long long)val, i, kGroup);
    live = live && v != 0;
    uint64_t t = h ^ (v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2));
    t *= 0xBF58476D1CE4E5B9ull;
    t ^= t >> 31;
    h = live ? t : h;
  }
  const uint32_t tag = row_tag(h);
  uint64_t p = h & (uint64_t)(cap - 1);
  bool found = false, searching = want;
  for (int64_t probe = 0; probe < cap; probe += kGroup) {
    if (!__any(searching)) break;
    // a window of 32 consecutive slots, one per lane: one round trip (cap >= 1024)
    unsigned long long w = ~0ull;
    if (searching) w = slots[(p + (uint64_t)lane) & (uint64_t)(cap - 1)];
    const int32_t idx = (int32_t)(uint32_t)(w & 0xFFFFFFFFull);
    const uint32_t empty = group_ballot(idx < 0, half);
    const int fe = first_bit(empty);
    const uint32_t before = fe >= kGroup ? 0xFFFFFFFFu : ((1u << fe) - 1u);        // the slots in front of the first empty one
    uint32_t m = group_ballot(searching && idx >= 0 && (uint32_t)(w >> 32) == tag, half) & before;
    while (__any(m != 0)) {
      // a tag match: the stored row, one coalesced read, compared position by position (rows_equal: equal up to the first common zero)
      const int32_t ci = __shfl(idx, m ? first_bit(m) : 0, kGroup);
      int64_t sv = 0;
      if (m != 0 && lane < L_set) sv = edges[(int64_t)ci * L_set + lane];
      const int fm = first_bit(group_ballot(sv != val, half)), fz = first_bit(group_ballot(sv == 0 && val == 0, half));
      if (m != 0 && fm >= fz) { found = true; m = 0; }
      m &= m - 1u;
    }
    if (found || empty != 0) searching = false;
    p = (p + (uint64_t)kGroup) & (uint64_t)(cap - 1);
  }
  return found;
}

__global__ __launch_bounds__(256) void neg_sample_long_kernel(const int32_t* __restrict__ set, const int64_t* __restrict__ set_edges,
                                                              int64_t n_set, int L_set, const int64_t* __restrict__ pos, int64_t P,
                                                              int L, int neg_num, int min_dis, const int32_t* __restrict__ node2chrom, int n_nodes,
                                                              const int32_t* __restrict__ chrom_range, int n_chrom,
                                                              const uint64_t* __restrict__ seed, int64_t* __restrict__ neg, int32_t* __restrict__ status) {
  const int lane = (int)threadIdx.x & (kGroup - 1), half = ((int)threadIdx.x / kGroup) & 1;
  const int64_t n = (int64_t)blockIdx.x * (256 / kGroup) + (int64_t)(threadIdx.x / kGroup);
  const bool valid = n < P * neg_num;             // group-uniform; a group behind the end takes part in the exchanges and stores nothing
  const int64_t j = valid ? n / neg_num : 0;
  const int64_t orig = (valid && lane < L) ? pos[j * L + lane] : 0;        // one coalesced row read
  const uint32_t nz = group_ballot(orig != 0, half);
  const int k = nz ? 32 - __clz((int)nz) : 0;                              // index of the last non-zero + 1
  // node -> chromosome -> [start, end) of this lane's own node, once, before the membership test of the positive (clamped indices)
  const bool in = lane < k && orig >= 1 && orig <= n_nodes;
  const int c = node2chrom[in ? orig : 0];
  const int cidx = (in && c >= 0 && c < n_chrom) ? c : -1;
  const int2 crange = reinterpret_cast<const int2*>(chrom_range)[cidx >= 0 ? cidx : 0];
  const uint64_t seed_v = *seed;
  // `while neighbor_check(temp, dict)` with temp == the positive on entry (main.py:390-392): not a member (empty set: phase 1) -> copied
  bool resample = false;
  if (n_set > 0) resample = group_contains(set, set_edges, L_set, orig, L, lane, half, valid && k > 0);       // n_set is kernel-uniform
  int64_t result = orig;
  if (__any(resample)) {
    const uint32_t key = rng_key(seed_v, kStreamNeg);
    const uint32_t kmask = k >= 32 ? 0xFFFFFFFFu : ((1u << k) - 1u);       // k = 32 uses all 32 bits: no shift by 32
    uint32_t mask = 0;
    if (resample)
      for (uint32_t a = 0; mask == 0; ++a) mask = rng_u32(key, (uint32_t)n, 0xFFFF0000u + a) & kmask;
    // a node outside [1, n_nodes] or without a chromosome cannot be redrawn: it is kept and the call is flagged (neg_sample_kernel)
    const bool chosen = resample && lane < k && ((mask >> lane) & 1u);
    const bool redraw = chosen && cidx >= 0;
    if (chosen && cidx < 0 && status) atomicOr(status, MATCHA_STATUS_BAD_CHROM);
    const int64_t cstart = crange.x, clen = (int64_t)crange.y - (int64_t)crange.x;
    const uint32_t stride = L <= MATCHA_MAX_L ? 8u : 32u;                  // L <= 8: the counters of neg_sample_kernel, bit for bit
    constexpr int64_t kBig = 0x7FFFFFFFFFFFFFFFll;                         // unused lanes sort behind every node id
    bool active = resample;
    for (int trial = 0; trial < kMaxTrials; ++trial) {
      if (!__any(active)) break;
      int64_t cand = lane < k ? orig : kBig;
      if (redraw) {
        const uint32_t r = rng_u32(key, (uint32_t)n, stride * (uint32_t)trial + (uint32_t)lane);
        cand = cstart + (int64_t)(((uint64_t)r * (uint64_t)clen) >> 32);
      }
      // bitonic sort over the group's 32 lanes, ascending: 15 compare-exchanges with the lane at distance st
#pragma unroll
      for (int sz = 2; sz <= kGroup; sz <<= 1) {
#pragma unroll
        for (int st = sz >> 1; st > 0; st >>= 1) {
          const int64_t other = (int64_t)__shfl_xor((long long)cand, st, kGroup);
          const bool take_min = ((lane & sz) == 0) == ((lane & st) == 0);
          const int64_t lo = cand < other ? cand : other, hi = cand < other ? other : cand;
          cand = take_min ? lo : hi;
        }
      }
      // duplicates / close neighbours (main.py:410-421): every lane against its left neighbour
      const int64_t gap = cand - (int64_t)__shfl_up((long long)cand, 1, kGroup);
      const bool bad = lane >= 1 && lane < k && (gap == 0 || gap <= min_dis);
      const bool ok = active && group_ballot(bad, half) == 0;
      cand = lane < k ? cand : 0;
      const bool known = group_contains(set, set_edges, L_set, cand, L, lane, half, ok);
      if (ok && !known) { result = cand; active = false; }
    }
    // trials exhausted: the row is returned equal to its positive and counted once (the reference would loop forever, main.py:392)
    if (active && lane == 0 && status) atomicAdd(status + 1, 1);
  }
  if (valid && lane < L) neg[n * L + lane] = result;                       // one coalesced store
}

// ---- planted outliers (matcha_outlier_plant; the reference's generate_outlier_part, History_version/Code/utils.py:184-233) -------------
// (the pair-set probe, pair_contains: set_probe.hpp)
// One group of 32 lanes per output row, lane i = position i, like neg_sample_long_kernel and under its rule for cross-lane operations: every
// shuffle and ballot is executed by all 64 lanes, a group with nothing left to do is predicated off (`active`, `ok`).  Local row i is global
// row n = n0 + i, a copy of positive i / draws (copy n % draws of it where n0 is a multiple of draws).  The plant rule is stated in include/matcha_hip.h.
constexpr int kPlantTrials = 256;
__global__ __launch_bounds__(256) void outlier_plant_kernel(const int32_t* __restrict__ set, const int64_t* __restrict__ set_edges, int64_t n_set,
                                                            int L_set, const int32_t* __restrict__ pair_set, const int64_t* __restrict__ pair_edges,
                                                            int64_t n_pair, int L_pair, const int64_t* __restrict__ pos, int64_t P, int L, int draws,
                                                            int cycle, int min_dis, const int32_t* __restrict__ node2chrom, int n_nodes,
                                                            const int32_t* __restrict__ chrom_range, int n_chrom, const uint64_t* __restrict__ seed,
                                                            int64_t n0, int64_t* __restrict__ out, int32_t* __restrict__ planted,
                                                            int32_t* __restrict__ status) {
  const int lane = (int)threadIdx.x & (kGroup - 1), half = ((int)threadIdx.x / kGroup) & 1;
  const int64_t i = (int64_t)blockIdx.x * (256 / kGroup) + (int64_t)(threadIdx.x / kGroup);
  const bool valid = i < P * draws;               // group-uniform; a group behind the end takes part in the exchanges and stores nothing
  const int64_t n = n0 + i;
  const int64_t orig = (valid && lane < L) ? pos[(i / draws) * L + lane] : 0;          // one coalesced row read
  const int k = first_bit(group_ballot(lane >= L || orig == 0, half));                 // the non-zero prefix (32: no zero in the row)
  const bool in = lane < k && orig >= 1 && orig <= n_nodes;
  const bool bad_id = group_ballot(lane < k && !in, half) != 0;
  const int c = node2chrom[in ? orig : 0];
  const int cidx = (in && c >= 0 && c < n_chrom) ? c : -1;
  const int2 crange = reinterpret_cast<const int2*>(chrom_range)[cidx >= 0 ? cidx : 0];
  const uint32_t key = rng_key(*seed, kStreamOutlier);
  int p = 0;
  if (k >= 2) p = cycle ? (int)((n % draws) % k) : (int)(((uint64_t)rng_u32(key, (uint32_t)n, 0xFFFF0000u) * (uint64_t)k) >> 32);
  // the chromosome of the locus that leaves, from its lane
  const int pc = __shfl(cidx, p, kGroup);
  const int64_t cstart = __shfl(crange.x, p, kGroup), clen = (int64_t)__shfl(crange.y, p, kGroup) - cstart;
  const bool no_chrom = k >= 2 && (pc < 0 || clen <= 0);
  if (valid && lane == 0 && (bad_id || no_chrom) && status) atomicOr(status, MATCHA_STATUS_BAD_CHROM);
  constexpr int64_t kBig = 0x7FFFFFFFFFFFFFFFll;                           // unused lanes sort behind every node id
  int64_t result = orig;
  int plant = -1;
  bool active = valid && k >= 2 && !bad_id && !no_chrom;
  for (int trial = 0; trial < kPlantTrials; ++trial) {
    if (!__any(active)) break;
    const uint32_t r = rng_u32(key, (uint32_t)n, (uint32_t)trial);
    const int64_t j = cstart + (int64_t)(((uint64_t)r * (uint64_t)(active ? clen : 0)) >> 32);
    const bool dup = group_ballot(lane < k && orig == j, half) != 0;       // j is a locus of the positive (the one it replaces included)
    const int rank = __popc(group_ballot(lane < k && lane != p && orig < j, half));      // where j stands in cand
    int64_t cand = lane < k ? (lane == p ? j : orig) : kBig;
    // bitonic sort over the group's 32 lanes, ascending (neg_sample_long_kernel)
#pragma unroll
    for (int sz = 2; sz <= kGroup; sz <<= 1) {
#pragma unroll
      for (int st = sz >> 1; st > 0; st >>= 1) {
        const int64_t other = (int64_t)__shfl_xor((long long)cand, st, kGroup);
        const bool take_min = ((lane & sz) == 0) == ((lane & st) == 0);
        const int64_t lo = cand < other ? cand : other, hi = cand < other ? other : cand;
        cand = take_min ? lo : hi;
      }
    }
    const int64_t gap = cand - (int64_t)__shfl_up((long long)cand, 1, kGroup);
    const bool bad = lane >= 1 && lane < k && (gap == 0 || gap <= min_dis);
    bool ok = active && !dup && group_ballot(bad, half) == 0;
    cand = lane < k ? cand : 0;
    if (n_pair > 0) {                                                      // kernel-uniform: no known pair through the planted bin
      bool hit = false;
      if (ok && lane < k && cand != j) hit = pair_contains(pair_set, pair_edges, L_pair, cand < j ? cand : j, cand < j ? j : cand);
      ok = ok && group_ballot(hit, half) == 0;
    }
    bool known = false;
    if (n_set > 0) known = group_contains(set, set_edges, L_set, cand, L, lane, half, ok);
    if (ok && !known) { result = cand; plant = rank; active = false; }
  }
  // trials exhausted: the row is returned equal to its positive, planted = -1, and counted once
  if (active && lane == 0 && status) atomicAdd(status + 1, 1);
  if (valid && lane < L) out[i * L + lane] = result;                       // one coalesced store
  if (valid && lane == 0) planted[i] = plant;
}

}  // namespace matcha

using namespace matcha;

static int64_t set_capacity(int64_t n_edges) {
  int64_t cap = 1024;
  while (cap < 2 * n_edges) cap <<= 1;
  return cap;
}

extern "C" size_t matcha_hashset_bytes(int64_t n_edges) {
  return (size_t)kSetHeader * sizeof(int32_t) + (size_t)set_capacity(n_edges < 0 ? 0 : n_edges) * sizeof(SetSlot);
}

// The three entry points below exist twice: the short ones (rows of up to MATCHA_MAX_L = 8 columns, neg_sample_kernel) and the `_long` ones (up
// to MATCHA_MAX_LONG_L = 32, neg_sample_long_kernel).  The set kernels loop to a run-time width and serve both; the checks are shared.
static int hashset_build_impl(const char* fn, int max_l, void* set, size_t set_bytes, const int64_t* edges, int64_t n_edges, int32_t L,
                              matcha_stream_t stream) {
  MATCHA_CHECK_ARG(set && (edges || n_edges == 0), "%s: null pointer", fn);
  MATCHA_CHECK_ARG(L >= 1 && L <= max_l, "%s: L=%d", fn, L);
  MATCHA_CHECK_ARG(n_edges >= 0 && n_edges < (1ll << 31), "%s: n_edges=%lld", fn, (long long)n_edges);
  MATCHA_CHECK_ARG(set_bytes >= matcha_hashset_bytes(n_edges), "%s: set buffer too small", fn);
  hipStream_t st = (hipStream_t)stream;
  const int64_t cap = set_capacity(n_edges);
  hipLaunchKernelGGL(hashset_clear_kernel, dim3((unsigned)cdiv(cap, 256)), dim3(256), 0, st, (int32_t*)set, cap);
  MATCHA_CHECK_LAUNCH("hashset_clear_kernel");
  if (n_edges > 0) {
    hipLaunchKernelGGL(hashset_insert_kernel, dim3((unsigned)cdiv(n_edges, 256)), dim3(256), 0, st, (int32_t*)set, edges, n_edges, L);
    MATCHA_CHECK_LAUNCH("hashset_insert_kernel");
  }
  return MATCHA_OK;
}

static int hashset_contains_impl(const char* fn, int max_l, const void* set, const int64_t* edges, int32_t L_set, const int64_t* rows, int64_t n,
                                 int32_t L, int32_t* out, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(set && rows && out, "%s: null pointer", fn);
  MATCHA_CHECK_ARG(L >= 1 && L <= max_l && L_set >= 1 && L_set <= max_l, "%s: bad width", fn);
  if (n <= 0) return MATCHA_OK;
  hipLaunchKernelGGL(hashset_contains_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const int32_t*)set,
                     edges, L_set, rows, n, L, out);
  MATCHA_CHECK_LAUNCH("hashset_contains_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_hashset_build(void* set, size_t set_bytes, const int64_t* edges, int64_t n_edges, int32_t L,
                                    matcha_stream_t stream) {
  return hashset_build_impl("matcha_hashset_build", MATCHA_MAX_L, set, set_bytes, edges, n_edges, L, stream);
}
extern "C" int matcha_hashset_build_long(void* set, size_t set_bytes, const int64_t* edges, int64_t n_edges, int32_t L,
                                         matcha_stream_t stream) {
  return hashset_build_impl("matcha_hashset_build_long", MATCHA_MAX_LONG_L, set, set_bytes, edges, n_edges, L, stream);
}

extern "C" int matcha_hashset_contains(const void* set, const int64_t* edges, int32_t L_set, const int64_t* rows, int64_t n,
                                       int32_t L, int32_t* out, matcha_stream_t stream) {
  return hashset_contains_impl("matcha_hashset_contains", MATCHA_MAX_L, set, edges, L_set, rows, n, L, out, stream);
}
extern "C" int matcha_hashset_contains_long(const void* set, const int64_t* edges, int32_t L_set, const int64_t* rows, int64_t n,
                                            int32_t L, int32_t* out, matcha_stream_t stream) {
  return hashset_contains_impl("matcha_hashset_contains_long", MATCHA_MAX_LONG_L, set, edges, L_set, rows, n, L, out, stream);
}

extern "C" int matcha_neg_sample(const void* set, const int64_t* set_edges, int64_t n_set_edges, int32_t L_set,
                                 const int64_t* pos, int64_t P, int32_t L, int32_t neg_num, int32_t min_dis,
                                 const int32_t* node2chrom, int32_t n_nodes, const int32_t* chrom_range, int32_t n_chrom,
                                 const uint64_t* seed, int64_t* neg, int32_t* status, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(pos && neg && node2chrom && chrom_range && seed, "matcha_neg_sample: null pointer");
  MATCHA_CHECK_ARG(((uintptr_t)chrom_range) % 8 == 0, "matcha_neg_sample: chrom_range must be 8-byte aligned (the kernel reads [lo, hi] pairs as one int2)");
  MATCHA_CHECK_ARG(n_nodes >= 1 && n_chrom >= 1, "matcha_neg_sample: n_nodes=%d n_chrom=%d", n_nodes, n_chrom);
  MATCHA_CHECK_ARG(n_set_edges == 0 || (set && set_edges), "matcha_neg_sample: non-empty set without buffers");
  MATCHA_CHECK_ARG(L >= 1 && L <= MATCHA_MAX_L && neg_num >= 1, "matcha_neg_sample: L=%d neg_num=%d", L, neg_num);
  if (P <= 0) return MATCHA_OK;
  ProfScope ps(MATCHA_PROF_NEG_SAMPLE, (double)P * L * 8.0 * (1.0 + neg_num), (hipStream_t)stream);
  hipLaunchKernelGGL(neg_sample_kernel, dim3((unsigned)cdiv(P * neg_num, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const int32_t*)set, set_edges, n_set_edges, L_set > 0 ? L_set : L, pos, P, L, neg_num, min_dis, node2chrom, n_nodes,
                     chrom_range, n_chrom, seed, neg, status);
  MATCHA_CHECK_LAUNCH("neg_sample_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_neg_sample_long(const void* set, const int64_t* set_edges, int64_t n_set_edges, int32_t L_set,
                                      const int64_t* pos, int64_t P, int32_t L, int32_t neg_num, int32_t min_dis,
                                      const int32_t* node2chrom, int32_t n_nodes, const int32_t* chrom_range, int32_t n_chrom,
                                      const uint64_t* seed, int64_t* neg, int32_t* status, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(pos && neg && node2chrom && chrom_range && seed, "matcha_neg_sample_long: null pointer");
  MATCHA_CHECK_ARG(((uintptr_t)chrom_range) % 8 == 0, "matcha_neg_sample_long: chrom_range must be 8-byte aligned (the kernel reads [lo, hi] pairs as one int2)");
  MATCHA_CHECK_ARG(n_nodes >= 1 && n_chrom >= 1, "matcha_neg_sample_long: n_nodes=%d n_chrom=%d", n_nodes, n_chrom);
  MATCHA_CHECK_ARG(n_set_edges == 0 || (set && set_edges), "matcha_neg_sample_long: non-empty set without buffers");
  MATCHA_CHECK_ARG(L >= 1 && L <= MATCHA_MAX_LONG_L && neg_num >= 1, "matcha_neg_sample_long: L=%d neg_num=%d", L, neg_num);
  MATCHA_CHECK_ARG(L_set >= 1 && L_set <= MATCHA_MAX_LONG_L, "matcha_neg_sample_long: L_set=%d", L_set);
  MATCHA_CHECK_ARG(n_set_edges >= 0 && n_set_edges < (1ll << 31), "matcha_neg_sample_long: n_set_edges=%lld", (long long)n_set_edges);
  if (P <= 0) return MATCHA_OK;
  // the negative's index is the random stream's 32-bit hi counter, and a block owns eight negatives
  MATCHA_CHECK_ARG(P <= ((1ll << 31) - 1) / neg_num, "matcha_neg_sample_long: P=%lld x neg_num=%d negatives", (long long)P, neg_num);
  ProfScope ps(MATCHA_PROF_NEG_SAMPLE, (double)P * L * 8.0 * (1.0 + neg_num), (hipStream_t)stream);
  hipLaunchKernelGGL(neg_sample_long_kernel, dim3((unsigned)cdiv(P * neg_num, 256 / kGroup)), dim3(256), 0, (hipStream_t)stream,
                     (const int32_t*)set, set_edges, n_set_edges, L_set, pos, P, L, neg_num, min_dis, node2chrom, n_nodes,
                     chrom_range, n_chrom, seed, neg, status);
  MATCHA_CHECK_LAUNCH("neg_sample_long_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_outlier_plant(const void* set, const int64_t* set_edges, int64_t n_set_edges, int32_t L_set,
                                    const void* pair_set, const int64_t* pair_edges, int64_t n_pair_edges, int32_t L_pair,
                                    const int64_t* pos, int64_t P, int32_t L, int32_t draws, int32_t cycle, int32_t min_dis,
                                    const int32_t* node2chrom, int32_t n_nodes, const int32_t* chrom_range, int32_t n_chrom,
                                    const uint64_t* seed, int64_t n0, int64_t* out, int32_t* planted, int32_t* status, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(pos && out && planted && node2chrom && chrom_range && seed, "matcha_outlier_plant: null pointer");
  MATCHA_CHECK_ARG(((uintptr_t)chrom_range) % 8 == 0, "matcha_outlier_plant: chrom_range must be 8-byte aligned (the kernel reads [lo, hi] pairs as one int2)");
  MATCHA_CHECK_ARG(n_nodes >= 1 && n_chrom >= 1, "matcha_outlier_plant: n_nodes=%d n_chrom=%d", n_nodes, n_chrom);
  MATCHA_CHECK_ARG(n_set_edges == 0 || (set && set_edges), "matcha_outlier_plant: non-empty set without buffers");
  MATCHA_CHECK_ARG(n_pair_edges == 0 || (pair_set && pair_edges), "matcha_outlier_plant: non-empty pair set without buffers");
  MATCHA_CHECK_ARG(L >= 1 && L <= MATCHA_MAX_LONG_L && draws >= 1, "matcha_outlier_plant: L=%d draws=%d", L, draws);
  MATCHA_CHECK_ARG(L_set >= 1 && L_set <= MATCHA_MAX_LONG_L, "matcha_outlier_plant: L_set=%d", L_set);
  MATCHA_CHECK_ARG(n_set_edges >= 0 && n_set_edges < (1ll << 31), "matcha_outlier_plant: n_set_edges=%lld", (long long)n_set_edges);
  MATCHA_CHECK_ARG(n_pair_edges >= 0 && n_pair_edges < (1ll << 31), "matcha_outlier_plant: n_pair_edges=%lld", (long long)n_pair_edges);
  MATCHA_CHECK_ARG(n_pair_edges == 0 || (L_pair >= 2 && L_pair <= MATCHA_MAX_LONG_L), "matcha_outlier_plant: L_pair=%d (a pair set holds rows of two nodes)", L_pair);
  MATCHA_CHECK_ARG(n0 >= 0, "matcha_outlier_plant: n0=%lld must not be negative", (long long)n0);
  if (P <= 0) return MATCHA_OK;
  // the row's global index is the random stream's 32-bit hi counter, and a block owns eight rows
  MATCHA_CHECK_ARG(P <= ((1ll << 31) - 1) / draws, "matcha_outlier_plant: P=%lld x draws=%d rows", (long long)P, draws);
  MATCHA_CHECK_ARG(n0 <= (1ll << 31) - 1 - P * draws, "matcha_outlier_plant: n0=%lld + P*draws=%lld rows reach 2^31", (long long)n0, (long long)(P * draws));
  hipLaunchKernelGGL(outlier_plant_kernel, dim3((unsigned)cdiv(P * draws, 256 / kGroup)), dim3(256), 0, (hipStream_t)stream,
                     (const int32_t*)set, set_edges, n_set_edges, L_set, (const int32_t*)pair_set, pair_edges, n_pair_edges, L_pair, pos, P, L,
                     draws, cycle != 0 ? 1 : 0, min_dis, node2chrom, n_nodes, chrom_range, n_chrom, seed, n0, out, planted, status);
  MATCHA_CHECK_LAUNCH("outlier_plant_kernel");
  return MATCHA_OK;
}
