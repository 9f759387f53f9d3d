// The membership set's table format and its one-lane probes for rows of two and three nodes held in registers (the set itself is built by
// sampler.hip: matcha_hashset_build).  Shared by the outlier plant (sampler.hip) and the hypergraph walk (walk.hip).
#pragma once
#include "common.hpp"

namespace matcha {

// Set layout (round 6): 64 int32 header words (words 0..1 = capacity, a power of two), then `capacity` slots of 8 bytes: {int32 index of the
// stored hyperedge in the edge list (-1 = empty), uint32 tag = upper 32 bits of the row's hash}.  A probe reads a WINDOW of eight consecutive
// slots in one round trip (linear probing: the probe chain of a row lies inside its window with probability 1 - load^8) and compares tags;
// only a tag match costs a second trip (the stored row itself: exactness does not rest on the tag).  Rounds 1-5 kept bare indices and loaded a
// stored row per occupied slot: slot -> row -> next slot -> row ..., two dependent trips per probe, and the slowest lane of a wavefront paid
// a chain of ~5 probes -- the negative sampler was a chain of 10+ global round trips (18.8 us for 288 negatives).
constexpr int kSetHeader = 64;         // int32 words reserved in front of the slots (word 0..1 = capacity)
constexpr int kSetWindow = 8;          // slots per probe window
struct SetSlot { int32_t idx; uint32_t tag; };
static_assert(sizeof(SetSlot) == 8, "a slot is one 8-byte word (inserted with a 64-bit compare-and-swap)");
__device__ __forceinline__ uint32_t row_tag(uint64_t h) { return (uint32_t)(h >> 32); }

// one step of row_hash (sampler.hip): the hash of a row is this chain over its non-zero prefix, started at kRowHashSeed
constexpr uint64_t kRowHashSeed = 0x9E3779B97F4A7C15ull;
__device__ __forceinline__ uint64_t row_hash_step(uint64_t h, uint64_t v) {
  h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 31;
  return h;
}

// Is the pair (lo, hi), 1 <= lo < hi, a row of the pair set?  row_hash / set_contains of sampler.hip for a row of two nodes, on two registers:
// one lane, one probe chain (the reference's dict_pair lookup).
__device__ __forceinline__ bool pair_contains(const int32_t* __restrict__ set, const int64_t* __restrict__ edges, int L_set, int64_t lo, int64_t hi) {
  const int64_t cap = reinterpret_cast<const int64_t*>(set)[0];
  const unsigned long long* slots = reinterpret_cast<const unsigned long long*>(set + kSetHeader);
  const uint64_t h = row_hash_step(row_hash_step(kRowHashSeed, (uint64_t)lo), (uint64_t)hi);
  const uint32_t tag = row_tag(h);
  uint64_t p = h & (uint64_t)(cap - 1);
  for (int64_t probe = 0; probe < cap; ++probe) {
    const unsigned long long w = slots[p];
    const int32_t idx = (int32_t)(uint32_t)(w & 0xFFFFFFFFull);
    if (idx < 0) return false;
    if ((uint32_t)(w >> 32) == tag) {
      const int64_t* row = edges + (int64_t)idx * L_set;
      if (row[0] == lo && row[1] == hi && (L_set == 2 || row[2] == 0)) return true;
    }
    p = (p + 1) & (uint64_t)(cap - 1);
  }
  return false;
}

// ... and the triple (a, b, c), 1 <= a < b < c, in a set of rows of three nodes (L_set >= 3)
__device__ __forceinline__ bool triple_contains(const int32_t* __restrict__ set, const int64_t* __restrict__ edges, int L_set, int64_t a, int64_t b,
                                                int64_t c) {
  const int64_t cap = reinterpret_cast<const int64_t*>(set)[0];
  const unsigned long long* slots = reinterpret_cast<const unsigned long long*>(set + kSetHeader);
  const uint64_t h = row_hash_step(row_hash_step(row_hash_step(kRowHashSeed, (uint64_t)a), (uint64_t)b), (uint64_t)c);
  const uint32_t tag = row_tag(h);
  uint64_t p = h & (uint64_t)(cap - 1);
  for (int64_t probe = 0; probe < cap; ++probe) {
    const unsigned long long w = slots[p];
    const int32_t idx = (int32_t)(uint32_t)(w & 0xFFFFFFFFull);
    if (idx < 0) return false;
    if ((uint32_t)(w >> 32) == tag) {
      const int64_t* row = edges + (int64_t)idx * L_set;
      if (row[0] == a && row[1] == b && row[2] == c && (L_set == 3 || row[3] == 0)) return true;
    }
    p = (p + 1) & (uint64_t)(cap - 1);
  }
  return false;
}

}  // namespace matcha
