// The two tile-list passes of the ragged plan as block-level roles.  Both depend on the batch only (row_off, sb_first: complete
// behind row_fill_kernel); the node route's table launches in front of the encoder depend on the parameters only.
//   tile_pack_role      one wavefront packs one (superblock, list): tile_pack_kernel runs it in 64-thread blocks, the table front end's forward
//                       (front_fused.hip) in 256-thread blocks behind its own -- four tasks per block
//   tile_compact_role   one ONE-WAVEFRONT block of `nparts` scans the superblock counts and moves its share of one list: node_r_kernel
//                       (fused_fwd32.hip) hosts it.  tile_compact_kernel keeps its 1024-thread form (ragged.hip); the lists are the same bits
#pragma once
#include "kernels.hpp"

namespace matcha {

// Tiles of the fused kernels: runs of whole consecutive hyperedges with at most 63 tokens (+ the shared padding token = 64
// rows), packed greedily so the MFMA tiles are ~96 % full (fixed windows of 64 - L first-token indices gave 90 %).
// Greedy packing is sequential, so it runs per SUPERBLOCK (the hyperedges whose first token lies in a window of kSuperTok
// tokens, ~32 tiles): one wavefront per superblock loads 64 row offsets at a time; a ballot finds the first hyperedge that
// ends beyond the open tile, which closes it (about 4 closes per 64 hyperedges); only a superblock's last tile is partial.  A second kernel compacts the per-superblock lists.
// tile_meta[w] = {first token t0, tokens, first hyperedge b0, hyperedges}; entries past the tile count are zero.
constexpr int kFullTok = 63;
constexpr int kHalfTok = 31;
constexpr int kSuperTok = 63 * 32;

// one wavefront packs superblock s of one list (half = the <= 31-token list); returns the number of tiles written to out[0 .. cap_per_sb)
__device__ __forceinline__ int tile_pack_wave(const int32_t* __restrict__ row_off, int64_t B, int nsb, int s, bool half, int cap_per_sb,
                                              const int32_t* __restrict__ sb_first, int4* __restrict__ out, int lane) {
  const int kTileTok = half ? kHalfTok : kFullTok;
  const int b_lo = sb_first[s];                        // marked by the fill pass (B: nothing starts here)
  int b_hi = (int)B;
  for (int q = s + 1; q < nsb; ++q)                    // next superblock that has a first hyperedge (normally s + 1)
    if (sb_first[q] < (int)B) { b_hi = sb_first[q]; break; }
  int nt = 0;
  if (b_lo < b_hi) {
    int tile_b0 = b_lo;
    int tile_tok0 = __builtin_amdgcn_readfirstlane(row_off[b_lo]);
    for (int base = b_lo; base < b_hi; base += 64) {
      const int idx = base + lane;
      const bool valid = idx < b_hi;
      const int so = valid ? row_off[idx] : 0;         // first token of hyperedge idx
      const int eo = valid ? row_off[idx + 1] : 0;     // one past its last token (monotone over idx)
      for (;;) {
        const uint64_t over = __ballot(valid && eo - tile_tok0 > kTileTok);   // hyperedges that end beyond the open tile
        if (over == 0) break;
        const int i = __ffsll((long long)over) - 1;    // the first of them closes the tile and opens the next one
        const int start = __builtin_amdgcn_readlane(so, i);
        if (lane == 0 && nt < cap_per_sb) out[nt] = make_int4(tile_tok0, start - tile_tok0, tile_b0, base + i - tile_b0);
        ++nt;
        tile_b0 = base + i;
        tile_tok0 = start;
      }
    }
    const int end = __builtin_amdgcn_readfirstlane(row_off[b_hi]);
    if (lane == 0 && nt < cap_per_sb) out[nt] = make_int4(tile_tok0, end - tile_tok0, tile_b0, b_hi - tile_b0);
    ++nt;
  }
  return nt < cap_per_sb ? nt : cap_per_sb;
}

// list 0: tiles of <= 63 tokens; 1: half tiles of <= 31 tokens (same superblocks, own lists).  Task t = (list first + t / nsb, superblock t % nsb)
struct TilePackArgs {
  const int32_t* row_off; int64_t B; int nsb; const int32_t* sb_first;
  int cap_per_sb[2]; int32_t* sb_tiles[2]; int32_t* sb_cnt[2];
  int first, ntasks;                                   // first list built (0 or 1); nsb * (2 - first) tasks
};
__device__ __forceinline__ void tile_pack_role(const TilePackArgs& a, int task, int lane) {
  if (task >= a.ntasks) return;
  const bool half = a.first + task / a.nsb != 0;       // (the argument block's pairs are picked by selects, not indexed: an index would put a copy of the block in scratch)
  const int s = task % a.nsb;
  const int cap_per_sb = half ? a.cap_per_sb[1] : a.cap_per_sb[0];
  int32_t* sb_tiles = half ? a.sb_tiles[1] : a.sb_tiles[0];
  int32_t* sb_cnt = half ? a.sb_cnt[1] : a.sb_cnt[0];
  const int nt = tile_pack_wave(a.row_off, a.B, a.nsb, s, half, cap_per_sb, a.sb_first, reinterpret_cast<int4*>(sb_tiles) + (int64_t)s * cap_per_sb, lane);
  if (lane == 0) sb_cnt[s] = nt;
}

// exclusive scan of the superblock tile counts, compaction, zero fill; count[2 + list] = tiles
struct CompactArgs {
  const int32_t* sb_tiles[2]; int32_t* sb_cnt[2]; int cap_per_sb[2]; int ntiles_cap[2]; int32_t* meta[2];
  int nsb; int32_t* count; int first;                  // first list built (1: half tiles only -- count[2] = 0)
};
constexpr int kCompactRoleSb = 1024;                   // superblocks the role form takes (its offsets live in LDS); beyond: the stand-alone kernel
// Block `part` of `nparts` one-wavefront blocks, list a.first alone (the caller hosts the role only when one list is built).  Every block
// repeats the scan of the <= 1024 counts (a few shuffle rounds; sb_cnt is NOT rewritten in place as the stand-alone kernel does -- other blocks
// are reading it, and nobody reads the offsets afterwards), then moves tiles part * 64 + lane, + 64 nparts, ... of the compact list, finding each one's superblock by
// bisection like the stand-alone kernel, and zeroes its share of the entries behind the list.  offs: kCompactRoleSb + 1 ints of LDS.
__device__ __forceinline__ void tile_compact_role(const CompactArgs& a, int part, int nparts, int lane, int* __restrict__ offs) {
  const bool half = a.first != 0;                      // (selects, not indices: see tile_pack_role)
  const int which = half ? 1 : 0, nsb = a.nsb;
  const int32_t* __restrict__ sb_cnt = half ? a.sb_cnt[1] : a.sb_cnt[0];
  const int cap_per_sb = half ? a.cap_per_sb[1] : a.cap_per_sb[0], ntiles_cap = half ? a.ntiles_cap[1] : a.ntiles_cap[0];
  int carry = 0;
  for (int base = 0; base < nsb; base += 64) {
    const int i = base + lane;
    const int c = i < nsb ? sb_cnt[i] : 0;
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    if (i < nsb) offs[i] = carry + incl - c;
    carry += __shfl(incl, 63, 64);
  }
  const int total = carry < ntiles_cap ? carry : ntiles_cap;
  if (lane == 0) offs[nsb] = total;
  if (part == 0 && lane == 0) {
    a.count[2 + which] = total;
    if (which != 0) a.count[2] = 0;                    // half tiles only: no 64-row tile list this time
  }
  __syncthreads();                                     // (a block of one wavefront: orders the LDS writes above against the reads below)
  const int4* __restrict__ src = reinterpret_cast<const int4*>(half ? a.sb_tiles[1] : a.sb_tiles[0]);
  int4* __restrict__ dst = reinterpret_cast<int4*>(half ? a.meta[1] : a.meta[0]);
  const int step = nparts * 64;
  auto fetch = [&](int j) {                            // tile j of the compact list (clamped: four loads in flight per lane whatever the count)
    const int i = j < total ? j : total - 1;
    int lo = 0, hi = nsb;                              // the last superblock whose offset is <= i (empty ones in front of it share the offset)
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (offs[mid] <= i) lo = mid; else hi = mid; }
    return src[(int64_t)lo * cap_per_sb + (i - offs[lo])];
  };
  for (int i0 = part * 64 + lane; i0 < total; i0 += 4 * step) {      // (four named values, not an array: the array went to scratch)
    const int4 v0 = fetch(i0), v1 = fetch(i0 + step), v2 = fetch(i0 + 2 * step), v3 = fetch(i0 + 3 * step);
    dst[i0] = v0;
    if (i0 + step < total) dst[i0 + step] = v1;
    if (i0 + 2 * step < total) dst[i0 + 2 * step] = v2;
    if (i0 + 3 * step < total) dst[i0 + 3 * step] = v3;
  }
  for (int i = total + part * 64 + lane; i < ntiles_cap + 2; i += step) dst[i] = make_int4(0, 0, 0, 0);
}

// what launch_ragged_plan leaves to its caller when the two passes are to ride in later launches (ragged.hip); pending: it did
struct PlanDeferred { bool pending; TilePackArgs pack; CompactArgs compact; };
int launch_tile_pack(const TilePackArgs& a, hipStream_t st);            // the stand-alone kernels, for a host that cannot take the role
int launch_tile_compact(const CompactArgs& a, hipStream_t st);

}  // namespace matcha
