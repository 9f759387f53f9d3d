// Ragged execution plan: compact the real (non-padding) token slots of x [B, L] into a CSR list.
//
// The reference computes every padding slot like a real token (pads are attended as keys/values, SURVEY.md headline
// fact 7), but all padding slots hold the SAME vector -- tanh(next_w(0 + attribute_nn.bias)) -- so their K/V rows are
// one constant per step, their queries are masked out downstream (Modules.py:614, :309) and nothing else depends on
// them.  The HIP path therefore runs the token-level layers on  Tr real tokens + ONE shared padding token  (index Tr)
// and the attention kernels add the (L - k)-fold padding-key term in closed form.  Results are identical to the padded
// computation; the work drops by the padding fraction (30 % for k uniform in {2..5} padded to 5).
//
//   row_off [B+1]   first compact token of hyperedge b (exclusive prefix sum of k_b); row_off[B] = Tr
//   tok_slot [T+1]  compact token -> original slot b*L + l (dropout counters follow the original slots, so masks are
//                   the ones the oracle generates for the padded layout); tok_slot[Tr] = B*L
//   tok_id [T+1]    node id of the compact token; tok_id[Tr] = 0 (padding id).  Ids outside [0, n_nodes] are flagged in the
//                   caller's status word and replaced by 0, so that no later kernel indexes out of bounds
//   tok_key [T+1]   the same ids as int32 with 0 in every unused slot (the (id, gradient row) list of table_grad.hip and of
//                   the row-sparse data-parallel exchange)
//   count [4]       {Tr + 1, Tr, number of tiles, number of half tiles}  -- device-side counts consumed by every kernel through m_dev / t_dev
//   tok_pos [T+1]   position of the compact token inside its hyperedge | k << 8 (fused kernels: token -> hyperedge rows)
//   tile_meta       tiles of whole hyperedges (<= 63 tokens) for the fused d = 64 kernels (fused_bwd.hip walks these)
//   half_meta       the same token stream packed into HALF tiles of whole hyperedges with <= 31 tokens (+ the shared padding token =
//                   32 rows: one wavefront of the wave-independent fused forward, fused_fwd32.hip); count[3] = number of half tiles
//   tok_tile [T+1]  compact token -> (tile << 6) | row inside that tile: where the forward's wavefront stores the token's Q / K / V
//                   rows for the backward kernel, whose 64-row tiles cut the stream at other places than the half tiles
//   row_src [B]     packed plans only (launch_ragged_plan's `packed`, the fused d = 64 step): the plan's rows are a permutation of the batch's, ordered
//                   by size class so that the half tiles fill to 31 tokens; row_src[b'] = batch row of plan row b'.  Every array above is then in
//                   plan order (tok_slot still names the ORIGINAL slot).  matcha_ragged_plan never packs
#include "kernels.hpp"
#include "ragged_roles.hpp"

namespace matcha {

constexpr int kRpt = 1;                      // rows per thread of the counting / filling passes (round 6: 1 -- four rows per thread left 64 workgroups for the
                                             // bench's 65 536 rows, a quarter of the CUs, each thread a serial chain of ~56 scattered stores: 12.9 us; now 256 workgroups)
constexpr int kRowsPerBlock = 256 * kRpt;

__device__ __forceinline__ int block_exclusive_scan_256(int v, int* lds4, int* total) {
  // 256 threads: inclusive scan inside each wave, then the 4 wave totals
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

// ---- the packed row order ("Packed row order"): rows by size class, so that the greedy packer's half tiles fill to 31 tokens ------------------------
// A row's class is its number of real tokens k = 0 .. MATCHA_MAX_L.  row_count_kernel leaves the classes' counts per block (cls_hist [nblk][16]),
// row_scan_kernel turns them into per-class bases and lets one wavefront derive the SCHEDULE from the class totals: phases (recipe a_k = rows of
// class k per half tile with sum k a_k <= 31, m tiles), a phase ending when a class cannot fill another tile; the last phase takes what is left,
// class by class.  Inside a tile the classes stand in ascending order.  Row r of class k (r in batch order) then has its plan row and first token
// in closed form (row_fill_kernel).  tests/row_pack_ref.py is the twin of all of it, integer for integer.
constexpr int kPackCls = MATCHA_MAX_L + 1;
constexpr int kPackPhases = 12;
constexpr int kPackTailTok = 64 * kHalfTok;        // at most this many tokens left (or 1 / 32 of the batch's): the remaining rows in class order (the greedy packer's loss there: a few tiles)
constexpr int kPackStride = 56;                    // ints per phase: m, rows, toks, row_base, tok_base, pred_k, last_k, -, then five arrays of kPackCls
constexpr int kPackHead = 16;                      // sched[0] = number of phases; the phases start here
constexpr int kPhA = 8, kPhRowIn = kPhA + kPackCls, kPhTokIn = kPhRowIn + kPackCls, kPhBase = kPhTokIn + kPackCls, kPhPrevK = kPhBase + kPackCls;
static_assert(kPhPrevK + kPackCls <= kPackStride && kPackCls <= 16 && kRpt == 1, "schedule layout");
size_t ragged_pack_sched_bytes() { return (size_t)(kPackHead + kPackPhases * kPackStride) * 4; }
size_t ragged_pack_hist_bytes(int64_t B) { return (size_t)cdiv(B, kRowsPerBlock) * 16 * 4; }

__global__ __launch_bounds__(256) void row_count_kernel(const int64_t* __restrict__ x, int64_t B, int L, int32_t* __restrict__ blk_sum,
                                                        int32_t* __restrict__ cls_hist) {
  __shared__ int lds4[4];
  __shared__ int hist[16];
  const int64_t b0 = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x * kRpt;
  int cnt = 0;
  for (int i = 0; i < kRpt; ++i)
    if (b0 + i < B)
      for (int l = 0; l < L; ++l) cnt += x[(b0 + i) * L + l] != 0 ? 1 : 0;
  if (cls_hist && threadIdx.x < 16) hist[threadIdx.x] = 0;
  int total;
  (void)block_exclusive_scan_256(cnt, lds4, &total);     // (its barrier orders the zeros above against the adds below)
  if (threadIdx.x == 0) blk_sum[blockIdx.x] = total;
  if (cls_hist) {
    const int cls = b0 < B ? cnt : -1;
#pragma unroll
    for (int c = 0; c < kPackCls; ++c) {
      const uint64_t m = __ballot(cls == c);
      if ((threadIdx.x & 63) == 0 && m) atomicAdd(&hist[c], __popcll(m));
    }
    __syncthreads();
    if (threadIdx.x < 16) cls_hist[(int64_t)blockIdx.x * 16 + threadIdx.x] = hist[threadIdx.x];
  }
}

// one wavefront, lane c = class c: the schedule from the class totals (tests/row_pack_ref.py: schedule, _recipe)
__device__ __forceinline__ int pack_lane_sum(int v) {      // over the kPackCls class lanes, uniform result
  int s = 0;
#pragma unroll
  for (int c = 0; c < kPackCls; ++c) s += __builtin_amdgcn_readlane(v, c);
  return s;
}
__device__ __forceinline__ void pack_schedule(const int* __restrict__ ntot, int32_t* __restrict__ sched, int lane) {
  const int c = lane;
  int rem = c < kPackCls ? ntot[c] : 0;
  int row_base = 0, tok_base = 0, cls_base = 0, pred_k = 0, np = 0;
  const int tail_tok = max(kPackTailTok, pack_lane_sum(c * rem) >> 5);      // the last 1 / 32 of the tokens (at least 64 tiles' worth): in class order
  while (pack_lane_sum(rem) > 0) {
    const int T = pack_lane_sum(c * rem);
    const bool last = np == kPackPhases - 1 || T <= tail_tok;
    int a = rem, m = 1;
    if (!last) {
      // the classes' shares of the remaining tokens, rounded down ...
      int s = 0;
      while ((T >> s) >= (1 << 26)) ++s;
      const int rs = rem >> s;
      const int Ts = pack_lane_sum(c * rs);
      a = 0;                                             // (class 0 and the idle lanes take no share: their product below could overflow, and Ts may be 0)
      if (c >= 1 && c < kPackCls && Ts > 0) a = min(rem, (int)(((uint32_t)kHalfTok * (uint32_t)rs) / (uint32_t)Ts));
      const int left = kHalfTok - pack_lane_sum(c * a);
      // ... and the slots left filled exactly: a bounded knapsack over what remains, classes 8 .. 1 (reach: bit w = w tokens can be added)
      const int spare = rem - a;
      uint32_t reach = 1u, before[kPackCls];
#pragma unroll
      for (int cc = MATCHA_MAX_L; cc >= 1; --cc) {
        before[cc] = reach;
        const int avail = min(__builtin_amdgcn_readlane(spare, cc), left / cc);
        for (int j = 0; j < avail; ++j) reach |= reach << cc;
        reach &= 0xffffffffu >> (31 - left);
      }
      int w = 31 - __clz((int)reach);
#pragma unroll
      for (int cc = 1; cc <= MATCHA_MAX_L; ++cc) {
        int j = 0;
        while (j * cc < w && !((before[cc] >> (w - j * cc)) & 1u)) ++j;
        if (c == cc) a += j;
        w -= j * cc;
      }
      // tiles until a class cannot fill another one; the all-padding rows spread over them
      int q = (c >= 1 && c < kPackCls && a > 0) ? (int)((uint32_t)rem / (uint32_t)a) : 0x7fffffff;
      m = q;
#pragma unroll
      for (int cc = 1; cc < kPackCls; ++cc) m = min(m, __builtin_amdgcn_readlane(q, cc));
      if (c == 0) a = (int)((uint32_t)rem / (uint32_t)m);
    }
    int row_in = 0, tok_in = 0, prev_k = -1, last_k = -1, rows = 0, toks = 0;
#pragma unroll
    for (int cc = 0; cc < kPackCls; ++cc) {
      const int ac = __builtin_amdgcn_readlane(a, cc);
      if (c == cc) { row_in = rows; tok_in = toks; prev_k = last_k; }
      rows += ac;
      toks += cc * ac;
      if (ac > 0) last_k = cc;
    }
    int32_t* ph = sched + kPackHead + np * kPackStride;
    if (c == 0) { ph[0] = m; ph[1] = rows; ph[2] = toks; ph[3] = row_base; ph[4] = tok_base; ph[5] = pred_k; ph[6] = last_k; }
    if (c < kPackCls) { ph[kPhA + c] = a; ph[kPhRowIn + c] = row_in; ph[kPhTokIn + c] = tok_in; ph[kPhBase + c] = cls_base; ph[kPhPrevK + c] = prev_k; }
    rem -= m * a;
    cls_base += m * a;
    row_base += m * rows;
    tok_base += m * toks;
    pred_k = last_k;
    ++np;
    if (last) break;
  }
  if (lane == 0) sched[0] = np;
}

// exclusive scan of the block sums in place; count = {Tr + 1, Tr}
__global__ __launch_bounds__(1024) void row_scan_kernel(int32_t* __restrict__ blk_sum, int nblk, int32_t* __restrict__ count,
                                                        int32_t* __restrict__ sb_first, int nsb, int32_t n_rows,
                                                        int32_t* __restrict__ cls_hist, int32_t* __restrict__ sched) {
  __shared__ int part[1024];
  for (int i = threadIdx.x; i <= nsb; i += 1024) sb_first[i] = n_rows;       // superblocks in which no hyperedge starts: empty range
  // packed order: wavefront c < kPackCls scans class c's per-block counts (64 lanes, nblk / 64 blocks each).  Their loads go first, the totals
  // reach LDS in front of the barrier below, and the LAST wavefront derives the schedule behind it while the others write their bases
  __shared__ int ntot[16];
  const int hch = (nblk + 63) / 64;
  const int hlane = threadIdx.x & 63, hcls = threadIdx.x >> 6;
  const int h0 = hlane * hch < nblk ? hlane * hch : nblk, h1 = h0 + hch < nblk ? h0 + hch : nblk;
  const bool hist_wave = cls_hist && hcls < kPackCls;
  int hloc = 0;
  if (hist_wave)
    for (int b = h0; b < h1; ++b) hloc += cls_hist[(int64_t)b * 16 + hcls];
  const int chunk = (nblk + 1023) / 1024;
  const int b0 = threadIdx.x * chunk, b1 = (b0 + chunk < nblk) ? b0 + chunk : nblk;
  int local = 0;
  for (int b = b0; b < b1; ++b) local += blk_sum[b];
  // exclusive scan of the 1024 per-thread sums: inclusive scan inside each wavefront (six shuffle steps), then the sixteen wave totals
  // (a serial pass of thread 0 over the 1024 entries cost 8 us of this 10 us kernel at every batch size)
  __shared__ int wtot[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wtot[wave] = incl;
  int hinc = hloc;
  if (hist_wave) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(hinc, o, 64);
      if (lane >= o) hinc += u;
    }
    if (lane == 63) ntot[wave] = hinc;
  }
  __syncthreads();
  if (cls_hist && wave == 15) pack_schedule(ntot, sched, lane);
  int wbase = 0, total = 0;
#pragma unroll
  for (int w2 = 0; w2 < 16; ++w2) { const int v = wtot[w2]; if (w2 < wave) wbase += v; total += v; }
  part[threadIdx.x] = wbase + incl - local;
  if (threadIdx.x == 0) {
    count[0] = total + 1;
    count[1] = total;
  }
  int run = part[threadIdx.x];
  for (int b = b0; b < b1; ++b) { const int v = blk_sum[b]; blk_sum[b] = run; run += v; }
  if (hist_wave) {                                       // the class's exclusive bases per counting block, in place
    int at = hinc - hloc;
    for (int b = h0; b < h1; ++b) { const int v = cls_hist[(int64_t)b * 16 + hcls]; cls_hist[(int64_t)b * 16 + hcls] = at; at += v; }
  }
}

// PACK: the rows go to the plan rows and token positions of the schedule (row_src[plan row] = batch row; tok_slot keeps the ORIGINAL slot, which
// keys the dropout counters); otherwise plan row = batch row, bit for bit the plan of every earlier version
template <bool PACK>
__global__ __launch_bounds__(256) void row_fill_kernel(const int64_t* __restrict__ x, int64_t B, int L, const int32_t* __restrict__ blk_base,
                                                       const int32_t* __restrict__ count, int32_t* __restrict__ row_off,
                                                       int32_t* __restrict__ tok_slot, int64_t* __restrict__ tok_id,
                                                       int32_t* __restrict__ tok_pos, int32_t* __restrict__ sb_first, int super_tok,
                                                       int32_t* __restrict__ tok_key, int64_t n_nodes, int32_t* __restrict__ status,
                                                       int64_t* __restrict__ node_ids, int32_t* __restrict__ node_cnt, float* __restrict__ node_zero,
                                                       const int32_t* __restrict__ cls_base, const int32_t* __restrict__ sched, int32_t* __restrict__ row_src,
                                                       const float* __restrict__ y_in, const float* __restrict__ w_in, float* __restrict__ y_plan, float* __restrict__ w_plan) {
  __shared__ int lds4[4];
  __shared__ int sch[PACK ? kPackHead + kPackPhases * kPackStride : 1];
  __shared__ int wcls[4][16];
  const int64_t b0 = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x * kRpt;
  // this thread's rows (and the row in front of them) in registers: ONE round of loads, all in flight together, on clamped
  // addresses with the masks applied to the values (the first version read x three times behind dependent waits)
  int64_t v[kRpt][MATCHA_MAX_L], vp[MATCHA_MAX_L];
#pragma unroll
  for (int i = 0; i < kRpt; ++i) {
    const int64_t bc = b0 + i < B ? b0 + i : B - 1;
#pragma unroll
    for (int l = 0; l < MATCHA_MAX_L; ++l) v[i][l] = x[bc * L + (l < L ? l : L - 1)];
  }
  float yv = 0.f, wv = 0.f;
  if (PACK) {
    // the whole schedule table into LDS (phases past the count hold whatever the workspace held: never read), no dependent read of its length
    for (int i = threadIdx.x; i < kPackHead + kPackPhases * kPackStride; i += 256) sch[i] = sched[i];
    const int64_t bc = b0 < B ? b0 : B - 1;
    if (y_in) yv = y_in[bc];
    if (w_in) wv = w_in[bc];
  } else {
    const int64_t bp = b0 > 0 ? (b0 - 1 < B ? b0 - 1 : B - 1) : 0;
#pragma unroll
    for (int l = 0; l < MATCHA_MAX_L; ++l) vp[l] = x[bp * L + (l < L ? l : L - 1)];
  }
  int kk[kRpt], cnt = 0;
#pragma unroll
  for (int i = 0; i < kRpt; ++i) {
    int k = 0;
#pragma unroll
    for (int l = 0; l < MATCHA_MAX_L; ++l) {
      v[i][l] = (b0 + i < B && l < L) ? v[i][l] : 0;
      k += v[i][l] != 0 ? 1 : 0;
    }
    kk[i] = k;
    cnt += k;
  }
  int kprev = 0;
  if (!PACK) {
#pragma unroll
    for (int l = 0; l < MATCHA_MAX_L; ++l) kprev += (b0 > 0 && l < L && vp[l] != 0) ? 1 : 0;
  }
  int pos = 0;
  int64_t bdst = b0;                                     // plan row of this thread's row
  if (PACK) {
    // rank of the row inside its class: the block's base + the rows of the class in front of it in the block (ballots, the waves' counts through LDS)
    const int cls = b0 < B ? kk[0] : -1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int rk = 0;
#pragma unroll
    for (int c = 0; c < kPackCls; ++c) {
      const uint64_t m = __ballot(cls == c);
      if (cls == c) rk = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) wcls[wave][c] = __popcll(m);
    }
    __syncthreads();                                     // wcls and the schedule in LDS
    if (cls >= 0) {
      for (int w = 0; w < wave; ++w) rk += wcls[w][cls];
      const int r = cls_base[(int64_t)blockIdx.x * 16 + cls] + rk;
      int p = 0;                                         // the last phase whose class base is <= r holds the row
      for (int q = 1; q < sch[0]; ++q)
        if (sch[kPackHead + q * kPackStride + kPhBase + cls] <= r) p = q;
      const int* ph = sch + kPackHead + p * kPackStride;
      const int a = ph[kPhA + cls], q = r - ph[kPhBase + cls];
      const int t = (int)((uint32_t)q / (uint32_t)a), j = q - t * a;
      bdst = ph[3] + t * ph[1] + ph[kPhRowIn + cls] + j;
      pos = ph[4] + t * ph[2] + ph[kPhTokIn + cls] + j * cls;
      // the plan row in front: the slot before this one in the recipe, the last slot of the tile before, or of the phase before
      kprev = j > 0 ? cls : ph[kPhPrevK + cls] >= 0 ? ph[kPhPrevK + cls] : t > 0 ? ph[6] : ph[5];
    }
  } else {
    pos = blk_base[blockIdx.x] + block_exclusive_scan_256(cnt, lds4, nullptr);
  }
#pragma unroll
  for (int i = 0; i < kRpt; ++i) {
    const int64_t b = b0 + i;
    if (b < B) {
      row_off[bdst] = pos;
      if (PACK) {                                        // the batch row of the plan row, and the row's targets in plan order (the forward's tail reads them by plan row)
        row_src[bdst] = (int32_t)b;
        if (y_in) y_plan[bdst] = yv;
        if (w_in) w_plan[bdst] = wv;
      }
      const int k = kk[i];
      // first hyperedge of a planning superblock: its first token lies in another window of super_tok tokens than its predecessor's
      if (bdst == 0 || pos / super_tok != (pos - kprev) / super_tok) sb_first[pos / super_tok] = (int32_t)bdst;
      kprev = k;
      int nth = 0;
#pragma unroll
      for (int l = 0; l < MATCHA_MAX_L; ++l) {
        int64_t id = v[i][l];
        if (id != 0) {
          if (id < 0 || id > n_nodes) {                  // the reference raises IndexError here (nn.Embedding, Modules.py:34)
            if (status) atomicOr(status, MATCHA_STATUS_BAD_ID);
            id = 0;
          }
          tok_slot[pos] = (int32_t)(b * L + l); tok_id[pos] = id; tok_key[pos] = (int32_t)id; tok_pos[pos] = nth | (k << 8); ++pos; ++nth;
        }
      }
    }
  }
  const int tr = count[1];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    row_off[B] = tr;
    tok_slot[tr] = (int32_t)(B * L);
    tok_id[tr] = 0;
    tok_pos[tr] = 0;
  }
  // tok_key of every slot behind the real tokens is 0 (the padding token's included): written here instead of a memset of the whole
  // array in front of the plan (the real tokens' keys are written above by their owners; nobody else touches slots >= tr)
  for (int64_t i = tr + (int64_t)blockIdx.x * 256 + threadIdx.x; i < B * L + 1; i += (int64_t)gridDim.x * 256) tok_key[i] = 0;
  // node route of the table front end (model.hip): the id list 0..n_nodes and its length, written here like tok_key's zeros -- no memset, no copy
  if (node_ids) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= n_nodes; i += (int64_t)gridDim.x * 256) node_ids[i] = i;
    if (blockIdx.x == 0 && threadIdx.x == 0) { node_cnt[0] = (int32_t)(n_nodes + 1); node_cnt[1] = (int32_t)n_nodes; }
  }
  if (node_zero)      // ... and the zeros of the backward's per-node accumulator [n_nodes + 1][64]
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (n_nodes + 1) * 16; i += (int64_t)gridDim.x * 256)
      reinterpret_cast<float4*>(node_zero)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// (the tiles' definition, tile_pack_wave and the argument blocks of the two tile-list passes: ragged_roles.hpp -- both passes also run as block
// roles of the node route's table launches, model.hip)
__global__ __launch_bounds__(64) void tile_pack_kernel(TilePackArgs a) {
  tile_pack_role(a, (int)blockIdx.y * a.nsb + (int)blockIdx.x, threadIdx.x);
}

// exclusive scan of the superblock tile counts (one block, 1024 counts per pass), compaction, zero fill; count[2] = tiles
// blockIdx.x = 0: tiles -> tile_meta, count[2];  1: half tiles -> half_meta, count[3]
__global__ __launch_bounds__(1024) void tile_compact_kernel(CompactArgs a) {
  const int nsb = a.nsb, x0 = a.first;
  int32_t* __restrict__ count = a.count;
  const int which = (int)blockIdx.x + x0;
  if (x0 != 0 && threadIdx.x == 0) count[2] = 0;       // half tiles only: no 64-row tile list this time
  const int32_t* __restrict__ sb_tiles = a.sb_tiles[which];
  int32_t* __restrict__ sb_cnt = a.sb_cnt[which];
  const int cap_per_sb = a.cap_per_sb[which], ntiles_cap = a.ntiles_cap[which];
  int32_t* __restrict__ meta = a.meta[which];
  __shared__ int wtot[16];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int base = 0; base < nsb; base += 1024) {
    const int i = base + threadIdx.x;
    const int c = i < nsb ? sb_cnt[i] : 0;
    // inclusive scan inside each wavefront (six shuffle steps), then the sixteen wave totals (a Hillis-Steele pass over LDS took
    // twenty barriers per 1024 counts)
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(incl, o, 64);
      if (lane >= o) incl += u;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int wbase = 0, tot = 0;
#pragma unroll
    for (int w2 = 0; w2 < 16; ++w2) { const int v = wtot[w2]; if (w2 < wave) wbase += v; tot += v; }
    if (i < nsb) sb_cnt[i] = carry + wbase + incl - c;
    __syncthreads();
    if (threadIdx.x == 0) carry += tot;
    __syncthreads();
  }
  const int total = carry < ntiles_cap ? carry : ntiles_cap;
  if (threadIdx.x == 0) count[2 + which] = total;
  __syncthreads();                                     // sb_cnt (now offsets) written by this block: visible after the barrier
  const int4* __restrict__ src = reinterpret_cast<const int4*>(sb_tiles);
  int4* __restrict__ dst = reinterpret_cast<int4*>(meta);
  __shared__ int offs[1025];
  if (nsb <= 1024) {
    // the offsets of the superblocks in LDS; every thread then moves tiles i = tid, tid + 1024, ... of the COMPACT list, finding each one's
    // superblock by bisection over the offsets -- independent loads, four in flight per thread (a wavefront per superblock was a chain of
    // nsb / 16 dependent round trips)
    for (int i = threadIdx.x; i < nsb; i += 1024) offs[i] = sb_cnt[i];
    if (threadIdx.x == 0) offs[nsb] = total;
    __syncthreads();
    for (int i0 = threadIdx.x; i0 < total; i0 += 4 * 1024) {
      int4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * 1024 < total ? i0 + u * 1024 : total - 1;
        int lo = 0, hi = nsb;                          // the last superblock whose offset is <= i (empty ones in front of it share the offset)
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (offs[mid] <= i) lo = mid; else hi = mid; }
        v[u] = src[(int64_t)lo * cap_per_sb + (i - offs[lo])];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i0 + u * 1024 < total) dst[i0 + u * 1024] = v[u];
    }
  } else {
    // one wavefront per superblock: its (few) tiles move as consecutive int4
    for (int s = wave; s < nsb; s += 16) {
      const int lo = sb_cnt[s], hi = (s + 1 < nsb) ? sb_cnt[s + 1] : total;
      for (int j = lane; lo + j < hi && j < cap_per_sb; j += 64)
        if (lo + j < ntiles_cap) dst[lo + j] = src[(int64_t)s * cap_per_sb + j];
    }
  }
  for (int i = total + threadIdx.x; i < ntiles_cap + 2; i += 1024) dst[i] = make_int4(0, 0, 0, 0);
}

// tok_tile[t] = (tile << 6) | row for every token of every planned tile (one 64-thread block per tile slot; slots past the count are zero)
__global__ __launch_bounds__(64) void tok_tile_kernel(const int32_t* __restrict__ meta, int32_t* __restrict__ tok_tile) {
  const int4 m = reinterpret_cast<const int4*>(meta)[blockIdx.x];
  if ((int)threadIdx.x < m.y) tok_tile[m.x + threadIdx.x] = (int32_t)((blockIdx.x << 6) | threadIdx.x);
}

// ---- the whole plan in ONE launch for small batches (B <= 1024 rows, <= 8 planning superblocks: the reference's own 384-row step) ------------
// The five kernels above are five dependent launches of a few microseconds each -- at 384 rows a tenth of the step (main.py:527-528).  Here
// one workgroup of 1024 threads does the same work in the same order and writes the SAME plan bit for bit (tests/test_hip_kernels.py compares
// both paths with oracle/c/ragged_plan.c): thread b owns hyperedge b (count, block scan, token lists), wavefronts pack the superblocks of the
// two lists side by side, the lists are compacted by offset, the token -> tile map follows.
constexpr int kSmallRows = 1024;
constexpr int kSmallSb = 8;
struct PlanSmallArgs {
  const int64_t* x; int64_t B; int L; int64_t n_nodes; int32_t* status;
  int32_t *row_off, *tok_slot; int64_t* tok_id; int32_t *tok_pos, *tok_key, *count, *sb_first;
  int nsb, level;
  int32_t* sb_tiles[2]; int cap_per_sb[2]; int ntiles_cap[2]; int32_t* meta[2];
  int32_t* tok_tile;
  float* node_zero; int64_t* node_ids; int32_t* node_cnt;      // node route of the table front end: the id list 0..n_nodes and its length (null: not asked)
};
__global__ __launch_bounds__(1024) void plan_small_kernel(PlanSmallArgs a) {
  __shared__ int wtot[16];
  __shared__ int sbf[kSmallSb + 1];
  __shared__ int cnt[2][kSmallSb];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = a.L;
  const int64_t B = a.B;
  const bool on = tid < B;
  int64_t v[MATCHA_MAX_L];
  int k = 0;
#pragma unroll
  for (int l = 0; l < MATCHA_MAX_L; ++l) {
    v[l] = (on && l < L) ? a.x[(int64_t)tid * L + l] : 0;
    k += v[l] != 0 ? 1 : 0;
  }
  if (tid <= a.nsb && tid <= kSmallSb) sbf[tid] = (int)B;              // superblocks in which no hyperedge starts: empty range
  int incl = k;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  int wbase = 0, total = 0;
#pragma unroll
  for (int w2 = 0; w2 < 16; ++w2) { const int t = wtot[w2]; if (w2 < wave) wbase += t; total += t; }
  int pos = wbase + incl - k;
  const int kprev = __shfl_up(k, 1, 64);
  int kp = lane > 0 ? kprev : 0;
  // (the row in front of a wave's first row: its k through LDS)
  __shared__ int klast[16];
  if (lane == 63) klast[wave] = k;
  __syncthreads();
  if (lane == 0 && wave > 0) kp = klast[wave - 1];
  if (on) {
    a.row_off[tid] = pos;
    if (tid == 0 || pos / kSuperTok != (pos - kp) / kSuperTok) sbf[pos / kSuperTok] = tid;
    int nth = 0, p = pos;
#pragma unroll
    for (int l = 0; l < MATCHA_MAX_L; ++l) {
      int64_t id = v[l];
      if (id != 0) {
        if (id < 0 || id > a.n_nodes) {                  // the reference raises IndexError here (nn.Embedding, Modules.py:34)
          if (a.status) atomicOr(a.status, MATCHA_STATUS_BAD_ID);
          id = 0;
        }
        a.tok_slot[p] = (int32_t)(tid * L + l); a.tok_id[p] = id; a.tok_key[p] = (int32_t)id; a.tok_pos[p] = nth | (k << 8); ++p; ++nth;
      }
    }
  }
  if (tid == 0) {
    a.row_off[B] = total;
    a.tok_slot[total] = (int32_t)(B * L);
    a.tok_id[total] = 0;
    a.tok_pos[total] = 0;
    a.count[0] = total + 1;
    a.count[1] = total;
    if (a.level <= 0) { a.count[2] = 0; a.count[3] = 0; }
  }
  for (int64_t i = total + tid; i < B * L + 1; i += 1024) a.tok_key[i] = 0;
  if (a.node_ids) {
    for (int64_t i = tid; i <= a.n_nodes; i += 1024) a.node_ids[i] = i;
    if (tid == 0) { a.node_cnt[0] = (int32_t)(a.n_nodes + 1); a.node_cnt[1] = (int32_t)a.n_nodes; }
  }
  if (a.node_zero)
    for (int64_t i = tid; i < (a.n_nodes + 1) * 16; i += 1024) reinterpret_cast<float4*>(a.node_zero)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();                                       // row_off (global) and sbf (LDS) are complete
  if (tid <= a.nsb) a.sb_first[tid] = sbf[tid < kSmallSb ? tid : kSmallSb];
  if (a.level <= 0) return;
  const int first = a.level >= 2 ? 0 : 1;                // list 0: 64-row tiles, list 1: half tiles
  for (int task = wave; task < a.nsb * (2 - first); task += 16) {
    const int which = first + task / a.nsb, sb = task - (task / a.nsb) * a.nsb;
    const int nt = tile_pack_wave(a.row_off, B, a.nsb, sb, which != 0, a.cap_per_sb[which], sbf,
                                  reinterpret_cast<int4*>(a.sb_tiles[which]) + (int64_t)sb * a.cap_per_sb[which], lane);
    if (lane == 0) cnt[which][sb] = nt;
  }
  __syncthreads();                                       // the per-superblock lists (global scratch) and their counts
  for (int which = first; which < 2; ++which) {
    int off[kSmallSb + 1];
    int run = 0;
    for (int sb = 0; sb < a.nsb; ++sb) { off[sb] = run; run += cnt[which][sb]; }
    const int tot = run < a.ntiles_cap[which] ? run : a.ntiles_cap[which];
    if (tid == 0) a.count[2 + which] = tot;
    const int4* src = reinterpret_cast<const int4*>(a.sb_tiles[which]);
    int4* dst = reinterpret_cast<int4*>(a.meta[which]);
    for (int sb = wave; sb < a.nsb; sb += 16)
      for (int j = lane; j < cnt[which][sb]; j += 64)
        if (off[sb] + j < a.ntiles_cap[which]) dst[off[sb] + j] = src[(int64_t)sb * a.cap_per_sb[which] + j];
    for (int i = tot + tid; i < a.ntiles_cap[which] + 2; i += 1024) dst[i] = make_int4(0, 0, 0, 0);
  }
  if (first != 0 && tid == 0) a.count[2] = 0;            // half tiles only: no 64-row tile list this time
  if (a.level >= 2) {
    __syncthreads();                                     // tile_meta complete
    const int4* tm = reinterpret_cast<const int4*>(a.meta[0]);
    for (int t = wave; t < a.ntiles_cap[0]; t += 16) {
      const int4 m = tm[t];
      if (lane < m.y) a.tok_tile[m.x + lane] = (int32_t)((t << 6) | lane);
    }
  }
}

static inline int super_blocks(int64_t T) { return (int)cdiv(T + 1, kSuperTok); }
static inline int super_cap(int L) { return (int)cdiv(kSuperTok + L, 64 - L) + 2; }
static inline int tiles_cap(int64_t T, int L) { return (int)cdiv(T + 1, 64 - L) + super_blocks(T); }   // every tile but a superblock's last holds > 63 - L tokens
static inline int super_hcap(int L) { return (int)cdiv(kSuperTok + L, 32 - L) + 2; }
static inline int halves_cap(int64_t T, int L) { return (int)cdiv(T + 1, 32 - L) + super_blocks(T); }  // ... > 31 - L tokens

int ragged_tiles_cap(int64_t B, int L) { return tiles_cap(B * L, L); }
int ragged_halves_cap(int64_t B, int L) { return halves_cap(B * L, L); }

size_t ragged_bytes(int64_t B, int L) {
  const int64_t T = B * L;
  size_t n = 0;
  n += align_up((size_t)(B + 1) * 4, 256);        // row_off
  n += align_up((size_t)(T + 1) * 4, 256);        // tok_slot
  n += align_up((size_t)(T + 1) * 8, 256);        // tok_id
  n += 256;                                        // count
  n += align_up((size_t)cdiv(B, kRowsPerBlock) * 4, 256);
  n += align_up((size_t)(T + 1) * 4, 256);        // tok_pos
  n += align_up((size_t)(T + 1) * 4, 256);        // tok_key
  n += align_up((size_t)(tiles_cap(T, L) + 2) * 16, 256);                    // tile_meta
  n += align_up((size_t)super_blocks(T) * super_cap(L) * 16, 256);           // sb_tiles
  n += align_up((size_t)super_blocks(T) * 4, 256);                           // sb_cnt
  n += align_up((size_t)(super_blocks(T) + 1) * 4, 256);                     // sb_first
  n += align_up((size_t)(halves_cap(T, L) + 2) * 16, 256);                   // half_meta
  n += align_up((size_t)super_blocks(T) * super_hcap(L) * 16, 256);          // sb_htiles
  n += align_up((size_t)super_blocks(T) * 4, 256);                           // sb_hcnt
  n += align_up((size_t)(T + 1) * 4, 256);                                   // tok_tile
  return n;
}

void ragged_carve(int64_t B, int L, char* base, Ragged& r) {
  const int64_t T = B * L;
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base + off; off += align_up(bytes, 256); return p; };
  r.row_off = (int32_t*)take((size_t)(B + 1) * 4);
  r.tok_slot = (int32_t*)take((size_t)(T + 1) * 4);
  r.tok_id = (int64_t*)take((size_t)(T + 1) * 8);
  r.count = (int32_t*)take(256);
  r.blk_sum = (int32_t*)take((size_t)cdiv(B, kRowsPerBlock) * 4);
  r.nblk = (int)cdiv(B, kRowsPerBlock);
  r.ntiles = tiles_cap(T, L);
  r.tok_pos = (int32_t*)take((size_t)(T + 1) * 4);
  r.tok_key = (int32_t*)take((size_t)(T + 1) * 4);
  r.tile_meta = (int32_t*)take((size_t)(r.ntiles + 2) * 16);
  r.nsb = super_blocks(T);
  r.sb_cap = super_cap(L);
  r.sb_tiles = (int32_t*)take((size_t)r.nsb * r.sb_cap * 16);
  r.sb_cnt = (int32_t*)take((size_t)r.nsb * 4);
  r.sb_first = (int32_t*)take((size_t)(r.nsb + 1) * 4);
  r.nhalves = halves_cap(T, L);
  r.sb_hcap = super_hcap(L);
  r.half_meta = (int32_t*)take((size_t)(r.nhalves + 2) * 16);
  r.sb_htiles = (int32_t*)take((size_t)r.nsb * r.sb_hcap * 16);
  r.sb_hcnt = (int32_t*)take((size_t)r.nsb * 4);
  r.tok_tile = (int32_t*)take((size_t)(T + 1) * 4);
  // The packed row order's arrays take no bytes of their own (the plan's and the workspace's sizes are what they were): a plan that stops at the
  // half tiles (level <= 1, the only kind that packs) builds neither the 64-row tile list nor the token -> tile map, and the arrays live in those
  // three regions.  Where they do not fit (L <= 2, or fewer than five planning superblocks) the pointers stay null and the plan does not pack.
  r.row_src = nullptr; r.cls_hist = nullptr; r.sched = nullptr; r.y_plan = nullptr; r.w_plan = nullptr;
  if ((size_t)3 * B <= (size_t)T + 1 && ragged_pack_hist_bytes(B) <= (size_t)(r.ntiles + 2) * 16 && ragged_pack_sched_bytes() <= (size_t)r.nsb * r.sb_cap * 16) {
    r.row_src = r.tok_tile;
    r.y_plan = reinterpret_cast<float*>(r.tok_tile + B);
    r.w_plan = reinterpret_cast<float*>(r.tok_tile + 2 * B);
    r.cls_hist = r.tile_meta;
    r.sched = r.sb_tiles;
  }
}

// the two tile-list passes as launches of their own (the plan below; a host kernel that cannot take the role)
int launch_tile_pack(const TilePackArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(tile_pack_kernel, dim3(a.nsb, 2 - a.first), dim3(64), 0, st, a);
  MATCHA_CHECK_LAUNCH("tile_pack_kernel");
  return MATCHA_OK;
}
int launch_tile_compact(const CompactArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(tile_compact_kernel, dim3(2 - a.first), dim3(1024), 0, st, a);
  MATCHA_CHECK_LAUNCH("tile_compact_kernel");
  return MATCHA_OK;
}

// level 2: everything; 1: no 64-row tile list and no token -> tile map (the fused kernels that run work on half tiles only); 0: rows and
// tokens only (no fused kernel will read a tile list)
// defer != null: with the five-launch plan at level 1 the two tile-list passes are NOT launched -- their argument blocks are left in *defer
// (pending = true) for the caller, who runs them as roles of later launches or through launch_tile_pack / launch_tile_compact, in that order
// packed: the rows in the packed order (above) -- the caller asks only where ragged_plan_packs says the plan takes it, and hands r.row_src to its consumers
bool ragged_plan_packs(int64_t B, const Ragged& r) {
  return r.row_src && r.cls_hist && r.sched && r.y_plan && r.w_plan && !(B <= kSmallRows && r.nsb <= kSmallSb && !options().disable_small_batch);
}
int launch_ragged_plan(const int64_t* x, int64_t B, int L, int64_t n_nodes, int32_t* status, const Ragged& r, hipStream_t st, int level,
                       int64_t* node_ids, int32_t* node_cnt, float* node_zero, PlanDeferred* defer, bool packed, const float* y, const float* w) {
  if (defer) defer->pending = false;
  MATCHA_CHECK_ARG(!packed || (ragged_plan_packs(B, r) && level <= 1), "launch_ragged_plan: the packed order needs the five-launch plan at level <= 1");
  // The packed order needs no larger lists.  halves_cap and super_hcap rest on ONE invariant of tile_pack_wave, which holds for any row order: a
  // half tile closes only when the next row (<= L tokens) does not fit, so every tile but a superblock's last holds > kHalfTok - L tokens, and a
  // superblock is still the rows whose first token lies in a window of kSuperTok tokens.  What the host can check is that `r` was carved with
  // exactly those caps for this batch (tests/test_cpu_row_pack.py holds the twin's lists to the same two bounds)
  static_assert(kHalfTok == 31 && MATCHA_MAX_L < kHalfTok, "halves_cap / super_hcap: a row always fits an empty half tile");
  MATCHA_CHECK_ARG(!packed || (r.nsb == super_blocks(B * L) && r.sb_hcap == super_hcap(L) && r.nhalves == halves_cap(B * L, L)),
                   "launch_ragged_plan: the plan was not carved for B=%lld L=%d", (long long)B, L);
  if (B <= kSmallRows && r.nsb <= kSmallSb && !options().disable_small_batch) {
    PlanSmallArgs a;
    a.x = x; a.B = B; a.L = L; a.n_nodes = n_nodes; a.status = status;
    a.row_off = r.row_off; a.tok_slot = r.tok_slot; a.tok_id = r.tok_id; a.tok_pos = r.tok_pos; a.tok_key = r.tok_key; a.count = r.count; a.sb_first = r.sb_first;
    a.nsb = r.nsb; a.level = level;
    a.sb_tiles[0] = r.sb_tiles; a.cap_per_sb[0] = r.sb_cap; a.ntiles_cap[0] = r.ntiles; a.meta[0] = r.tile_meta;
    a.sb_tiles[1] = r.sb_htiles; a.cap_per_sb[1] = r.sb_hcap; a.ntiles_cap[1] = r.nhalves; a.meta[1] = r.half_meta;
    a.tok_tile = r.tok_tile;
    a.node_ids = node_ids; a.node_cnt = node_cnt; a.node_zero = node_zero;
    hipLaunchKernelGGL(plan_small_kernel, dim3(1), dim3(1024), 0, st, a);
    MATCHA_CHECK_LAUNCH("plan_small_kernel");
    return MATCHA_OK;
  }
  hipLaunchKernelGGL(row_count_kernel, dim3(r.nblk), dim3(256), 0, st, x, B, L, r.blk_sum, packed ? r.cls_hist : nullptr);
  MATCHA_CHECK_LAUNCH("row_count_kernel");
  hipLaunchKernelGGL(row_scan_kernel, dim3(1), dim3(1024), 0, st, r.blk_sum, r.nblk, r.count, r.sb_first, r.nsb, (int32_t)B, packed ? r.cls_hist : nullptr,
                     packed ? r.sched : nullptr);
  MATCHA_CHECK_LAUNCH("row_scan_kernel");
  if (packed)
    hipLaunchKernelGGL(row_fill_kernel<true>, dim3(r.nblk), dim3(256), 0, st, x, B, L, r.blk_sum, r.count, r.row_off, r.tok_slot, r.tok_id, r.tok_pos, r.sb_first, kSuperTok,
                       r.tok_key, n_nodes, status, node_ids, node_cnt, node_zero, r.cls_hist, r.sched, r.row_src, y, w, r.y_plan, r.w_plan);
  else
    hipLaunchKernelGGL(row_fill_kernel<false>, dim3(r.nblk), dim3(256), 0, st, x, B, L, r.blk_sum, r.count, r.row_off, r.tok_slot, r.tok_id, r.tok_pos, r.sb_first, kSuperTok,
                       r.tok_key, n_nodes, status, node_ids, node_cnt, node_zero, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  MATCHA_CHECK_LAUNCH("row_fill_kernel");
  if (level <= 0) return MATCHA_OK;
  const int first = level >= 2 ? 0 : 1;                // list 0: 64-row tiles, list 1: half tiles
  TilePackArgs pa;
  pa.row_off = r.row_off; pa.B = B; pa.nsb = r.nsb; pa.sb_first = r.sb_first; pa.first = first; pa.ntasks = r.nsb * (2 - first);
  pa.cap_per_sb[0] = r.sb_cap; pa.sb_tiles[0] = r.sb_tiles; pa.sb_cnt[0] = r.sb_cnt;
  pa.cap_per_sb[1] = r.sb_hcap; pa.sb_tiles[1] = r.sb_htiles; pa.sb_cnt[1] = r.sb_hcnt;
  CompactArgs ca;
  ca.sb_tiles[0] = r.sb_tiles; ca.sb_cnt[0] = r.sb_cnt; ca.cap_per_sb[0] = r.sb_cap; ca.ntiles_cap[0] = r.ntiles; ca.meta[0] = r.tile_meta;
  ca.sb_tiles[1] = r.sb_htiles; ca.sb_cnt[1] = r.sb_hcnt; ca.cap_per_sb[1] = r.sb_hcap; ca.ntiles_cap[1] = r.nhalves; ca.meta[1] = r.half_meta;
  ca.nsb = r.nsb; ca.count = r.count; ca.first = first;
  if (defer && level == 1) {
    defer->pending = true; defer->pack = pa; defer->compact = ca;
    return MATCHA_OK;
  }
  MATCHA_TRY(launch_tile_pack(pa, st));
  MATCHA_TRY(launch_tile_compact(ca, st));
  if (level >= 2) {
    hipLaunchKernelGGL(tok_tile_kernel, dim3(r.ntiles), dim3(64), 0, st, r.tile_meta, r.tok_tile);
    MATCHA_CHECK_LAUNCH("tok_tile_kernel");
  }
  return MATCHA_OK;
}

}  // namespace matcha

using namespace matcha;

extern "C" size_t matcha_ragged_plan_bytes(int64_t B, int32_t L) {
  if (B < 1 || L < 1 || L > MATCHA_MAX_L || B * (int64_t)L >= (1ll << 31) - 2) return 0;
  return ragged_bytes(B, L);
}

extern "C" int matcha_ragged_plan(const int64_t* x, int64_t B, int32_t L, int32_t n_nodes, int32_t* status, void* ws, size_t ws_bytes,
                                  matcha_ragged_view* view, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(x && ws && view, "matcha_ragged_plan: null pointer");
  MATCHA_CHECK_ARG(B >= 1 && L >= 1 && L <= MATCHA_MAX_L && B * (int64_t)L < (1ll << 31) - 2, "matcha_ragged_plan: B=%lld L=%d", (long long)B, L);
  MATCHA_CHECK_ARG(n_nodes >= 1, "matcha_ragged_plan: n_nodes=%d", n_nodes);
  MATCHA_CHECK_ARG(((uintptr_t)ws) % 256 == 0, "matcha_ragged_plan: workspace must be 256-byte aligned");
  if (ws_bytes < ragged_bytes(B, L)) { set_error("matcha_ragged_plan: workspace %zu < %zu bytes", ws_bytes, ragged_bytes(B, L)); return MATCHA_ENOMEM; }
  Ragged r;
  ragged_carve(B, L, (char*)ws, r);
  view->row_off = r.row_off; view->tok_slot = r.tok_slot; view->tok_id = r.tok_id; view->tok_key = r.tok_key; view->tok_pos = r.tok_pos;
  view->count = r.count; view->tile_meta = r.tile_meta; view->tiles_cap = r.ntiles;
  view->half_meta = r.half_meta; view->halves_cap = r.nhalves; view->tok_tile = r.tok_tile;
  return launch_ragged_plan(x, B, L, n_nodes, status, r, (hipStream_t)stream, 2);
}
