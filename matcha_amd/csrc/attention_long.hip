// Per-hyperedge multi-head self-attention for LONG rows: k <= L <= MATCHA_MAX_LONG_L = 32 real tokens, forward only, on the ragged token
// layout (attention.hip / attention_wide.hip hold L <= 8 rows of all eight heads in one wavefront's registers).
//
// At k <= 32 a head's score matrix is ONE 32 x 32 tile, i.e. one accumulator of v_mfma_f32_32x32x2_f32 (16 VGPRs; exact f32 products in an
// f32 fma chain, so the fp32 grade holds without any plane splitting).  One wavefront owns one (hyperedge, head); the eight wavefronts of a
// workgroup are the eight heads of one hyperedge, so with the merged heads' shared key / value rows the rows one head pulls in are cache
// hits for the other seven.  An all-padding hyperedge leaves at once: the work follows the real tokens, not B L.
//
// The tile is computed TRANSPOSED, S^T[j][i] = K_j . Q_i (A operand: key rows, B operand: query rows).  In the accumulator layout lane
// (r = lane & 31, h = lane >> 5) then holds QUERY i = r and the sixteen KEYS j = 8 (v >> 2) + 4 h + (v & 3), v = 0..15: the softmax of a
// query is a reduction over a lane's own registers plus ONE exchange with lane ^ 32, and register v of the probabilities is, as it stands,
// the A operand of step v of  O[i][f] = sum_j P[i][j] V[j][f]  (the step's two k slots are the keys j_v and j_v + 4 of the two lane
// halves), whose B operand is 32 consecutive features of those two value rows -- one coalesced 128-byte load per half -- and whose result
// leaves 32 consecutive features of a query in the 32 lanes of a half: whole-line stores.  Steps whose keys all lie behind the row's last
// column are skipped; a tile's sixteen value loads are issued together in front of its steps.  One operand set is live at a time (the score
// accumulator with four float4 pairs in flight, then probabilities, sixteen values and the output tile: 124 VGPRs, no scratch), whatever embed_dim.
//
// Semantics as attention.hip:9-15: only the diagonal is masked (probability exactly 0); the n_pad = L - k padding slots all carry the
// shared padding token's K / V row (token index Tr) and enter as ONE extra key column j = k with multiplicity n_pad -- denominator
// += n_pad exp(s_pad), output += n_pad P_pad V_pad; padding queries are not evaluated; k = 1 attends the padding slots only; k = L has
// no padding column (k = 32 fills the tile, and then n_pad = 0).
#include "attention_long.hpp"

namespace matcha {

namespace {
constexpr int kProbStride = 33;              // row stride of a wavefront's probability tile in LDS (floats)

// the writes of some lanes of a wavefront to its private LDS tile, read by other lanes of the SAME wavefront: LDS serves one wavefront's
// instructions in order, so only the compiler has to keep the order (as attention_long_bwd.hip)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
}  // namespace

// Q / O rows are [T, 8 d]; O may be the same buffer as Q (a wavefront reads its (hyperedge, head) slice of Q completely before it writes
// the same slice of O, and no other wavefront touches that slice), hence no __restrict__ on them
// (waves_per_eu 4: the register budget of four wavefronts per SIMD, 128; left alone the allocator takes 133 and the occupancy drops to three)
//
// Two instances of one text.  attn_long_kernel<false> is "attn_long_kernel" in the launch log, the forward of model(x) and of training (mask
// and attn unused: its instructions are those of the kernel before it was a template, 124 VGPRs, no LDS).  attn_long_kernel<true> is
// "attn_long_prob_kernel", the instance behind Classifier.get_embedding (126 VGPRs, 33 KB of LDS, no scratch: still four wavefronts per SIMD,
// i.e. two workgroups per CU): the same tile, softmax and O = P V on the same operands -- the same O bits --, and between the softmax and the
// products it writes the probabilities of its (hyperedge b, head) as block (head B + b) of L L floats of `attn`, the reference's [8 B, L, L]:
// row = query slot, column = key slot, both as they stand in x.  EVERY element of the block is written -- a real query's real keys from the
// compact tile (compact index = rank of the slot in the row's real-column set mask[b], the plan's), every padding key slot the padding
// column's probability WITHOUT its multiplicity (one value per query, so the padding slots of a query hold the same bits), the diagonal 0 (the
// softmax's), a padding query's row 0, a k = 0 hyperedge's block 0 -- so the caller's tensor needs no memset and nothing runs behind the kernel.
// Store pattern: in the accumulator layout a lane holds one query and sixteen keys, so a direct store would put the 32 lanes of a half on 32
// different rows of the block (L floats apart: a 4-byte piece of up to 32 lines per instruction) and would need a second pass for the padding
// slots and rows.  Instead the wavefront's compact tile goes through its own 32 x 33 floats of LDS (33: the 32 queries of a half land in 32
// banks) and the lanes then walk the block as it lies in memory, 64 consecutive floats per store instruction, looking their slot's compact
// (row, column) up with two popcounts.  The tile is the wavefront's own: the ordering point is wave-local, no workgroup barrier.
template <bool PROB>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_long_kernel(
    const float* Q, const float* __restrict__ K, const float* __restrict__ V, const int32_t* __restrict__ row_off, int64_t B, int L, int d,
    int64_t kv_ld, int kv_head, float inv_temp, float* O, const uint32_t* __restrict__ mask, float* __restrict__ attn) {
  const int lane = threadIdx.x & 63, head = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t b = blockIdx.x;
  const int t0 = row_off[b];
  const int k = row_off[b + 1] - t0;              // real tokens of this hyperedge (wave-uniform)
  if (k <= 0) {
    if (PROB) {                                   // no token, no query: the whole block is zero
      float* blk = attn + ((int64_t)head * B + b) * (L * L);
      for (int e = lane; e < L * L; e += 64) blk[e] = 0.f;
    }
    return;
  }
  const int64_t tp = row_off[B];                  // the shared padding token
  const int n_pad = L - k;
  const int64_t hd = (int64_t)MATCHA_N_HEAD * d;
  // tile row r as a key / as a query: real token r, else the padding token (column k when n_pad > 0; behind it rows nobody weighs)
  const int64_t trow = r < k ? (int64_t)t0 + r : tp;

  // ---- S^T = K Q^T and the softmax of query i = r over its keys (attention_long.hpp: shared with the backward kernel, which recomputes the same bits)
  float p[16];
  {
    const float4* kp = reinterpret_cast<const float4*>(K + trow * kv_ld + (int64_t)head * kv_head) + h;
    const float4* qp = reinterpret_cast<const float4*>(Q + trow * hd + (int64_t)head * d) + h;
    const f32x16 acc = long_tile_nt(kp, qp, d / 8);
    long_softmax(acc, k, n_pad, r, h, inv_temp, p);
  }

  if (PROB) {
    __shared__ float tiles[MATCHA_N_HEAD * 32 * kProbStride];
    float* tile = tiles + head * (32 * kProbStride);
    // compact tile -> LDS, tile[i][j] at i 33 + j: columns 0 .. k (k: the padding column, divided by its multiplicity; only read when n_pad > 0,
    // and k = 32 has none), rows of queries i >= k are never read
    const float inv_pad = 1.f / (float)(n_pad > 0 ? n_pad : 1);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int j = 8 * (v >> 2) + 4 * h + (v & 3);
      tile[r * kProbStride + j] = j == k ? p[v] * inv_pad : p[v];
    }
    wave_lds_sync();
    const uint32_t m = mask[b];
    float* blk = attn + ((int64_t)head * B + b) * (L * L);
    const uint32_t magic = (65536u + (uint32_t)L - 1u) / (uint32_t)L;      // e / L = e magic >> 16 for e < 1024, L <= 32
    for (int e = lane; e < L * L; e += 64) {
      const uint32_t li = ((uint32_t)e * magic) >> 16, lj = (uint32_t)e - li * (uint32_t)L;
      const bool qreal = (m >> li) & 1u, kreal = (m >> lj) & 1u;
      const int ci = __popc(m & ((1u << li) - 1u));
      const int cj = kreal ? __popc(m & ((1u << lj) - 1u)) : k;
      const float t = tile[(qreal ? ci : 0) * kProbStride + cj];
      blk[e] = qreal ? t : 0.f;
    }
  }

  // ---- O = P V, 32 features at a time: A operand = the probabilities as they stand (lane = query), B operand = 32 consecutive features of the
  // step's two value rows (one 128-byte line per lane half); in the result lane r holds feature f0 + r of the sixteen queries
  // i = 8 (v >> 2) + 4 h + (v & 3), so every store instruction writes whole 128-byte lines of two rows
  // (addresses: one 64-bit base per tile for the hyperedge's rows and one for the padding token's, 32-bit offsets j kv_ld / i 8 d below them)
  const float* vrows = V + (int64_t)t0 * kv_ld + (int64_t)head * kv_head;
  const float* vpad = V + tp * kv_ld + (int64_t)head * kv_head;
  float* obase = O + (int64_t)t0 * hd + (int64_t)head * d;
  const uint32_t kvs = (uint32_t)kv_ld, os = (uint32_t)hd;
  for (int f0 = 0; f0 < d; f0 += 32) {
    const bool fon = f0 + r < d;                  // (d = 8 .. 24, 40, 48, 56: the tile's last features do not exist; computed on a clamped address, not stored)
    const int f = fon ? f0 + r : d - 1;
    const float* vf = vrows + f;
    const float* vpf = vpad + f;
    // the tile's sixteen value loads first, on addresses that are valid whatever k (a clamp, no branch), so that all of them are in flight
    // together: with the load inside the step's branch every step waited for its own round trip (32 in a row per wavefront at d = 64)
    // (a key behind the row reads the row's last token -- finite, weight 0 --, the padding column the padding token's value: one base, 32-bit offsets)
    float b[16];
    const float bpad = *vpf;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int j = 8 * (v >> 2) + 4 * h + (v & 3);
      b[v] = vf[(uint32_t)(j < k ? j : k - 1) * kvs];
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) b[v] = (8 * (v >> 2) + 4 * h + (v & 3)) == k ? bpad : b[v];
    f32x16 o = {0};
#pragma unroll
    for (int v = 0; v < 16; ++v)
      if (8 * (v >> 2) + (v & 3) <= k)            // wave-uniform: the step's first key is inside the row (or its padding column)
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(p[v], b[v], o, 0, 0, 0);
    float* of = obase + f;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int i = 8 * (v >> 2) + 4 * h + (v & 3);
      if (i < k && fon) of[(uint32_t)i * os] = o[v];
    }
  }
}

int launch_attn_long(const float* Q, const float* K, const float* V, const int32_t* row_off, int64_t B, int L, int d, int64_t kv_ld, int kv_head,
                     float* O, hipStream_t st, const uint32_t* mask, float* attn) {
  if (B <= 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(L >= 1 && L <= MATCHA_MAX_LONG_L && d >= 8 && d % 8 == 0 && B < (1ll << 31), "attn_long: B=%lld L=%d d=%d", (long long)B, L, d);
  MATCHA_CHECK_ARG(!attn || mask, "attn_long: probabilities without the plan's column sets");
  const float inv_temp = 1.0f / sqrtf((float)d);
  if (attn) {
    hipLaunchKernelGGL(attn_long_kernel<true>, dim3((unsigned)B), dim3(512), 0, st, Q, K, V, row_off, B, L, d, kv_ld, kv_head, inv_temp, O, mask, attn);
    MATCHA_CHECK_LAUNCH("attn_long_prob_kernel");
    return MATCHA_OK;
  }
  hipLaunchKernelGGL(attn_long_kernel<false>, dim3((unsigned)B), dim3(512), 0, st, Q, K, V, row_off, B, L, d, kv_ld, kv_head, inv_temp, O, mask, attn);
  MATCHA_CHECK_LAUNCH("attn_long_kernel");
  return MATCHA_OK;
}

}  // namespace matcha
