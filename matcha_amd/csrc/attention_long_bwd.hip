// Backward of the per-hyperedge multi-head self-attention for LONG rows (attention_long.hip): k <= L <= MATCHA_MAX_LONG_L = 32 real tokens.
//
// Ownership as in the forward: one wavefront per (hyperedge, head), the eight wavefronts of a workgroup are the eight heads of one hyperedge,
// a k = 0 hyperedge is passed over at once, every tile product on v_mfma_f32_32x32x2_f32 (exact f32 products in an f32 fma chain).  A fixed
// number of workgroups walks the hyperedges with a grid stride, so the slab space of the padding token's rows is bounded.
//
// Mathematics as attention.hip:185-191 (real i, j < k; the n_pad = L - k padding slots are ONE key column j = k with multiplicity n_pad; only
// the diagonal is masked; padding queries are not evaluated).  The probabilities are recomputed from Q and K by the forward's own functions
// (attention_long.hpp), with the multiplicity in the padding column: p_ik = n_pad Pp_i.  Then, per (hyperedge, head), with lane (r, h) = query
// i = r and register v = key j = long_tile_row(v, h) ("query layout", the forward's):
//   dP^T = V dO^T             the score product with V for K and dO for Q: dP_ij in the layout of p_ij, dPp_i in column k
//   sig_i = sum_j p_ij dP_ij  over the lane's registers + one exchange with lane ^ 32 (the padding column carries its n_pad)
//   ds_ij = p_ij (dP_ij - sig_i) / temp          (column k: n_pad dSp_i);  rows i >= k of p and ds are zeroed: they are no queries
//   dQ = ds K                 the forward's O = P V with ds for P and K for V: register v of ds is the A operand of step v as it stands
// and, with p and ds TRANSPOSED through a wave-private LDS tile (lane = key j, register = query i: "key layout"),
//   dV = p^T dO,  dK = ds^T Q the same product shape, B operand = 32 consecutive features of the step's two QUERY rows;  row j = k of the
//                             two results is this hyperedge's share of the padding token's dV / dK row (n_pad included).
// The padding token's rows collect in a wave-private LDS vector per head over the workgroup's walk and leave as ONE slab per workgroup,
// {dK_pad [8 d], dV_pad [8 d]}; attn_long_pad_reduce_kernel adds the slabs in a fixed order.  No float atomics: every output is the same
// bits from run to run.
//
// Two operand forms, as launch_attn_long: per-head K / V [T, 8 d] (dK / dV [T, 8 d], each wave stores its own tile), and the merged heads'
// shared rows kin / vin [T, d]: there the eight waves put their dV (then dK) tile into an LDS stage and the workgroup adds the eight in head order, one writer per element of a real token row: d kin / d vin [T, d].
//
// Addresses are valid for every k in 1..32 and n_pad in 0..31 by clamps, not branches: tile row r >= k reads the padding token's row (index
// row_off[B], which always exists), a key / query behind the row reads the row's last token with weight exactly 0.
#include "attention_long.hpp"

namespace matcha {

namespace {
constexpr int kLongBwdGrid = 512;            // workgroups of the walk (two per CU of an MI355X): the slab space is this many x 2 x 8 d floats
constexpr int kTStride = 36;                 // row stride of a transposing tile (floats): 16-byte aligned rows, 32 + 4 against bank conflicts
constexpr int kTFloats = 32 * kTStride;      // one wave's transposing tile

// the writes of some lanes of a wavefront to its private LDS tile, read by other lanes of the SAME wavefront: LDS serves one wavefront's
// instructions in order, so only the compiler has to keep the order
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// D[a][f] = sum_c w[register of c] rows[c][f] for 32 features (lane r: feature column f): the forward's O = P V.  Step v contracts the tile rows
// c = long_tile_row(v, 0) and c + 4 (the two lane halves); a step whose first row lies behind `last` is skipped (wave-uniform).  Row c reads
// rows[min(c, clamp) * stride + f] -- `rows` is wave-uniform, the offset 32 bits: one register per address --; with pad_at >= 0 row c == pad_at
// takes bpad instead (the padding token's row).
__device__ __forceinline__ f32x16 long_tile_wv(const float (&w)[16], const float* rows, uint32_t stride, uint32_t f, int h, int clamp, int last,
                                               int pad_at, float bpad) {
  float b[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int c = long_tile_row(v, h);
    b[v] = rows[(uint32_t)(c < clamp ? c : clamp) * stride + f];
  }
#pragma unroll
  for (int v = 0; v < 16; ++v) b[v] = long_tile_row(v, h) == pad_at ? bpad : b[v];
  f32x16 o = {0};
#pragma unroll
  for (int v = 0; v < 16; ++v)
    if (long_tile_row(v, 0) <= last) o = __builtin_amdgcn_mfma_f32_32x32x2f32(w[v], b[v], o, 0, 0, 0);
  return o;
}
}  // namespace

// K / V rows: stride kv_ld, per-head offset kv_head (8 d and d per head; d and 0 for the merged heads' shared rows).  dK / dV have the layout of
// K / V: per head [T, 8 d], or with `merged` the sums over the heads [T, d].  Dynamic LDS: 8 transposing tiles (+ merged: the stage) + 8 x [2][d] padding-row sums.
template <bool merged>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_long_bwd_kernel(
    const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V, const float* __restrict__ dO,
    const int32_t* __restrict__ row_off, int64_t B, int L, int d, int64_t kv_ld, int kv_head, float inv_temp,
    float* __restrict__ dQ, float* __restrict__ dK, float* __restrict__ dV, float* __restrict__ slab) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63;
  const int head = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave-uniform, and known to be: the head's base addresses stay scalar
  const int r = lane & 31, h = lane >> 5;
  float* tile = lds + head * kTFloats;                       // wave-private transposing tile
  float* stage = lds + MATCHA_N_HEAD * kTFloats;             // merged: the eight heads' output tiles [8][32][32], between barriers
  float* padacc = lds + MATCHA_N_HEAD * kTFloats + (merged ? MATCHA_N_HEAD * 1024 : 0) + head * 2 * d;    // wave-private: this head's dK_pad [d], dV_pad [d] over the workgroup's walk
  for (int f = lane; f < 2 * d; f += 64) padacc[f] = 0.f;
  wave_lds_sync();
  const int64_t tp = row_off[B];                             // the shared padding token
  const int64_t hd = (int64_t)MATCHA_N_HEAD * d;
  const uint32_t kvs = (uint32_t)kv_ld, qs = (uint32_t)hd;

  const int nb = (int)B;                                     // (B < 2^31: the launcher)
  for (int b = blockIdx.x; b < nb; b += gridDim.x) {
    const int t0 = row_off[b];
    const int k = row_off[b + 1] - t0;                       // real tokens of this hyperedge (uniform over the workgroup)
    if (k <= 0) continue;
    const int n_pad = L - k;
    const int64_t trow = r < k ? (int64_t)t0 + r : tp;       // tile row r as a key / as a query: real token r, else the padding token
    const int last = k - 1;

    // ---- p (the forward's bits) and ds in the query layout
    float p[16], ds[16];
    {
      const float4* kp = reinterpret_cast<const float4*>(K + (int64_t)head * kv_head + (trow * kv_ld + 4 * h));
      const float4* qp = reinterpret_cast<const float4*>(Q + (int64_t)head * d + (trow * hd + 4 * h));
      const f32x16 acc = long_tile_nt(kp, qp, d / 8);
      long_softmax(acc, k, n_pad, r, h, inv_temp, p);
    }
    {
      const float4* vp = reinterpret_cast<const float4*>(V + (int64_t)head * kv_head + (trow * kv_ld + 4 * h));
      const float4* gp = reinterpret_cast<const float4*>(dO + (int64_t)head * d + (trow * hd + 4 * h));
      const f32x16 dp = long_tile_nt(vp, gp, d / 8);         // dP_ij = dO_i . V_j, column k: dO_i . V_pad
      const bool query = r < k;
      float sig = 0.f;
#pragma unroll
      for (int v = 0; v < 16; ++v) { p[v] = query ? p[v] : 0.f; sig += p[v] * dp[v]; }
      sig += __shfl_xor(sig, 32, kWave);
#pragma unroll
      for (int v = 0; v < 16; ++v) ds[v] = query ? p[v] * (dp[v] - sig) * inv_temp : 0.f;
    }

    // p goes into the wave's tile at once (transposed): only ds stays in registers for dQ
#pragma unroll
    for (int v = 0; v < 16; ++v) tile[long_tile_row(v, h) * kTStride + r] = p[v];

    // ---- dQ = ds K, 32 features at a time (the forward's O = P V): keys 0 .. k - 1 and the padding column k
    {
      const float* krows = K + (int64_t)t0 * kv_ld + (int64_t)head * kv_head;
      const float* kpad = K + tp * kv_ld + (int64_t)head * kv_head;
      float* qbase = dQ + (int64_t)t0 * hd + (int64_t)head * d;
      for (int f0 = 0; f0 < d; f0 += 32) {
        const bool fon = f0 + r < d;
        const uint32_t f = fon ? f0 + r : d - 1;
        const f32x16 o = long_tile_wv(ds, krows, kvs, f, h, last, k, k, kpad[f]);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int i = long_tile_row(v, h);
          if (i < k && fon) qbase[(uint32_t)i * qs + f] = o[v];
        }
      }
    }

    // ---- key layout (lane = key j, registers = queries i): p^T out of the tile, ds into it -- one of the two in registers at a time
    auto read_tile = [&](float (&x)[16]) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 t = *reinterpret_cast<const float4*>(tile + r * kTStride + 8 * g + 4 * h);
        x[4 * g] = t.x; x[4 * g + 1] = t.y; x[4 * g + 2] = t.z; x[4 * g + 3] = t.w;
      }
    };
    wave_lds_sync();
    read_tile(p);
    wave_lds_sync();
#pragma unroll
    for (int v = 0; v < 16; ++v) tile[long_tile_row(v, h) * kTStride + r] = ds[v];

    // ---- dV = p^T dO, then dK = ds^T Q: rows j < k are token rows, row j = k (n_pad > 0) the padding token's share
    auto tiles = [&](const float (&w)[16], const float* src, float* out, float* pacc) {
      const float* rows = src + (int64_t)t0 * hd + (int64_t)head * d;
      float* obase = out + (int64_t)t0 * kv_ld + (int64_t)head * kv_head;
      for (int f0 = 0; f0 < d; f0 += 32) {
        const bool fon = f0 + r < d;
        const uint32_t f = fon ? f0 + r : d - 1;
        const f32x16 o = long_tile_wv(w, rows, qs, f, h, last, last, -1, 0.f);
#pragma unroll
        for (int v = 0; v < 16; ++v)
          if (long_tile_row(v, h) == k && n_pad > 0 && fon) pacc[f] += o[v];
        if (!merged) {
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const int j = long_tile_row(v, h);
            if (j < k && fon) obase[(uint32_t)j * kvs + f] = o[v];
          }
        } else {
#pragma unroll
          for (int v = 0; v < 16; ++v) stage[head * 1024 + long_tile_row(v, h) * 32 + r] = o[v];
          __syncthreads();
          int e0 = threadIdx.x;
          asm volatile("" : "+v"(e0));      // (keeps the element's address arithmetic here: hoisted out of the hyperedge loop it costs the registers that spill)
          for (int e = e0; e < 1024; e += 512) {
            const int j = e >> 5, fc = f0 + (e & 31);
            if (j < k && fc < d) {
              float s = stage[e];
#pragma unroll
              for (int w2 = 1; w2 < MATCHA_N_HEAD; ++w2) s += stage[w2 * 1024 + e];
              obase[(uint32_t)j * kvs + (uint32_t)fc] = s;      // (merged: kv_head = 0, obase is the hyperedge's first row of the head sums)
            }
          }
          __syncthreads();
        }
      }
    };
    tiles(p, dO, dV, padacc + d);
    wave_lds_sync();
    read_tile(ds);
    tiles(ds, Q, dK, padacc);
    wave_lds_sync();
  }

  // the workgroup's slab: {dK_pad [8 d], dV_pad [8 d]}, every head its own part
  wave_lds_sync();
  float* sl = slab + (int64_t)blockIdx.x * 2 * hd + (int64_t)head * d;
  for (int f = lane; f < d; f += 64) { sl[f] = padacc[f]; sl[hd + f] = padacc[d + f]; }
}

// The padding token's rows: dK[Tr] / dV[Tr] = the slabs added in block order (merged: then the heads in head order, into d kin / d vin [T, d]);
// dQ[Tr] = 0.  One block per 64 features of {dK, dV}, one wavefront per head.
__global__ __launch_bounds__(512) void attn_long_pad_reduce_kernel(const float* __restrict__ slab, int nblk, int d, int merged,
                                                                   const int32_t* __restrict__ row_off, int64_t B, float* __restrict__ dQ,
                                                                   float* __restrict__ dK, float* __restrict__ dV) {
  __shared__ float part[MATCHA_N_HEAD][64];
  const int o = threadIdx.x & 63, head = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + o;                          // index in [0, 2 d)
  const int64_t hd = (int64_t)MATCHA_N_HEAD * d;
  const int64_t tr = row_off[B];
  const bool on = i < 2 * d;
  const int which = on ? i / d : 0, f = on ? i - which * d : 0;
  float s0 = 0.f, s1 = 0.f;
  if (on) {
    const float* src = slab + (int64_t)which * hd + (int64_t)head * d + f;
    int p = 0;
    for (; p + 1 < nblk; p += 2) { s0 += src[(int64_t)p * 2 * hd]; s1 += src[(int64_t)(p + 1) * 2 * hd]; }
    if (p < nblk) s0 += src[(int64_t)p * 2 * hd];
  }
  const float s = s0 + s1;
  if (on && which == 0) dQ[tr * hd + (int64_t)head * d + f] = 0.f;
  if (!merged) {
    if (on) (which == 0 ? dK : dV)[tr * hd + (int64_t)head * d + f] = s;
    return;
  }
  part[head][o] = s;
  __syncthreads();
  if (head == 0 && on) {
    float t = part[0][o];
#pragma unroll
    for (int w = 1; w < MATCHA_N_HEAD; ++w) t += part[w][o];
    (which == 0 ? dK : dV)[tr * d + f] = t;
  }
}

static int attn_long_bwd_blocks(int64_t B) { return (int)(B < kLongBwdGrid ? B : kLongBwdGrid); }
size_t attn_long_bwd_slab_bytes(int64_t B, int d) {
  return align_up((size_t)(B < 1 ? 1 : attn_long_bwd_blocks(B)) * 2 * MATCHA_N_HEAD * d * sizeof(float), 256);
}

int launch_attn_long_bwd(const float* Q, const float* K, const float* V, const float* dO, const int32_t* row_off, int64_t B, int L, int d,
                         int64_t kv_ld, int kv_head, float* dQ, float* dK, float* dV, float* slab, hipStream_t st) {
  if (B <= 0) return MATCHA_OK;
  MATCHA_CHECK_ARG(L >= 1 && L <= MATCHA_MAX_LONG_L && d >= 8 && d % 8 == 0 && d <= 256 && B < (1ll << 31), "attn_long_bwd: B=%lld L=%d d=%d",
                   (long long)B, L, d);
  const int64_t hd = (int64_t)MATCHA_N_HEAD * d;
  const bool merged = kv_head == 0 && kv_ld == d;
  MATCHA_CHECK_ARG(merged || (kv_head == d && kv_ld == hd), "attn_long_bwd: kv_ld=%lld kv_head=%d is neither operand form", (long long)kv_ld, kv_head);
  const float inv_temp = 1.0f / sqrtf((float)d);
  const int nblk = attn_long_bwd_blocks(B);
  // 36 864 + 64 d bytes, + 32 768 with the merged heads' stage: two workgroups per CU up to embed_dim 128 there, one at 192 and 256
  const size_t lds = ((size_t)MATCHA_N_HEAD * kTFloats + (merged ? (size_t)MATCHA_N_HEAD * 1024 : 0) + (size_t)MATCHA_N_HEAD * 2 * d) * sizeof(float);
  static bool big_lds = false;
  if (merged && !big_lds) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attn_long_bwd_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    big_lds = true;
  }
  if (merged) hipLaunchKernelGGL(attn_long_bwd_kernel<true>, dim3((unsigned)nblk), dim3(512), lds, st, Q, K, V, dO, row_off, B, L, d, kv_ld, kv_head, inv_temp, dQ, dK, dV, slab);
  else hipLaunchKernelGGL(attn_long_bwd_kernel<false>, dim3((unsigned)nblk), dim3(512), lds, st, Q, K, V, dO, row_off, B, L, d, kv_ld, kv_head, inv_temp, dQ, dK, dV, slab);
  MATCHA_CHECK_LAUNCH("attn_long_bwd_kernel");
  hipLaunchKernelGGL(attn_long_pad_reduce_kernel, dim3((unsigned)cdiv(2 * d, 64)), dim3(512), 0, st, slab, nblk, d, merged ? 1 : 0, row_off, B, dQ, dK, dV);
  MATCHA_CHECK_LAUNCH("attn_long_pad_reduce_kernel");
  return MATCHA_OK;
}

}  // namespace matcha

using namespace matcha;

extern "C" size_t matcha_attn_long_bwd_workspace_bytes(int64_t B, int32_t d) {
  if (B < 0 || d < 8 || d > 256 || d % 8 != 0) { set_error("matcha_attn_long_bwd_workspace_bytes: B=%lld d=%d", (long long)B, (int)d); return 0; }
  return attn_long_bwd_slab_bytes(B, d);
}

extern "C" int matcha_attn_long_bwd(const float* Q, const float* K, const float* V, const float* dO, const int32_t* row_off, int64_t B, int32_t L,
                                    int32_t d, int32_t shared_kv, float* dQ, float* dK, float* dV, void* ws, size_t ws_bytes,
                                    matcha_stream_t stream) {
  MATCHA_CHECK_ARG(Q && K && V && dO && dQ && dK && dV && row_off && ws, "matcha_attn_long_bwd: null pointer");
  MATCHA_CHECK_ARG(L >= 2 && L <= MATCHA_MAX_LONG_L, "matcha_attn_long_bwd: L=%d outside 2..%d", (int)L, MATCHA_MAX_LONG_L);
  MATCHA_CHECK_ARG(d >= 8 && d <= 256 && d % 8 == 0, "matcha_attn_long_bwd: d=%d unsupported (a multiple of 8 up to 256)", (int)d);
  MATCHA_CHECK_ARG(B >= 0 && B < (1ll << 31), "matcha_attn_long_bwd: B=%lld", (long long)B);
  MATCHA_CHECK_ARG(ws_bytes >= attn_long_bwd_slab_bytes(B, d), "matcha_attn_long_bwd: workspace too small");
  const int64_t hd = (int64_t)MATCHA_N_HEAD * d;
  return launch_attn_long_bwd(Q, K, V, dO, row_off, B, L, d, shared_kv ? d : hd, shared_kv ? 0 : d, dQ, dK, dV, (float*)ws, (hipStream_t)stream);
}
