// Denoised contact maps (Code/denoise_contact.py:147-207): one chromosome's post-processing of the pairwise sweep, bit for bit
// with the reference's numpy for the same probabilities and the same observed block.
//
//   1. denoise_assemble_kernel   P = proba2matrix(pairs, None, proba) and O = the same assembly of origin[i-1, j-1] (:162, :168):
//                                tile pairs (a, b) / (b, a) of 64 x 64, the upper tile read row by row (proba at the closed-form
//                                pair offset of row r, origin rows at stride ld), the lower tile written through LDS -- every
//                                read and write coalesced.  m + m.T is evaluated literally (p + 0, 0 + p, the diagonal p + p).
//   2. denoise_row_sums_kernel   np.mean(X, axis=-1) in numpy's order: the row is reduced in buffers of 8192 elements added in
//                                sequence, each buffer by numpy's pairwise sum (leaves of <= 128 with eight stride-8 accumulators
//                                and a sequential tail; the leaves combined in the recursion's order).  The tree is static for a
//                                given buffer length: the host builds it once (PwPlan) and passes it by value.
//   3. denoise_col_sums_kernel   np.mean(X, axis=0): one float32 chain per column over rows 0 .. n-1, one lane per column, 32
//                                rows of loads in flight.
//   4. denoise_combine_kernel    my_proba = P / c1 / c2, origin_part = O / c1 / c2, my = maximum(my_proba * origin_part, my_proba)
//                                (:163-178); my_proba is written with the gap rows / columns of O already zeroed (:187-188).
//   5. sums of my (2. and 3.), then denoise_finish_kernel: my / c1 / c2, gap rows / columns -> 0 (:179-186).
//   6. denoise_pixels_kernel     balanced = m[i - lo, j - lo] in pair order (:205-207), one row of pairs per block.
//
// The coverage of a sum s is sqrt(s / n) + 1e-15f: float32 division, float32 sqrt and float32 add, all correctly rounded (no
// contraction, no fast reciprocal), so every pre-quantile matrix equals numpy's.  No float atomics: every sum has one owner and a
// fixed order, so two runs are bitwise identical.  The quantile transforms (:190-192) are matcha_quantile_uniform, fitted on all n^2
// values (subsample=None): deliberate difference (a) of DESIGN.md 7.2, identical to scikit-learn's default up to n = 100.  A
// chromosome without pairs (n <= min_dis) is refused (b: the reference crashes there); container formats (c) are the Python side's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "kernels.hpp"

#pragma clang fp contract(off)

namespace matcha {
namespace {

constexpr int kTile = 64;              // assemble: 64 x 64 tiles, 256 threads
constexpr int kBuf = 8192;             // numpy's reduction buffer (NPY_BUFSIZE elements)
constexpr int kLeaf = 128;             // numpy's PW_BLOCKSIZE
constexpr int kMaxLeaves = kBuf / 64;  // a split node (> 128) has children >= 64, so a buffer has at most 128 leaves
constexpr int kMaxLevels = 8;          // split depth of a buffer of <= 8192 elements is <= 7
constexpr int kColAhead = 32;          // column sums: rows of loads in flight per lane

// Pairs of row r (chromosome-relative) = max(0, K - r) with K = max(0, n - min_dis); they start at off(r).
__host__ __device__ __forceinline__ int64_t pair_offset(int64_t r, int64_t K) {
  const int64_t rr = r < K ? r : K;
  return rr * K - rr * (rr - 1) / 2;
}

// numpy's pairwise-sum tree of one buffer: leaves in order, and the combines, deepest level first.  A node's value lives at the
// index of its leftmost leaf; combining a node adds its right child's value (at the right child's leftmost leaf) into it.
struct PwPlan {
  int32_t len, n_leaves, n_levels;
  uint16_t leaf_start[kMaxLeaves];
  uint8_t leaf_len[kMaxLeaves];        // 1 .. 128
  uint8_t level_end[kMaxLevels];       // cumulative combine counts per level
  uint8_t op_dst[kMaxLeaves], op_src[kMaxLeaves];
};

struct PwPlanBuilder {
  PwPlan* p;
  std::vector<std::vector<std::pair<int, int>>> ops;
  int build(int s, int L, int depth) {
    if (L <= kLeaf) {
      const int id = p->n_leaves++;
      p->leaf_start[id] = (uint16_t)s;
      p->leaf_len[id] = (uint8_t)L;
      return id;
    }
    int n2 = L / 2;
    n2 -= n2 % 8;
    const int a = build(s, n2, depth + 1);
    const int b = build(s + n2, L - n2, depth + 1);
    if ((int)ops.size() <= depth) ops.resize(depth + 1);
    ops[depth].push_back({a, b});
    return a;
  }
};

PwPlan make_pw_plan(int len) {
  PwPlan p{};
  p.len = len;
  PwPlanBuilder b{&p, {}};
  b.build(0, len, 0);
  int k = 0;
  for (int d = (int)b.ops.size() - 1; d >= 0; --d) {
    for (auto& o : b.ops[d]) { p.op_dst[k] = (uint8_t)o.first; p.op_src[k] = (uint8_t)o.second; ++k; }
    p.level_end[p.n_levels++] = (uint8_t)k;
  }
  return p;
}

// ---- 1. assembly --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void denoise_assemble_kernel(const float* __restrict__ proba, const float* __restrict__ origin, int64_t ld,
                                                               int32_t n, int32_t min_dis, float* __restrict__ P, float* __restrict__ O) {
  const int a = blockIdx.y, b = blockIdx.x;                            // tile pair (a, b) / (b, a), a <= b
  if (a > b) return;
  __shared__ float sp[kTile][kTile + 1];
  __shared__ float so[kTile][kTile + 1];
  const int tx = threadIdx.x % kTile, ty = threadIdx.x / kTile;
  const int64_t K = n > min_dis ? (int64_t)n - min_dis : 0;
  // m (before m + m.T): the upper band of tile (a, b), zero elsewhere
  for (int i = ty; i < kTile; i += 256 / kTile) {
    const int64_t r = (int64_t)a * kTile + i, c = (int64_t)b * kTile + tx;
    float p = 0.f, o = 0.f;
    if (r < n && c < n && c - r >= min_dis) {
      p = proba[pair_offset(r, K) + (c - r - min_dis)];
      o = origin[r * ld + c];
    }
    sp[i][tx] = p;
    so[i][tx] = o;
  }
  __syncthreads();
  // tile (a, b): m[r][c] + m[c][r]; m[c][r] is zero off the diagonal tile
  for (int i = ty; i < kTile; i += 256 / kTile) {
    const int64_t r = (int64_t)a * kTile + i, c = (int64_t)b * kTile + tx;
    if (r < n && c < n) {
      const float tp = a == b ? sp[tx][i] : 0.f, to = a == b ? so[tx][i] : 0.f;
      P[r * n + c] = sp[i][tx] + tp;
      O[r * n + c] = so[i][tx] + to;
    }
  }
  if (a == b) return;
  // tile (b, a): 0 + m[c][r]
  for (int i = ty; i < kTile; i += 256 / kTile) {
    const int64_t r = (int64_t)b * kTile + i, c = (int64_t)a * kTile + tx;
    if (r < n && c < n) {
      P[r * n + c] = 0.f + sp[tx][i];
      O[r * n + c] = 0.f + so[tx][i];
    }
  }
}

// ---- 2. row sums in numpy's pairwise order -> coverage denominators (and the row gap mask of O) ---------------------------------
struct RowSumArgs {
  const float* x[2];
  float* den[2];
  uint8_t* gap[2];                     // rows whose sum == 0 (nullptr: not wanted)
};

__global__ __launch_bounds__(256) void denoise_row_sums_kernel(RowSumArgs args, int32_t n, PwPlan full, PwPlan tail) {
  __shared__ float xs[kBuf];
  __shared__ float part[kMaxLeaves * 8];
  __shared__ float leaf[kMaxLeaves];
  const int mat = blockIdx.y;
  const int64_t r = blockIdx.x;
  const float* row = args.x[mat] + r * n;
  float total = 0.f;                                                   // the reduction's identity; buffers are added in sequence
  for (int c0 = 0; c0 < n; c0 += kBuf) {
    const PwPlan& pl = (n - c0 >= kBuf) ? full : tail;
    const int m = pl.len;
    for (int i = threadIdx.x; i < m; i += 256) xs[i] = row[c0 + i];
    __syncthreads();
    for (int t = threadIdx.x; t < pl.n_leaves * 8; t += 256) {         // eight stride-8 accumulators per leaf
      const int l = t >> 3, k = t & 7;
      const int s = pl.leaf_start[l], L = pl.leaf_len[l];
      if (L < 8) {
        if (k == 0) {
          float acc = -0.f;
          for (int i = 0; i < L; ++i) acc += xs[s + i];
          leaf[l] = acc;
        }
      } else {
        const int L8 = L - L % 8;
        float acc = xs[s + k];
        for (int i = 8; i < L8; i += 8) acc += xs[s + i + k];
        part[t] = acc;
      }
    }
    __syncthreads();
    for (int l = threadIdx.x; l < pl.n_leaves; l += 256) {
      const int s = pl.leaf_start[l], L = pl.leaf_len[l];
      if (L >= 8) {
        const float* q = part + l * 8;
        float res = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
        for (int i = L - L % 8; i < L; ++i) res += xs[s + i];
        leaf[l] = res;
      }
    }
    __syncthreads();
    int k0 = 0;
    for (int lv = 0; lv < pl.n_levels; ++lv) {                         // the recursion's adds, deepest first
      const int k1 = pl.level_end[lv];
      for (int k = k0 + (int)threadIdx.x; k < k1; k += 256) leaf[pl.op_dst[k]] = leaf[pl.op_dst[k]] + leaf[pl.op_src[k]];
      k0 = k1;
      __syncthreads();
    }
    if (threadIdx.x == 0) total = total + leaf[0];
    __syncthreads();                                                   // xs / leaf are reused by the next buffer
  }
  if (threadIdx.x == 0) {
    args.den[mat][r] = sqrtf(total / (float)n) + 1e-15f;
    if (args.gap[mat]) args.gap[mat][r] = total == 0.f;
  }
}

// ---- 3. column sums: one sequential chain per column -----------------------------------------------------------------------------
__global__ __launch_bounds__(64) void denoise_col_sums_kernel(RowSumArgs args, int32_t n) {
  const int mat = blockIdx.y;
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (c >= n) return;
  const float* x = args.x[mat] + c;
  float acc = 0.f;
  float v[kColAhead];
  int64_t r = 0;
  if (n >= kColAhead) {
#pragma unroll
    for (int j = 0; j < kColAhead; ++j) v[j] = x[(int64_t)j * n];
    for (r = kColAhead; r + kColAhead <= n; r += kColAhead) {
#pragma unroll
      for (int j = 0; j < kColAhead; ++j) {                            // add row r - 32 + j, then load row r + j into its slot
        acc += v[j];
        v[j] = x[(r + j) * n];
      }
    }
#pragma unroll
    for (int j = 0; j < kColAhead; ++j) acc += v[j];
  }
  for (; r < n; ++r) acc += x[r * n];
  args.den[mat][c] = sqrtf(acc / (float)n) + 1e-15f;
  if (args.gap[mat]) args.gap[mat][c] = acc == 0.f;
}

// ---- 4. combine ---------------------------------------------------------------------------------------------------------------
struct CombineArgs {
  const float *p_den1, *p_den2, *o_den1, *o_den2;
  const uint8_t *gap1, *gap2;
};

__device__ __forceinline__ float np_maximum(float a, float b) { return (a >= b || a != a) ? a : b; }

template <bool kVec>
__device__ __forceinline__ void load4(const float* p, float (&v)[4], int valid) {
  if (kVec && valid == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    for (int k = 0; k < 4; ++k) v[k] = k < valid ? p[k] : 0.f;
  }
}

template <bool kVec>
__device__ __forceinline__ void store4(float* p, const float (&v)[4], int valid) {
  if (kVec && valid == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < 4; ++k) if (k < valid) p[k] = v[k];
  }
}

// P lives in my_proba and O in origin_part (in place); my (before its own coverage) goes to `my`.
template <bool kVec>
__global__ __launch_bounds__(256) void denoise_combine_kernel(float* __restrict__ my_proba, float* __restrict__ origin_part, float* __restrict__ my,
                                                              int32_t n, CombineArgs a) {
  const int64_t r = blockIdx.y;
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (c >= n) return;
  const int valid = n - c < 4 ? (int)(n - c) : 4;
  const int64_t e = r * n + c;
  float p[4], o[4], mp[4], op[4], m[4];
  load4<kVec>(my_proba + e, p, valid);
  load4<kVec>(origin_part + e, o, valid);
  const float pr = a.p_den1[r], orr = a.o_den1[r];
  const bool g1 = a.gap1[r] != 0;
  for (int k = 0; k < 4; ++k) {
    const int64_t cc = k < valid ? c + k : c;
    mp[k] = p[k] / pr / a.p_den2[cc];
    op[k] = o[k] / orr / a.o_den2[cc];
    m[k] = np_maximum(mp[k] * op[k], mp[k]);
    if (g1 || a.gap2[cc]) mp[k] = 0.f;
  }
  store4<kVec>(my_proba + e, mp, valid);
  store4<kVec>(origin_part + e, op, valid);
  store4<kVec>(my + e, m, valid);
}

// ---- 5. my's own coverage and the gap mask ---------------------------------------------------------------------------------------
template <bool kVec>
__global__ __launch_bounds__(256) void denoise_finish_kernel(float* __restrict__ my, int32_t n, const float* __restrict__ den1,
                                                             const float* __restrict__ den2, const uint8_t* __restrict__ gap1,
                                                             const uint8_t* __restrict__ gap2) {
  const int64_t r = blockIdx.y;
  const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (c >= n) return;
  const int valid = n - c < 4 ? (int)(n - c) : 4;
  const int64_t e = r * n + c;
  float m[4];
  load4<kVec>(my + e, m, valid);
  const float d1 = den1[r];
  const bool g1 = gap1[r] != 0;
  for (int k = 0; k < 4; ++k) {
    const int64_t cc = k < valid ? c + k : c;
    m[k] = m[k] / d1 / den2[cc];
    if (g1 || gap2[cc]) m[k] = 0.f;
  }
  store4<kVec>(my + e, m, valid);
}

// ---- 6. pixels ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void denoise_pixels_kernel(const float* __restrict__ m, int32_t n, int32_t min_dis, float* __restrict__ out) {
  const int64_t r = blockIdx.y;
  const int64_t K = n > min_dis ? (int64_t)n - min_dis : 0;
  const int64_t cnt = K - r;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= cnt) return;
  out[pair_offset(r, K) + t] = m[r * n + r + min_dis + t];
}

struct DenoisePlan {
  size_t off_den, total;
};

DenoisePlan make_dplan(int32_t n) {
  DenoisePlan pl;
  pl.off_den = 0;
  pl.total = align_up((size_t)6 * n * sizeof(float), 256);             // 6 coverage denominators: P, O, my  x  rows, columns
  return pl;
}

bool denoise_n_ok(int32_t n) { return n >= 1 && (int64_t)n * n <= ((int64_t)1 << 31) - 1; }

// Row and column coverage denominators of one or two matrices (x1 may be null); den = {rows x0, cols x0, rows x1, cols x1}; the gap
// masks (sum == 0) are taken of the second matrix when given.
int launch_sums(const float* x0, const float* x1, float* const* den, uint8_t* gap_rows, uint8_t* gap_cols, int32_t n, hipStream_t st) {
  const int nmat = x1 ? 2 : 1;
  RowSumArgs ra{{x0, x1}, {den[0], x1 ? den[2] : nullptr}, {nullptr, gap_rows}};
  RowSumArgs ca{{x0, x1}, {den[1], x1 ? den[3] : nullptr}, {nullptr, gap_cols}};
  const int head = n < kBuf ? n : kBuf;
  const PwPlan full = make_pw_plan(head);
  const PwPlan tail = make_pw_plan(n % kBuf ? n % kBuf : head);
  hipLaunchKernelGGL(denoise_row_sums_kernel, dim3((unsigned)n, (unsigned)nmat), dim3(256), 0, st, ra, n, full, tail);
  MATCHA_CHECK_LAUNCH("denoise_row_sums_kernel");
  hipLaunchKernelGGL(denoise_col_sums_kernel, dim3((unsigned)cdiv(n, 64), (unsigned)nmat), dim3(64), 0, st, ca, n);
  MATCHA_CHECK_LAUNCH("denoise_col_sums_kernel");
  return MATCHA_OK;
}

}  // namespace
}  // namespace matcha

using namespace matcha;

extern "C" size_t matcha_denoise_workspace_bytes(int32_t n) {
  if (!denoise_n_ok(n)) return 0;
  return make_dplan(n).total;
}

extern "C" int matcha_denoise_intra(const float* proba, int64_t n_pairs, int32_t n, int32_t min_dis, const float* origin, int64_t origin_ld,
                                    float* my, float* origin_part, float* my_proba, uint8_t* gap, void* ws, size_t ws_bytes,
                                    matcha_stream_t stream) {
  MATCHA_CHECK_ARG(proba && origin && my && origin_part && my_proba && gap && ws, "matcha_denoise_intra: null pointer");
  MATCHA_CHECK_ARG(denoise_n_ok(n), "matcha_denoise_intra: n must be >= 1 with n * n < 2^31 (the quantile transform's limit)");
  MATCHA_CHECK_ARG(min_dis >= 0 && min_dis < n, "matcha_denoise_intra: min_dis must be in [0, n): the chromosome has no pairs");
  const int64_t K = (int64_t)n - min_dis;
  MATCHA_CHECK_ARG(n_pairs == K * (K + 1) / 2, "matcha_denoise_intra: n_pairs does not match n and min_dis");
  MATCHA_CHECK_ARG(origin_ld >= n, "matcha_denoise_intra: origin_ld < n");
  const DenoisePlan pl = make_dplan(n);
  MATCHA_CHECK_ARG(ws_bytes >= pl.total, "matcha_denoise_intra: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float* den = (float*)((char*)ws + pl.off_den);
  float* d[6] = {den, den + n, den + 2 * (int64_t)n, den + 3 * (int64_t)n, den + 4 * (int64_t)n, den + 5 * (int64_t)n};
  uint8_t* gap1 = gap;
  uint8_t* gap2 = gap + n;
  const unsigned nt = (unsigned)cdiv(n, kTile);
  hipLaunchKernelGGL(denoise_assemble_kernel, dim3(nt, nt), dim3(256), 0, st, proba, origin, origin_ld, n, min_dis, my_proba, origin_part);
  MATCHA_CHECK_LAUNCH("denoise_assemble_kernel");
  MATCHA_TRY(launch_sums(my_proba, origin_part, d, gap1, gap2, n, st));      // P: d[0] rows, d[1] cols; O: d[2], d[3] and the gaps
  const dim3 eg((unsigned)cdiv(n, 1024), (unsigned)n);
  const CombineArgs ca{d[0], d[1], d[2], d[3], gap1, gap2};
  if (n % 4 == 0) hipLaunchKernelGGL(denoise_combine_kernel<true>, eg, dim3(256), 0, st, my_proba, origin_part, my, n, ca);
  else hipLaunchKernelGGL(denoise_combine_kernel<false>, eg, dim3(256), 0, st, my_proba, origin_part, my, n, ca);
  MATCHA_CHECK_LAUNCH("denoise_combine_kernel");
  float* dm[4] = {d[4], d[5], nullptr, nullptr};
  MATCHA_TRY(launch_sums(my, nullptr, dm, nullptr, nullptr, n, st));
  if (n % 4 == 0) hipLaunchKernelGGL(denoise_finish_kernel<true>, eg, dim3(256), 0, st, my, n, d[4], d[5], gap1, gap2);
  else hipLaunchKernelGGL(denoise_finish_kernel<false>, eg, dim3(256), 0, st, my, n, d[4], d[5], gap1, gap2);
  MATCHA_CHECK_LAUNCH("denoise_finish_kernel");
  return MATCHA_OK;
}

extern "C" int matcha_denoise_pixels(const float* m, int32_t n, int32_t min_dis, float* out, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(m && out, "matcha_denoise_pixels: null pointer");
  MATCHA_CHECK_ARG(denoise_n_ok(n), "matcha_denoise_pixels: n must be >= 1 with n * n < 2^31");
  MATCHA_CHECK_ARG(min_dis >= 0 && min_dis < n, "matcha_denoise_pixels: min_dis must be in [0, n): the chromosome has no pairs");
  const int64_t K = (int64_t)n - min_dis;
  hipLaunchKernelGGL(denoise_pixels_kernel, dim3((unsigned)cdiv(K, 256), (unsigned)n), dim3(256), 0, (hipStream_t)stream, m, n, min_dis, out);
  MATCHA_CHECK_LAUNCH("denoise_pixels_kernel");
  return MATCHA_OK;
}
