// One token row [d] spread over a group of 16 adjacent lanes: each lane owns the float4 chunks j = 4*s + 64*c (s = lane & 15), so one
// wave-instruction reads four whole rows (4 x 256 B at d = 64) and every row statistic is a 4-step xor-shuffle reduction.  Shared by the
// token-level kernels (token_kernels.hip) and the per-locus classifier head (locus.hip), whose logits must be those of head_fwd_kernel bit
// for bit: the arithmetic below is the one place either of them takes it from.
#pragma once
#include "common.hpp"

namespace matcha {

constexpr int kTPT = 16;       // lanes per token row
constexpr int kMaxChunk = 4;   // float4 chunks per lane: d <= 256
constexpr float kLnEps = 1e-5f;

struct Row {
  float4 v[kMaxChunk];
};

template <int NCH>
__device__ __forceinline__ void load_row(const float* __restrict__ p, int s, int d, Row& r) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int j = 4 * s + 64 * c;
    r.v[c] = (j < d) ? *reinterpret_cast<const float4*>(p + j) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
template <int NCH>
__device__ __forceinline__ void store_row(float* __restrict__ p, int s, int d, const Row& r) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int j = 4 * s + 64 * c;
    if (j < d) *reinterpret_cast<float4*>(p + j) = r.v[c];
  }
}
// mean / rstd of a row spread over 16 lanes (two-pass, like ATen's LayerNorm on the values themselves)
template <int NCH>
__device__ __forceinline__ void row_stats(const Row& r, int s, int d, float& mean, float& rstd) {
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) sum += (r.v[c].x + r.v[c].y) + (r.v[c].z + r.v[c].w);   // lanes past d hold zeros
  sum = group_sum<kTPT>(sum);
  mean = sum / (float)d;
  float sq = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (4 * s + 64 * c < d) {
      const float a = r.v[c].x - mean, b = r.v[c].y - mean, e = r.v[c].z - mean, f = r.v[c].w - mean;
      sq += (a * a + b * b) + (e * e + f * f);
    }
  }
  sq = group_sum<kTPT>(sq);
  rstd = 1.0f / sqrtf(sq / (float)d + kLnEps);
}
template <int NCH>
__device__ __forceinline__ void normalize(const Row& in, int s, int d, float mean, float rstd, Row& out) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const bool ok = 4 * s + 64 * c < d;
    out.v[c].x = ok ? (in.v[c].x - mean) * rstd : 0.f;
    out.v[c].y = ok ? (in.v[c].y - mean) * rstd : 0.f;
    out.v[c].z = ok ? (in.v[c].z - mean) * rstd : 0.f;
    out.v[c].w = ok ? (in.v[c].w - mean) * rstd : 0.f;
  }
}
template <int NCH>
__device__ __forceinline__ void affine(const Row& xh, const Row& g, const Row& b, Row& out) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    out.v[c].x = xh.v[c].x * g.v[c].x + b.v[c].x;
    out.v[c].y = xh.v[c].y * g.v[c].y + b.v[c].y;
    out.v[c].z = xh.v[c].z * g.v[c].z + b.v[c].z;
    out.v[c].w = xh.v[c].w * g.v[c].w + b.v[c].w;
  }
}

// the instance of a kernel templated on the chunks per lane: NCH = 1 (d <= 64), 2 (d <= 128), 4 (d <= 256)
static inline int nch_of(int d) { return d <= 64 ? 1 : (d <= 128 ? 2 : 4); }

#define DISPATCH_NCH(d, CALL)                      \
  switch (nch_of(d)) {                             \
    case 1: { constexpr int NCH = 1; CALL; } break; \
    case 2: { constexpr int NCH = 2; CALL; } break; \
    default: { constexpr int NCH = 4; CALL; } break; \
  }

}  // namespace matcha
