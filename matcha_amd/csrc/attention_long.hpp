// What the long rows' attention forward (attention_long.hip) and backward (attention_long_bwd.hip) share: the 32 x 32 score tile of one
// (hyperedge, head) on v_mfma_f32_32x32x2_f32 and its softmax.  Both kernels call these two functions on the same operands, so the backward
// recomputes the forward's probabilities bit for bit and no [B, 8, L, L + 1] tensor is kept.
#pragma once
#include "kernels.hpp"

namespace matcha {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// accumulator register v of lane half h holds tile row 8 (v >> 2) + 4 h + (v & 3) (the column is lane & 31)
__device__ __forceinline__ constexpr int long_tile_row(int v, int h) { return 8 * (v >> 2) + 4 * h + (v & 3); }

// T[a][b] = A_a . B_b over 8 n4 features: ap / bp are the lane's rows of the two operands, already offset by the lane half's float4 (per 8 features
// the two lane halves take the two adjacent float4 of their row -- a row's pair shares a 32-byte sector --, one feature per k-step: the order of
// the contraction is free as long as both operands follow it).  Lane (r, h) gets T[long_tile_row(v, h)][r] in register v.
__device__ __forceinline__ f32x16 long_tile_nt(const float4* ap, const float4* bp, int n4) {
  f32x16 acc = {0};
  auto step4 = [&](const float4& a, const float4& q) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, q.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, q.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, q.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, q.w, acc, 0, 0, 0);
  };
  int c = 0;
  for (; c + 4 <= n4; c += 4) {                 // four float4 pairs in flight in front of their sixteen steps
    const float4 a0 = ap[2 * c], q0 = bp[2 * c], a1 = ap[2 * c + 2], q1 = bp[2 * c + 2];
    const float4 a2 = ap[2 * c + 4], q2 = bp[2 * c + 4], a3 = ap[2 * c + 6], q3 = bp[2 * c + 6];
    step4(a0, q0); step4(a1, q1); step4(a2, q2); step4(a3, q3);
  }
  for (; c < n4; ++c) step4(ap[2 * c], bp[2 * c]);
  return acc;
}

// softmax of query i = r over its keys, from the transposed score tile acc (register v: key j = long_tile_row(v, h)): weight 1 for a real key
// j != i, n_pad for the padding column j = k, 0 behind it.  p[v] comes back WITH the multiplicity: p at j = k is n_pad P_pad.
__device__ __forceinline__ void long_softmax(const f32x16& acc, int k, int n_pad, int r, int h, float inv_temp, float (&p)[16]) {
  const float padf = (float)n_pad;
  float mx = -3.4e38f;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int j = 8 * (v >> 2) + 4 * h + (v & 3);
    const bool on = (j < k && j != r) || (j == k && n_pad > 0);
    p[v] = acc[v] * inv_temp;
    if (on) mx = fmaxf(mx, p[v]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, kWave));
  float den = 0.f;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int j = 8 * (v >> 2) + 4 * h + (v & 3);
    const bool on = (j < k && j != r) || (j == k && n_pad > 0);
    const float e = on ? __expf(p[v] - mx) : 0.f;      // (one v_exp, like the fused forward's softmax: the fp32 grade holds at scores of +-60, the `sharp` cases of tests/test_hip_long_grid.py)
    p[v] = j == k ? padf * e : e;
    den += p[v];
  }
  den += __shfl_xor(den, 32, kWave);
  const float inv = 1.f / den;                    // (a query r >= k is never stored; every stored query has a key: L >= 2)
#pragma unroll
  for (int v = 0; v < 16; ++v) p[v] *= inv;
}

}  // namespace matcha
