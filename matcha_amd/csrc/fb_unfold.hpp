// Un-folding of the LayerNorm affines behind the fused backward's chain rule, as block-level roles.
//   fb_unfold_rows   16 rows of one (matrix, head): fb_unfold_kernel runs it on the rows it summed from the slab, fbm_chain_kernel's paired body
//                    on the rows its own block just produced (fused_bwd.hip) -- one text, so both give the same bits
//   fb_unfold2_vec   one 64-vector of the final sums: fb_unfold2_kernel runs eight of them in one block of 512 threads, node_scatter_kernel's
//                    two bodies (front_fused.hip) in two blocks behind its own (StepRoute::paired on the node route)
#pragma once
#include "kernels.hpp"

namespace matcha {

constexpr int kWgSlab = 4 * 4096 + 6 * 64;   // dW'q dW'k dW'v dWfc1 | dcq dck dcv dKpad dVpad dfc1_b
constexpr int kVecOff = 4 * 4096;
constexpr float kEpsLn = 1e-5f;

__device__ __forceinline__ void ln_row16(const float4& v, float& mean, float& rstd) {
  const float s = group_sum<16>((v.x + v.y) + (v.z + v.w));
  mean = s * (1.f / 64.f);
  const float a = v.x - mean, b = v.y - mean, c = v.z - mean, e = v.w - mean;
  const float q = group_sum<16>((a * a + b * b) + (c * c + e * e));
  rstd = __builtin_amdgcn_rsqf(q * (1.f / 64.f) + kEpsLn);
}

struct UnfoldArgs {
  const float* wslab; int nchunks;
  const float* X; const int32_t* count; int x_pad_row0;        // x_pad_row0: X is the per-node table, the padding token's row is row 0
  const float* W[3]; const float* g[3]; const float* b[3];     // original projection weights [512, 64] and LN affines
  float* gW[3]; float* gfc1;                                    // accumulated into
  float* part;                                                  // [32][3][3][64]: {dg, db, dx_hat_pad} partials
};
// 256 threads = 16 rows x 16 lanes (float4): thread (rl, c4) holds s = the slab sum of row 16 slice + rl, columns c4 .. c4 + 3 of matrix `mat`
// ({q, k, v, fc1}) of `head`; dc / dpad = that row's entries of the bias and padding-row vectors (mat < 3).  red: 16 x 3 x 64 floats of LDS.
// mat is uniform over the block (the barrier sits behind the fc1 return).
__device__ __forceinline__ void fb_unfold_rows(const UnfoldArgs& a, int slice, int mat, int head, float4 s, float dc, float dpad, float (*red)[3][64]) {
  const int tid = threadIdx.x, rl = tid >> 4, c4 = (tid & 15) * 4;
  const int row = slice * 16 + rl;
  if (mat == 3) {       // dfc1[n][head*64 + k]
    float4* o = reinterpret_cast<float4*>(a.gfc1 + (int64_t)row * 512 + head * 64 + c4);
    float4 v = *o;
    v.x += s.x; v.y += s.y; v.z += s.z; v.w += s.w;
    *o = v;
    return;
  }
  // the padding token's K / V rows are x_hat_pad . W'^T + c: its dK / dV enter dW' and dc like one more token
  const float4 xv = *reinterpret_cast<const float4*>(a.X + (a.x_pad_row0 ? (int64_t)0 : (int64_t)a.count[1] * 64) + c4);
  float m, rs;
  ln_row16(xv, m, rs);
  s.x += dpad * (xv.x - m) * rs; s.y += dpad * (xv.y - m) * rs; s.z += dpad * (xv.z - m) * rs; s.w += dpad * (xv.w - m) * rs;
  dc += dpad;
  const int64_t wi = ((int64_t)head * 64 + row) * 64 + c4;
  const float4 W = *reinterpret_cast<const float4*>(a.W[mat] + wi);
  const float4 G = *reinterpret_cast<const float4*>(a.g[mat] + c4), Bv = *reinterpret_cast<const float4*>(a.b[mat] + c4);
  {
    float4* o = reinterpret_cast<float4*>(a.gW[mat] + wi);
    float4 v = *o;
    v.x += s.x * G.x + dc * Bv.x; v.y += s.y * G.y + dc * Bv.y; v.z += s.z * G.z + dc * Bv.z; v.w += s.w * G.w + dc * Bv.w;
    *o = v;
  }
  *reinterpret_cast<float4*>(&red[rl][0][c4]) = make_float4(s.x * W.x, s.y * W.y, s.z * W.z, s.w * W.w);                              // dg
  *reinterpret_cast<float4*>(&red[rl][1][c4]) = make_float4(dc * W.x, dc * W.y, dc * W.z, dc * W.w);                                  // db
  *reinterpret_cast<float4*>(&red[rl][2][c4]) = make_float4(dpad * W.x * G.x, dpad * W.y * G.y, dpad * W.z * G.z, dpad * W.w * G.w);  // dx_hat_pad
  __syncthreads();
  if (tid < 192) {
    const int which = tid >> 6, k = tid & 63;
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) t += red[q][which][k];
    a.part[(((int64_t)(head * 4 + slice) * 3 + mat) * 3 + which) * 64 + k] = t;
  }
}

struct Unfold2Args {
  const float* part; const float* wslab; int nchunks;
  float* dg[3]; float* db[3]; float* dfc1_b; float* dxpad;
  int dxpad_add;     // merged heads: dxpad already holds the attention's gradient into the padding token's x_hat (fbm_chain_kernel): 1 adds the
                     // un-folding's term to it; 2: fbm_chain_kernel's paired body left it FINAL (fused_bwd.hip says why it can) and vec 6 is not run
};
// vec 0..5 = {dg, db} x {q, k, v}; vec 6 = dx_hat of the padding token; vec 7 = fc1 bias gradient; k = the element of the 64-vector.  Every
// (vec, k) is a serial sum of its own: whichever thread of whichever block runs it, the bits are the same.  (Sixteen loads in flight, not all 32:
// the host kernel's registers are the maximum over its roles, and node_scatter_kernel's token walk wants eight wavefronts per SIMD.)
__device__ __forceinline__ void fb_unfold2_vec(const Unfold2Args& a, int vec, int k) {
  float s = 0.f;
  if (vec < 6) {
    const int mat = vec >> 1, which = vec & 1;
#pragma unroll 16
    for (int p = 0; p < 32; ++p) s += a.part[(((int64_t)p * 3 + mat) * 3 + which) * 64 + k];
    float* o = (which == 0 ? a.dg[mat] : a.db[mat]) + k;
    *o += s;
  } else if (vec == 6) {
    if (a.dxpad_add == 2) return;
#pragma unroll 8
    for (int p = 0; p < 32; ++p) s += a.part[(((int64_t)p * 3 + 1) * 3 + 2) * 64 + k] + a.part[(((int64_t)p * 3 + 2) * 3 + 2) * 64 + k];
    a.dxpad[k] = a.dxpad_add ? a.dxpad[k] + s : s;
  } else {
    for (int c = 0; c < a.nchunks; ++c) s += a.wslab[(int64_t)c * kWgSlab + kVecOff + 320 + k];     // head 0's slabs
    a.dfc1_b[k] += s;
  }
}
// the role inside a launch of 256-thread blocks: two blocks, four vectors each
constexpr int kUnfold2RoleBlocks = 2;
__device__ __forceinline__ void fb_unfold2_role(const Unfold2Args& a, int role_block) {
  fb_unfold2_vec(a, role_block * 4 + ((int)threadIdx.x >> 6), (int)threadIdx.x & 63);
}

}  // namespace matcha
