// Per-locus scores (matcha_locus_scores, forward_long.hip): the classifier head with the per-token value kept.
//
// The reference's logit is the masked mean of a per-position score, pff_classifier((layer_norm1(dynamic) - layer_norm2(static))^2) of shape
// [B, L, 1] (Modules.py:290-311).  head_fwd_kernel (token_kernels.hip) holds that value in `o` just before it adds it to the row's total;
// head_scores_kernel is that kernel -- its lane layout, its term order, its sequential total, from the same token_row.hpp -- with `o` stored
// at the token's slot and, on request, the row's `lowest` least supported loci selected inside the 16-lane group.  The logit it writes is the
// one head_fwd_kernel writes, bit for bit.
#include "kernels.hpp"
#include "token_row.hpp"

namespace matcha {

namespace {

// (class << 8) | slot of one candidate of the selection: class 0 = a number, 1 = a NaN, 2 = nothing (a lane without a token, or a locus already
// taken).  Order: class, then -- numbers only -- value, then slot: ascending by value, ties to the lower slot, a NaN behind every number.
constexpr int kNone = (2 << 8) | 64;
__device__ __forceinline__ int sel_tag(float v, int slot) { return ((v != v) ? (1 << 8) : 0) | slot; }
__device__ __forceinline__ bool sel_less(float va, int ta, float vb, int tb) {
  const int ca = ta >> 8, cb = tb >> 8;
  if (ca != cb) return ca < cb;
  if (ca == 0 && va != vb) return va < vb;
  return ta < tb;
}

}  // namespace

template <int NCH>
__global__ __launch_bounds__(256) void head_scores_kernel(const int32_t* __restrict__ row_off, const int32_t* __restrict__ tok_slot,
                                                          const float* __restrict__ H2, const float* __restrict__ X, int64_t B, int L, int d,
                                                          HeadParams hp, float* __restrict__ scores, float* __restrict__ logits, int lowest,
                                                          int64_t* __restrict__ order) {
  const int s = threadIdx.x & 15;
  const int64_t b = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (b >= B) return;
  Row Gp, Bp, G1, B1, G2, B2, Wc;
  load_row<NCH>(hp.gp, s, d, Gp); load_row<NCH>(hp.bp, s, d, Bp);
  load_row<NCH>(hp.g1, s, d, G1); load_row<NCH>(hp.b1, s, d, B1);
  load_row<NCH>(hp.g2, s, d, G2); load_row<NCH>(hp.b2, s, d, B2);
  load_row<NCH>(hp.wc, s, d, Wc);
  const float bc = hp.bc[0];
  float total = 0.f, cnt = 0.f;
  const int t_lo = row_off[b], t_hi = row_off[b + 1];   // the hyperedge's real tokens (ragged layout: pads are not stored)
  // lane s keeps the scores of tokens s and s + 16 of the row (k <= 32) and their slots inside the row; a slot outside 0 .. L-1 -- the plan
  // cannot produce one unless x changed under it -- is dropped, so no store leaves the row
  const int64_t base = b * (int64_t)L;
  int sl0 = -1, sl1 = -1;
  if (t_lo + s < t_hi) sl0 = (int)((int64_t)tok_slot[t_lo + s] - base);
  if (t_lo + 16 + s < t_hi) sl1 = (int)((int64_t)tok_slot[t_lo + 16 + s] - base);
  if (sl0 < 0 || sl0 >= L) sl0 = -1;
  if (sl1 < 0 || sl1 >= L) sl1 = -1;
  float v0 = 0.f, v1 = 0.f;
  for (int64_t t = t_lo; t < t_hi; ++t) {
    Row h, hh, u, uh, dn, xr, xh, sn;
    float m, r;
    load_row<NCH>(H2 + t * d, s, d, h);
    row_stats<NCH>(h, s, d, m, r); normalize<NCH>(h, s, d, m, r, hh); affine<NCH>(hh, Gp, Bp, u);
    row_stats<NCH>(u, s, d, m, r); normalize<NCH>(u, s, d, m, r, uh); affine<NCH>(uh, G1, B1, dn);
    load_row<NCH>(X + t * d, s, d, xr);
    row_stats<NCH>(xr, s, d, m, r); normalize<NCH>(xr, s, d, m, r, xh); affine<NCH>(xh, G2, B2, sn);
    float o = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const float a = dn.v[c].x - sn.v[c].x, e = dn.v[c].y - sn.v[c].y, f = dn.v[c].z - sn.v[c].z, g = dn.v[c].w - sn.v[c].w;
      o += (a * a * Wc.v[c].x + e * e * Wc.v[c].y) + (f * f * Wc.v[c].z + g * g * Wc.v[c].w);
    }
    o = group_sum<kTPT>(o) + bc;
    total += o;
    cnt += 1.f;
    const int i = (int)(t - t_lo);
    if (i == s) v0 = o;
    if (i == s + 16) v1 = o;
  }
  const float z = total / (cnt + 1e-15f);
  if (s == 0 && logits) logits[b] = z;
  // every element of the row, once: the real loci where they stand in x, 0.0f at the slots no token claims
  uint32_t real = (sl0 >= 0 ? 1u << sl0 : 0u) | (sl1 >= 0 ? 1u << sl1 : 0u);
#pragma unroll
  for (int o = kTPT / 2; o > 0; o >>= 1) real |= (uint32_t)__shfl_xor((int)real, o, kWave);
  if (sl0 >= 0) scores[base + sl0] = v0;
  if (sl1 >= 0) scores[base + sl1] = v1;
  if (s < L && !((real >> s) & 1u)) scores[base + s] = 0.0f;
  if (s + 16 < L && !((real >> (s + 16)) & 1u)) scores[base + s + 16] = 0.0f;
  if (lowest <= 0) return;
  // `lowest` rounds of a 16-lane minimum over (score, slot); the winner's owner retires it.  Lane s keeps results s and s + 16.
  int t0 = sl0 >= 0 ? sel_tag(v0, sl0) : kNone, t1 = sl1 >= 0 ? sel_tag(v1, sl1) : kNone;
  int r0 = -1, r1 = -1;
  for (int j = 0; j < lowest; ++j) {
    const bool first = sel_less(v0, t0, v1, t1);
    float bv = first ? v0 : v1;
    int bt = first ? t0 : t1;
#pragma unroll
    for (int o = kTPT / 2; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, kWave);
      const int ot = __shfl_xor(bt, o, kWave);
      const bool take = sel_less(ov, ot, bv, bt);
      bv = take ? ov : bv;
      bt = take ? ot : bt;
    }
    const int win = (bt >> 8) == 2 ? -1 : (bt & 0xFF);
    if (win >= 0 && win == sl0) t0 = kNone;
    if (win >= 0 && win == sl1) t1 = kNone;
    if (j == s) r0 = win;
    if (j == s + 16) r1 = win;
  }
  int64_t* ord = order + b * (int64_t)lowest;
  if (s < lowest) ord[s] = r0;
  if (s + 16 < lowest) ord[s + 16] = r1;
}

int launch_head_scores(const int32_t* row_off, const int32_t* tok_slot, const float* H2, const float* X, int64_t B, int L, int d,
                       const HeadParams& hp, float* scores, float* logits, int lowest, int64_t* order, hipStream_t st) {
  if (B <= 0) return MATCHA_OK;
  DISPATCH_NCH(d, hipLaunchKernelGGL((head_scores_kernel<NCH>), dim3((unsigned)cdiv(B, 16)), dim3(256), 0, st, row_off, tok_slot, H2, X, B, L, d,
                                     hp, scores, logits, lowest, order));
  MATCHA_CHECK_LAUNCH("head_scores_kernel");
  return MATCHA_OK;
}

}  // namespace matcha
