// Fused backward of the multi-head attention block for embed_dim 64 (training path of the metric's configuration), merged heads
// (per head r = B_h x_hat + b_h, s_ij = r_i . x_hat_j, z_i = sum_j p_ij x_hat_j, dyn += M_h z_i).
//
// Given X (the encoder input, [Tn, 64]), dDyn = dL/d(fc1 output before bias) ([Tn, 64], produced by the tail's backward inside the
// forward kernel or by the pff / tail backward kernels) and the record the training forward left per (half tile, head) -- its wavefront's
// r rows as register images + the attention probabilities --, fused_bwdh_kernel produces for ONE head
//   dB_h, dM_h, db_h, the column sums of dDyn, the padding token's d x_hat, and the head's contribution to d x_hat
// without materialising r / z / P or their gradients in HBM (Modules.py:519-572 backward).
//
// Work decomposition ("head-major"): workgroup (head, chunk) walks the half tiles of its chunk of hyperedges.  B_h and M_h stay in
// registers as MFMA fragments (three bf16 planes each, round 5), dB_h and dM_h accumulate in MFMA accumulators for the whole walk and are
// written once per workgroup into a slab.  fbm_reduce_kernel sums the slabs in a fixed order, fbm_chain_kernel applies the chain rule back to the folded projections
// (dW'q = W'k dB, dW'k = W'q dB^T + cq (x) db, dWfc1_h = dM W'v^T + ..., dW'v = Wfc1_h^T dM), fb_unfold_kernel un-folds the LayerNorm affines:
//   W' = W * g, c = W . b   =>   dW = dW' * g + dc (x) b,   dg = sum_n dW' * W,   db = W^T dc.
// The eight heads of a token add their d x_hat into one [T, 64] buffer (float atomics, one instruction = four token rows x 64 B) or, for
// deterministic / row-sparse callers, write eight slabs that lnhat_bwd_kernel / front_bwd_kernel sum in a fixed order.
//
// The reference's own four-product formulation (Q, K, V, fc1 per head) is NOT in this file any more: option disable_merged runs it on
// the layer-by-layer kernels (attention.hip, gemm_lds.hip), which is what the merged kernels are tested against.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "bf16x3.hpp"
#include "kernels.hpp"
#include "tail_reduce.hpp"
#include "fb_unfold.hpp"

namespace matcha {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int kLd = 68;              // LDS row stride (floats)
// (kWgSlab / kVecOff -- the slab format dW'q dW'k dW'v dWfc1 | dcq dck dcv dKpad dVpad dfc1_b -- and ln_row16: fb_unfold.hpp)
constexpr int kMaxChunks = 64;
// buffer descriptor of the per-node adds (fused_bwdh_kernel): dword 3 of a raw gfx9 buffer of 32-bit data, and a byte offset that lies past the
// range of every descriptor the launcher admits (< 2^31 bytes), so that the hardware drops the lane
constexpr int kRsrcRaw32 = 0x00020000;
constexpr uint32_t kOffPastAny = 0x80000000u;

#define ZR8(p)                                                                                           \
  do {                                                                                                   \
    *reinterpret_cast<float4*>(p) = make_float4(0.f, 0.f, 0.f, 0.f);                                     \
    *reinterpret_cast<float4*>((p) + 4) = make_float4(0.f, 0.f, 0.f, 0.f);                               \
  } while (0)

// Attention forward + backward on LDS tiles, token-parallel: one 8-lane group per QUERY token (lane `sub` owns features
// [8 sub, 8 sub + 8)), so a tile's <= 63 tokens fill the 32 groups of the workgroup in two passes and the work per group
// is O(k) instead of O(k^2).  Formulas: attention.hip (attn_bwd_kernel).
//   row phase (token i):    P_i., Pp_i, O_i, dS_i., dSp_i, dQ_i  -- everything that needs only row i of the score matrix;
//                           P_i. and dS_i. go to LDS ([64][8] each), O_i and dQ_i stay in registers
//   column phase (token j): dV_j = sum_i P_ij dO_i,  dK_j = sum_i dS_ij Q_i   over the hyperedge's rows
//   write phase:            O -> Fs, dQ/dK/dV over Q/K/V (after a barrier: the column phase reads Q and dO of other rows)
// acc: this lane's running sums {dK_pad, dV_pad} x 8 features.
// Eight consecutive floats as four packed pairs: dot products and axpys compile to v_pk_mul / v_pk_fma (two flops per lane
// per instruction) instead of scalar chains the compiler re-packs with extra moves.

// The attention rows are STREAMED: one key / value row in use and one in flight.  FB_PIN(addr, x): an empty asm that takes the LDS offset
// of the NEXT row and the eight registers of the running sum as in / out operands: the load of row j + 1 cannot be issued before the
// arithmetic on row j - 1 has produced x.  (sched_barrier alone does not do it: instruction selection has already placed the unchained
// LDS loads of all rows ahead of the arithmetic -- 40 to 80 operand registers -- when the machine scheduler sees the fence.)
#define FB_PIN(addr, x) asm volatile("" : "+v"(addr), "+v"((x).a), "+v"((x).b), "+v"((x).c), "+v"((x).d))
// Keys = values (merged heads: both are the x_hat rows, kpad = vpad = the padding token's x_hat): ONE pass over the rows.  With the weights
// w_j = p_ij (w_pad = n_pad p_i,pad) and d_j = dz_i . x_j:   z_i = sum_j w_j x_j,   sig = sum_j w_j d_j,   A = sum_j (w_j d_j) x_j, and
//   d r_i = sum_j dS_ij x_j = (A - sig z_i) / temp        (dS_ij = w_j (d_j - sig) / temp; the sums include the padding term),
// so the second read of every row (attn_row8's K pass) and its address arithmetic go away.  Same outputs as attn_row8.
template <int ML>
__device__ __forceinline__ void attn_row8_kv(const float* __restrict__ Qs, const float* __restrict__ Xs, const float* __restrict__ Fs,
                                             const float* __restrict__ xpad, const float* __restrict__ Ps, float* __restrict__ dSs, int li, int li0,
                                             int k, int n_pad, int sub, float inv_temp, V8& o, V8& gq, V8& accK, V8& accV) {
  const float padf = (float)n_pad;
  const bool hp = n_pad > 0;
  float p[ML], ds[ML], pp;
  {
    const float4 pa = *reinterpret_cast<const float4*>(&Ps[li * 8]), pb = *reinterpret_cast<const float4*>(&Ps[li * 8 + 4]);
    const float w[8] = {pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w};
#pragma unroll
    for (int j = 0; j < ML; ++j) p[j] = (j < k) ? w[j] : 0.f;
    pp = hp ? w[7] : 0.f;
  }
  const float ppf = padf * pp;
  const int ro0 = li0 * kLd + 8 * sub;                   // row j (clamped to the hyperedge): ro0 + min(j, k - 1) rows
  const V8 go = ld8(&Fs[li * kLd + 8 * sub]);
  const V8 vp = ld8(xpad + 8 * sub);
  const float dsp_raw = group_sum8_dpp(dot8(go, vp));
  float sig = ppf * dsp_raw;
  o = scale8(ppf, vp);
  V8 a = scale8(ppf * dsp_raw, vp);
  V8 vn = ld8(&Xs[ro0]), vn2 = ld8(&Xs[ro0 + (1 < k ? 1 : 0) * kLd]);      // two rows in flight
#pragma unroll
  for (int j = 0; j < ML; ++j) {
    const V8 v = vn;
    vn = vn2;
    if (j + 2 < ML) {
      int ad = ro0 + (j + 2 < k ? j + 2 : 0) * kLd;
      FB_PIN(ad, o);
      vn2 = ld8(&Xs[ad]);
    }
    axpy8(o, p[j], v);
    const float d = group_sum8_dpp(dot8(go, v));
    ds[j] = d;
    const float wd = p[j] * d;
    sig += wd;
    axpy8(a, wd, v);
  }
#pragma unroll
  for (int j = 0; j < ML; ++j) ds[j] = p[j] * (ds[j] - sig) * inv_temp;
  const float dspf = padf * (pp * (dsp_raw - sig) * inv_temp);
  axpy8(accV, ppf, go);
  // d r_i = (A - sig z_i) / temp
  {
    const float ns = -sig;
    axpy8(a, ns, o);
    gq = scale8(inv_temp, a);
  }
  {
    int ad = li * kLd + 8 * sub;
    FB_PIN(ad, gq);
    const V8 q = ld8(&Qs[ad]);
    axpy8(accK, dspf, q);
  }
  if (sub == 1) {                                          // row i of dS for the column phase (P is in Ps already)
    float* dst = dSs + li * 8;
    *reinterpret_cast<float4*>(dst) = make_float4(ds[0], ds[1 % ML], ML > 2 ? ds[2 % ML] : 0.f, ML > 3 ? ds[3 % ML] : 0.f);
    if (ML > 4) *reinterpret_cast<float4*>(dst + 4) = make_float4(ds[4 % ML], ML > 5 ? ds[5 % ML] : 0.f, ML > 6 ? ds[6 % ML] : 0.f, ML > 7 ? ds[7 % ML] : 0.f);
  }
}

// The row phase of the VALUE-TABLE instance (node route): y_j = M_h x_hat_j is gathered per node (Ys), so
//   d_j = dz_i . x_hat_j = dDyn_i . y_j,   d_pad = dDyn_i . y_pad
// needs neither dZ nor Z.  TWO passes: the y rows give d_j and sig, then the x_hat rows take dS_ij directly,
//   d r_i = sum_j dS_ij x_hat_j + dS_i,pad x_hat_pad
// -- no z sum (Z is never formed), no A - sig z cancellation, eight packed operations per key instead of twelve and one running sum alive
// per pass.  (The one-pass form -- A - sig z with the y row read next to the x_hat row -- was measured in the same call: step 1.189-1.192 ms
// against 1.176-1.181 ms for this one, parent 1.200-1.204 ms; profiles/r10_node_v.md.)
// accU += n_pad p_i,pad dDyn_i (u_pad: what the padding key's VALUE contributes to dM_h and to its own d x_hat).
#define FB_PIN1(addr, s) asm volatile("" : "+v"(addr), "+v"(s))
template <int ML>
__device__ __forceinline__ void attn_row8_v(const float* __restrict__ Qs, const float* __restrict__ Xs, const float* __restrict__ Ys, const float* __restrict__ Ds,
                                            const float* __restrict__ xpad, const float* __restrict__ ypad, const float* __restrict__ Ps, float* __restrict__ dSs,
                                            int li, int li0, int k, int n_pad, int sub, float inv_temp, V8& gq, V8& accK, V8& accU) {
  const float padf = (float)n_pad;
  const bool hp = n_pad > 0;
  float p[ML], ds[ML], pp;
  {
    const float4 pa = *reinterpret_cast<const float4*>(&Ps[li * 8]), pb = *reinterpret_cast<const float4*>(&Ps[li * 8 + 4]);
    const float w[8] = {pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w};
#pragma unroll
    for (int j = 0; j < ML; ++j) p[j] = (j < k) ? w[j] : 0.f;
    pp = hp ? w[7] : 0.f;
  }
  const float ppf = padf * pp;
  const int ro0 = li0 * kLd + 8 * sub;                   // row j (clamped to the hyperedge): ro0 + min(j, k - 1) rows
  const V8 go = ld8(&Ds[li * kLd + 8 * sub]);
  const float dsp_raw = group_sum8_dpp(dot8(go, ld8(ypad + 8 * sub)));
  float sig = ppf * dsp_raw;
  {
    V8 vn = ld8(&Ys[ro0]), vn2 = ld8(&Ys[ro0 + (1 < k ? 1 : 0) * kLd]);      // two rows in flight
    float part = 0.f;                                      // the pin chains the load of row j + 2 to row j - 1's dot product, NOT to its DPP reduction
#pragma unroll
    for (int j = 0; j < ML; ++j) {
      const V8 v = vn;
      vn = vn2;
      if (j + 2 < ML) {
        int ad = ro0 + (j + 2 < k ? j + 2 : 0) * kLd;
        FB_PIN1(ad, part);
        vn2 = ld8(&Ys[ad]);
      }
      part = dot8(go, v);
      const float d = group_sum8_dpp(part);
      ds[j] = d;
      sig += p[j] * d;
    }
  }
#pragma unroll
  for (int j = 0; j < ML; ++j) ds[j] = p[j] * (ds[j] - sig) * inv_temp;
  const float dspf = padf * (pp * (dsp_raw - sig) * inv_temp);
  axpy8(accU, ppf, go);
  gq = scale8(dspf, ld8(xpad + 8 * sub));
  {
    V8 vn = ld8(&Xs[ro0]), vn2 = ld8(&Xs[ro0 + (1 < k ? 1 : 0) * kLd]);
#pragma unroll
    for (int j = 0; j < ML; ++j) {
      const V8 v = vn;
      vn = vn2;
      if (j + 2 < ML) {
        int ad = ro0 + (j + 2 < k ? j + 2 : 0) * kLd;
        FB_PIN(ad, gq);
        vn2 = ld8(&Xs[ad]);
      }
      axpy8(gq, ds[j], v);
    }
  }
  {
    int ad = li * kLd + 8 * sub;
    FB_PIN(ad, gq);
    const V8 q = ld8(&Qs[ad]);
    axpy8(accK, dspf, q);
  }
  if (sub == 1) {                                          // row i of dS for the column phase (P is in Ps already)
    float* dst = dSs + li * 8;
    *reinterpret_cast<float4*>(dst) = make_float4(ds[0], ds[1 % ML], ML > 2 ? ds[2 % ML] : 0.f, ML > 3 ? ds[3 % ML] : 0.f);
    if (ML > 4) *reinterpret_cast<float4*>(dst + 4) = make_float4(ds[4 % ML], ML > 5 ? ds[5 % ML] : 0.f, ML > 6 ? ds[6 % ML] : 0.f, ML > 7 ? ds[7 % ML] : 0.f);
  }
}

template <int ML>
__device__ __forceinline__ void attn_col8(const float* __restrict__ Qs, const float* __restrict__ Fs, const float* __restrict__ Ps,
                                          const float* __restrict__ dSs, int li, int li0, int k, int sub, V8& gk, V8& gv) {
  const int jj = li - li0;
  gk = zero8();
  gv = zero8();
  const int ro0 = li0 * kLd + 8 * sub;
  V8 qn = ld8(&Qs[ro0]), gn = ld8(&Fs[ro0]);
#pragma unroll
  for (int i = 0; i < ML; ++i) {
    const V8 q = qn, go = gn;
    const int ri = li0 + (i < k ? i : 0);
    // unconditional loads (the row index is clamped into the hyperedge, whose rows hold finite values) + a select: `cond ? load : 0` becomes a
    // branch around the load
    const float pl = Ps[ri * 8 + jj], dl = dSs[ri * 8 + jj];
    const float pij = (i < k) ? pl : 0.f, dsij = (i < k) ? dl : 0.f;
    if (i + 1 < ML) {
      int a = ro0 + (i + 1 < k ? i + 1 : 0) * kLd;
      FB_PIN(a, gk);
      qn = ld8(&Qs[a]); gn = ld8(&Fs[a]);
    }
    axpy8(gv, pij, go);
    axpy8(gk, dsij, q);
  }
}

// -DFB_TIMING: per-phase wall-clock (100 MHz) of workgroup 0, printed at the end -- development builds only
#ifdef FB_TIMING
#define FB_T(i) do { const long long now__ = wall_clock64(); tph[i] += now__ - tlast; tlast = now__; } while (0)
#else
#define FB_T(i) do { } while (0)
#endif

#define MFMA16(A, B, C) __builtin_amdgcn_mfma_f32_16x16x4f32((A), (B), (C), 0, 0, 0)      /* the small per-step products (fbm_chain_kernel) */

// ---- the backward of  r = B_h x + b_h,  s_ij = r_i . x_j,  z_i = sum_j p_ij x_j,  dyn += M_h z  (merged heads) ----------
// Per (half tile, head) FOUR 64 x 64 products instead of the reference formulation's eight:  dZ = dDyn M_h;  d x_hat = dR B_h + (the
// attention's own gradient into its keys / values, which ARE the x_hat rows);  dB_h += dR^T x_hat;  dM_h += dDyn^T Z.  The attention runs
// attn_row8_kv / attn_col8 with Q := r, K := V := x_hat, dO := dZ; what those return as dK + dV is d x_hat's attention part (tile Gs), what
// they accumulate for the padding key / value is d x_hat of the padding token.  fbm_chain_kernel then applies the chain rule from
// (dB_h, db_h, dM_h, d bdyn) to the folded projections, and the LayerNorm un-folding follows.
constexpr int kWgSlabM = 2 * 4096 + 4 * 64;     // dB_h dM_h | db_h (column sums of dR), d bdyn (column sums of dDyn), dxpad, spare
constexpr int kVecOffM = 2 * 4096;
// Walk: workgroup = (head, chunk of the forward's own HALF tiles: whole hyperedges, <= 31 tokens, ragged.hip half_meta), FOUR wavefronts,
// TWO workgroups per CU -- at different phases, so one's attention (latency-bound vector + LDS work) runs under the other's GEMMs.  Every
// wavefront owns 16 feature columns of each product.  The forward's saved record is per (half tile, head): its wavefront's register image.
constexpr int kTileH = 32 * kLd;
// ---- round 5: the four products on the bf16 matrix pipe (fp32-accurate: three bf16 planes per operand, six plane products; the note is in
// fused_fwd32.hip, the arithmetic restated in tests/test_cpu_bf16x3.py) ---------------------------------------------------------------------
// The f32 MFMA shares the vector ALUs with the attention arithmetic (128 x 32 cycles per wavefront and half tile next to ~600 vector
// instructions); v_mfma_f32_16x16x32_bf16 has its own pipe.  What makes it pay HERE is that every GEMM operand is split ONCE where it is
// produced and kept in LDS as bf16 planes -- dDyn and x_hat by the staging threads (one split per workgroup, not per wavefront: a 16 x 16
// output tile reuses a fragment only six times), dR and Z by the attention's write phase, B_h and M_h once per workgroup walk in registers:
//   plane tile = [32 tokens][80 bf16] x 3 planes (160-byte rows: with 144-byte rows a third of the LDS cycles were bank conflicts --
//     SQ_LDS_BANK_CONFLICT 70 M of SQ_LDS_IDX_ACTIVE 221 M per launch; on 40-dword rows both kinds of read are conflict-free)
//   row fragment (contraction over FEATURES: dZ^T = M_h^T dDyn^T, d x_hat = dR B_h)   = one ds_read_b128 per plane
//   column fragment (contraction over TOKENS: dB_h += dR^T x_hat, dM_h += dDyn^T Z)   = two ds_read_b64_tr_b16 per plane -- the hardware
//     transpose read hands lane i of a 16-lane group column i of a 4 row x 16 column block (MI355X guide T10)
// LDS per workgroup (81 280 B: two workgroups per CU just fit): x_hat f32 (the attention's keys / values) + planes, dDyn planes, RB = r f32 ->
// dR planes, FB = dZ f32 -> Z planes, G f32.  One set only: the next half tile's rows wait in registers (fetched during the GEMMs) and are
// staged at the top of the next iteration.
constexpr int kPS = 80;                 // bf16 per plane row: 40 dwords -- with the token slots below BOTH fragment reads are conflict-free (bank sets
                                        // {0,40,16,56,32,8,48,24} + 4 kq for the 16-byte row reads, 8-bank slots 40 r mod 64 for eight consecutive rows)
constexpr int kPlane = 32 * kPS;        // bf16 per plane
constexpr int kPT = 3 * kPlane;         // bf16 per three-plane tile (15 360 B)
// column fragments: contraction slot 8 kq + j holds token 4 kq + j (j < 4) or 16 + 4 kq + (j - 4) -- free, both operands of a product use the
// same map -- so that a 32-lane half reads EIGHT CONSECUTIVE rows per transposed read.  The lane's block address: row 4 kq + ((lane & 15) >> 2),
// columns c0 + 4 (lane & 3); lane i of the 16-lane group receives column c0 + i
typedef Planes<kPS, 16> PL;
__device__ __forceinline__ Frag3 frag_row(const short* __restrict__ p) { return PL::row(p); }
__device__ __forceinline__ void frag_store(short* __restrict__ p, const Frag3& f) { PL::store(p, f); }
__device__ __forceinline__ Frag3 frag_col(const short* __restrict__ p) { return PL::col(p); }

struct FusedBwdHArgs {
  const float* X; const float* dDyn; const int32_t* count; const int32_t* half_meta; const int32_t* tok_pos;
  int L; int nhalves; int nchunks;
  const float* mB; const float* mM;               // merged matrices [8][64][64] (launch_prep_heads)
  float* dxh; int64_t tcap;
  int dx_atomic;                                   // 1: every head adds into ONE [tcap][64] buffer with float atomics (zeroed by the launcher); 0: one slab per head
  float* wslab;                                    // [8][nchunks][kWgSlabM]
  const float* rimg;                               // [nhalves][8][kImgRecH]: r rows (register images) + attention probabilities of the forward
  const int32_t* xrow;                             // NODE instances: X is the per-node table of NORMALISED rows [n_nodes + 1][64] (node_xhat_kernel) and token t reads
                                                   // row xrow[t] (the plan's tok_key: 0 = padding) -- no LayerNorm in the staging
  const float* rn; int64_t rn_head;                // NODE instances, non-null: the heads' r rows per node [8][rn_head / 64][64] (node_r_kernel); the record holds probabilities only
  const float* vn;                                 // VTAB instances: the heads' value rows per node, y = M_h x_hat, laid out like rn (node_r_kernel's V role)
  float* dx_node;                                  // VTAB instances, non-null: d x_hat is added per NODE -- [8][rn_head / 64][64], one replica per head (zeroed by the caller), token t
                                                   // into row xrow[t]: the same atomic bytes as into dxh, and no row per token is left to walk (node_scatter_kernel finishes per node)
};
constexpr size_t kBwdLdsBytes = (size_t)2 * kTileH * 4 + (size_t)4 * kPT * 2 + (64 + 256 + 256 + 32 + 32) * 4;
static_assert(2 * kBwdLdsBytes <= 160 * 1024, "two workgroups per CU");

// VTAB (node route with the r AND the value table): per (half tile, head) THREE products and five barrier phases.  With
// y_j = M_h x_hat_j gathered per node and U_j = sum_i p_ij dDyn_i in the column phase's value accumulator,
//   d_j = dDyn_i . y_j;   d x_hat = [dR | U] [B_h ; M_h] + GK;   dM_h = U^T x_hat + u_pad (x) x_hat_pad;   d x_hat_pad = accK + u_pad M_h
// (u_pad = sum_i n_pad p_i,pad dDyn_i) -- no dZ product, no Z, dDyn only a vector operand.  LDS regions by lifetime: Dp = dDyn f32 rows (+ y_pad
// behind them), FBp = y f32 rows -> U planes (written by the column phase: nobody reads y behind the row phase's barrier), Gs = GK only.
template <int ML, bool NODE, bool VTAB = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void fused_bwdh_kernel(FusedBwdHArgs g) {
  static_assert(NODE || !VTAB, "the value table belongs to the node route");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Xs = lds;                                   // x_hat f32 (keys = values of the attention)
  float* Gs = lds + kTileH;                          // attention's gradient into the x_hat rows (keys + values)
  short* Xp = reinterpret_cast<short*>(lds + 2 * kTileH);   // x_hat planes
  short* Dp = Xp + kPT;                              // dDyn planes
  short* RBp = Dp + kPT;                             // r f32 -> dR planes
  short* FBp = RBp + kPT;                            // dZ f32 -> Z planes
  float* Rs = reinterpret_cast<float*>(RBp);
  float* Fs = reinterpret_cast<float*>(FBp);
  float* Ds = reinterpret_cast<float*>(Dp);          // VTAB: dDyn f32 rows [32][kLd], zero past the tokens
  float* ypad = Ds + kTileH;                         // VTAB: y of the padding token (VN[head][0]) behind them, inside the Dp region
  float* sm = reinterpret_cast<float*>(FBp + kPT);
  float* xpad = sm;
  float* dSs = xpad + 64;             // [32][8]
  float* Ps = dSs + 256;              // [32][8]
  int* tinfo = reinterpret_cast<int*>(Ps + 256);     // [32]
  int* keys_s = tinfo + 32;                          // [32] dx_node: the half tile's table rows (tok_key), read by the d x_hat phase

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c16 = lane & 15, kq = lane >> 4;           // 16x16x32 fragments: row / column c16, contraction slots 8 kq + {0..7}
  const int fb = 16 * wave;                            // this wave's 16 feature columns
  const int srow = tid >> 4, sc4 = (tid & 15) * 4;     // staging: 16 rows x 16 lanes (float4), twice

  int head, chunk;
  if ((g.nchunks & 7) == 0) {
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    head = j & 7;
    chunk = (j >> 3) * 8 + xcd;
  } else {
    head = blockIdx.x & 7;
    chunk = blockIdx.x >> 3;
  }
  const int tr = g.count[1];
  int nh = g.count[3];
  if (nh > g.nhalves) nh = g.nhalves;
  const int per = (nh + g.nchunks - 1) / g.nchunks;
  const int tile_lo = chunk * per;
  const int tile_hi = (tile_lo + per < nh) ? tile_lo + per : nh;
  const float inv_temp = 0.125f;
#ifdef FB_TIMING
  long long tph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long tlast = wall_clock64();
#endif

  if (tid < 16) {                     // the padding token's x_hat
    const float4 xv = *reinterpret_cast<const float4*>(g.X + (NODE ? (int64_t)0 : (int64_t)tr * 64) + sc4);
    if constexpr (NODE) {
      *reinterpret_cast<float4*>(&xpad[sc4]) = xv;
    } else {
      float m, rs;
      ln_row16(xv, m, rs);
      *reinterpret_cast<float4*>(&xpad[sc4]) = make_float4((xv.x - m) * rs, (xv.y - m) * rs, (xv.z - m) * rs, (xv.w - m) * rs);
    }
  }
  if constexpr (VTAB) {
    static_assert((size_t)(kTileH + 64) * 4 <= (size_t)kPT * 2, "dDyn rows + y_pad fit the Dp region");
    if (tid >= 64 && tid < 80) *reinterpret_cast<float4*>(&ypad[sc4]) = *reinterpret_cast<const float4*>(g.vn + (int64_t)head * g.rn_head + sc4);
  }

  // weight-gradient accumulators: rows 16 mt + 4 kq + reg, column fb + c16 of dB_h and dM_h (four 16 x 16 tiles each)
  f32x4 ab0 = {0.f, 0.f, 0.f, 0.f}, ab1 = ab0, ab2 = ab0, ab3 = ab0, am0 = ab0, am1 = ab0, am2 = ab0, am3 = ab0;
  V8 accK = zero8(), accV = zero8();                  // the padding token's gradient as a key (sum dS_i,pad r_i) and as a value (sum p_i,pad dz_i)
  // column sums of dDyn (columns sc4 + {0..3} over the rows this thread stages) and of dR (features 8 sub + {0..7} over this lane group's tokens)
  f2 cd0 = {0.f, 0.f}, cd1 = cd0;
  V8 accR = zero8();

  const int4* meta = reinterpret_cast<const int4*>(g.half_meta);
  const int4 mzero = make_int4(0, 0, 0, 0);
  int4 mc = tile_lo < tile_hi ? meta[tile_lo] : mzero;
  int4 mn = tile_lo + 1 < tile_hi ? meta[tile_lo + 1] : mzero;
  float4 xn0, xn1, dn0, dn1;
  int tpn = 0, kyn = 0;               // (kyn, dx_node: the token's table row, fetched with tok_pos one half tile ahead)
  int kx0 = 0, kx1 = 0;               // NODE: the table rows of the half tile whose rows are fetched NEXT (loaded one half tile earlier: no dependent load in the prefetch)
#define FBH_KEY_GLOAD(I, M)                                                                              \
  do {                                                                                                   \
    const int row__ = srow + 16 * (I);                                                                   \
    kx##I = g.xrow[(M).x + (row__ < (M).y ? row__ : ((M).y > 0 ? (M).y - 1 : 0))];                       \
  } while (0)
  f32x4 ri0, ri1, yi0, yi1, pn = {0.f, 0.f, 0.f, 0.f};
#define FBH_ROW_GLOAD(I, M)                                                                              \
  do {                                                                                                   \
    const int row__ = srow + 16 * (I);                                                                   \
    const int64_t tok__ = (M).x + (row__ < (M).y ? row__ : ((M).y > 0 ? (M).y - 1 : 0));                 \
    xn##I = *reinterpret_cast<const float4*>(g.X + (NODE ? (int64_t)kx##I : tok__) * 64 + sc4);           \
    dn##I = *reinterpret_cast<const float4*>(g.dDyn + tok__ * 64 + sc4);                                 \
  } while (0)
  // DXN (the per-node adds' walk, below): tok_pos and the key are loaded by EVERY thread (slot tid & 31, the index clamped as above) and in front
  // of the rows -- a load under `tid < 32` behind them is one the compiler cannot count when it waits for the rows (see the walk)
#define FBH_ROWS_GLOAD(M, DXN)                                                                           \
  do {                                                                                                   \
    if ((DXN) || tid < 32) {                                                                             \
      const int s__ = tid & 31;                                                                          \
      const int i__ = (M).x + (s__ < (M).y ? s__ : ((M).y > 0 ? (M).y - 1 : 0));                         \
      tpn = g.tok_pos[i__];                                                                              \
      if ((DXN) || (VTAB && g.dx_node)) kyn = g.xrow[i__];                                               \
    }                                                                                                    \
    FBH_ROW_GLOAD(0, M); FBH_ROW_GLOAD(1, M);                                                            \
  } while (0)
  // NODE with the r table: this head's r rows of the same two table rows, row-major like the x_hat rows (16 lanes per 256-byte row).  Issued
  // next to FBH_ROWS_GLOAD while kx0 / kx1 still hold that half tile's keys
  const bool r_tab = VTAB || (NODE && g.rn != nullptr);
#define FBH_R_GLOAD()                                                                                    \
  do {                                                                                                   \
    const float* rh__ = g.rn + (int64_t)head * g.rn_head + sc4;                                          \
    ri0 = *reinterpret_cast<const f32x4*>(rh__ + (int64_t)kx0 * 64); ri1 = *reinterpret_cast<const f32x4*>(rh__ + (int64_t)kx1 * 64); \
    if constexpr (VTAB) {                                                                                \
      const float* vh__ = g.vn + (int64_t)head * g.rn_head + sc4;                                        \
      yi0 = *reinterpret_cast<const f32x4*>(vh__ + (int64_t)kx0 * 64); yi1 = *reinterpret_cast<const f32x4*>(vh__ + (int64_t)kx1 * 64); \
    }                                                                                                    \
  } while (0)
  // x_hat row -> Xs (f32) and Xp (planes); dDyn row (zero past the tokens) -> Dp (planes) + its column sums
#define FBH_ROW_STAGE(I)                                                                                 \
  do {                                                                                                   \
    const int row__ = srow + 16 * (I);                                                                   \
    const float msk__ = row__ < n_real ? 1.f : 0.f;                                                      \
    const float4 xv__ = xn##I, dv__ = dn##I;                                                             \
    float4 xh__;                                                                                         \
    if constexpr (NODE) {                                                                                \
      xh__ = make_float4(xv__.x * msk__, xv__.y * msk__, xv__.z * msk__, xv__.w * msk__);                \
    } else {                                                                                             \
      const float mean__ = group_sum16_dpp((xv__.x + xv__.y) + (xv__.z + xv__.w)) * (1.f / 64.f);        \
      const float a__ = xv__.x - mean__, b__ = xv__.y - mean__, c__ = xv__.z - mean__, e__ = xv__.w - mean__; \
      const float q__ = group_sum16_dpp((a__ * a__ + b__ * b__) + (c__ * c__ + e__ * e__));              \
      const float rs__ = msk__ * __builtin_amdgcn_rsqf(q__ * (1.f / 64.f) + kEpsLn);                     \
      xh__ = make_float4(a__ * rs__, b__ * rs__, c__ * rs__, e__ * rs__);                                \
    }                                                                                                    \
    *reinterpret_cast<float4*>(&Xs[row__ * kLd + sc4]) = xh__;                                           \
    {                                                                                                    \
      const P3 p0__ = split2(xh__.x, xh__.y), p1__ = split2(xh__.z, xh__.w);                             \
      short* d__ = Xp + row__ * kPS + sc4;                                                               \
      *reinterpret_cast<u32x2*>(d__) = (u32x2){p0__.h, p1__.h}; *reinterpret_cast<u32x2*>(d__ + kPlane) = (u32x2){p0__.m, p1__.m}; \
      *reinterpret_cast<u32x2*>(d__ + 2 * kPlane) = (u32x2){p0__.l, p1__.l};                             \
    }                                                                                                    \
    const float4 dm__ = make_float4(dv__.x * msk__, dv__.y * msk__, dv__.z * msk__, dv__.w * msk__);     \
    if constexpr (VTAB) {                                                                                \
      *reinterpret_cast<float4*>(&Ds[row__ * kLd + sc4]) = dm__;                                         \
    } else {                                                                                             \
      const P3 p0__ = split2(dm__.x, dm__.y), p1__ = split2(dm__.z, dm__.w);                             \
      short* d__ = Dp + row__ * kPS + sc4;                                                               \
      *reinterpret_cast<u32x2*>(d__) = (u32x2){p0__.h, p1__.h}; *reinterpret_cast<u32x2*>(d__ + kPlane) = (u32x2){p0__.m, p1__.m}; \
      *reinterpret_cast<u32x2*>(d__ + 2 * kPlane) = (u32x2){p0__.l, p1__.l};                             \
    }                                                                                                    \
    cd0 += (f2){dm__.x, dm__.y}; cd1 += (f2){dm__.z, dm__.w};                                            \
  } while (0)
  // the forward wavefront's register image: float4 index (wc * 4 + gq) * 64 + 32 h + r holds features 32 wc + 8 gq + 4 h + {0..3} of row r
#define FBH_RIMG_GLOAD(HALF)                                                                             \
  do {                                                                                                   \
    const f32x4* r__ = reinterpret_cast<const f32x4*>(g.rimg + ((int64_t)(HALF) * MATCHA_N_HEAD + head) * kImgRecH);  \
    if (tid < 64) pn = __builtin_nontemporal_load(r__ + 512 + tid);                                      \
    if (!r_tab) { ri0 = __builtin_nontemporal_load(r__ + tid); ri1 = __builtin_nontemporal_load(r__ + 256 + tid); } \
  } while (0)
  // B_h and M_h as register fragments for the whole walk: lane (c16, kq), step s holds W[32 s + 8 kq + {0..7}][fb + c16] -- the A operand of
  // dZ^T = M_h^T dDyn^T (rows = features) and the B operand of d x_hat = dR B_h (columns = features); three planes each
  Frag3 Mf[2], Bf[2];
  {
    if constexpr (NODE) { FBH_KEY_GLOAD(0, mc); FBH_KEY_GLOAD(1, mc); }
    FBH_ROWS_GLOAD(mc, false);
    if constexpr (NODE) { if (r_tab) FBH_R_GLOAD(); FBH_KEY_GLOAD(0, mn); FBH_KEY_GLOAD(1, mn); }
    if (tile_lo < tile_hi) FBH_RIMG_GLOAD(tile_lo);
    const float* mp = g.mM + (int64_t)head * 4096 + (8 * kq) * 64 + fb + c16;
    const float* bp = g.mB + (int64_t)head * 4096 + (8 * kq) * 64 + fb + c16;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float vm[8], vb[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { vm[j] = mp[(32 * s + j) * 64]; vb[j] = bp[(32 * s + j) * 64]; }
      Mf[s] = split8(vm); Bf[s] = split8(vb);
    }
  }

  // ---- stage half tile M, whose rows wait in registers: the FIRST one here, every later one at the END of the iteration before it ----
#define FBH_STAGE(M, DXN)                                                                                \
  do {                                                                                                   \
    const int n_real = (M).y;                                                                            \
    FBH_ROW_STAGE(0); FBH_ROW_STAGE(1);                                                                  \
    if (tid < 32) tinfo[tid] = tid < n_real ? ((tid - (tpn & 255)) | (tpn & ~255)) : 0;                  \
    if (((DXN) || (VTAB && g.dx_node)) && tid < 32) keys_s[tid] = kyn;                                   \
    if constexpr (VTAB) {                                                                                \
      *reinterpret_cast<f32x4*>(&Fs[srow * kLd + sc4]) = yi0; *reinterpret_cast<f32x4*>(&Fs[(srow + 16) * kLd + sc4]) = yi1; \
    }                                                                                                    \
    if (r_tab) {                                                                                         \
      *reinterpret_cast<f32x4*>(&Rs[srow * kLd + sc4]) = ri0; *reinterpret_cast<f32x4*>(&Rs[(srow + 16) * kLd + sc4]) = ri1; \
    } else {                                                                                             \
      f32x4* d__ = reinterpret_cast<f32x4*>(&Rs[(lane & 31) * kLd + 8 * wave + 4 * (lane >> 5)]);        \
      d__[0] = ri0; d__[8] = ri1;                                                                        \
    }                                                                                                    \
    if (tid < 64) reinterpret_cast<f32x4*>(Ps)[tid] = pn;                                                \
  } while (0)
  if (tile_lo < tile_hi) FBH_STAGE(mc, false);        // (nothing has used the tiles yet: no barrier in front; xpad / ypad lie outside them)

  // The walk is ROTATED: an iteration opens with the barrier behind the staging and closes with the staging of the NEXT half tile, so the
  // staging block is entered from the loop body only.  Why: vmcnt retires in order and the compiler, when it waits for a staged load, counts the
  // memory operations it KNOWS to be newer.  With the staging at the loop's top the prologue's path (no adds behind its loads) merged in front of
  // the waits, and the adds -- one branch each -- were operations that "may not have been issued": the waits came out as vmcnt(8) .. vmcnt(0), which
  // at run time meant "every float atomic of the half tile before has retired" (~1.2 us each with the chip busy) in front of a barrier, once
  // per half tile.  DXN (per-node adds, a walk of its own so that no other d x_hat path merges in front of the staging either): the eight adds
  // are straight-line code and NOTHING the staging consumes is issued behind them, so every wait of the staging leaves >= 8 operations in flight.
  auto walk = [&](auto dxn_c) __attribute__((always_inline)) {
  constexpr bool DXN = decltype(dxn_c)::value;
  for (int tile = tile_lo; tile < tile_hi; ++tile) {
    const int4 mnn = tile + 2 < tile_hi ? meta[tile + 2] : mzero;      // (far in front of the adds: consumed by the key loads behind barrier 4)
    const int t0 = mc.x, n_real = mc.y;
    __syncthreads();                                  // the half tile is staged
    FB_T(7);
    // per-lane indices re-derived from an opaque copy of the thread id (loop-invariant addresses are hoisted and spilled otherwise)
    int tid_ = tid;
    asm volatile("" : "+v"(tid_));
    const int lane = tid_ & 63, wave = tid_ >> 6;
    const int c16 = lane & 15, kq = lane >> 4;
    const int fb = 16 * wave;
    const int srow = tid_ >> 4, sc4 = (tid_ & 15) * 4;
    const int sub = lane & 7;
    (void)srow; (void)sc4;
    // ---- dZ^T = M_h^T . dDyn^T: lane (c16, kq) ends with token c16 (+ 16) and features fb + 4 kq + {0..3} ----
    if constexpr (!VTAB) {
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
      const short* dp = Dp + c16 * kPS + 8 * kq;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const Frag3 b0 = frag_row(dp + 32 * s), b1 = frag_row(dp + 16 * kPS + 32 * s);
        acc0 = mma6(acc0, Mf[s], b0); acc1 = mma6(acc1, Mf[s], b1);
      }
      *reinterpret_cast<f32x4*>(&Fs[c16 * kLd + fb + 4 * kq]) = acc0;
      *reinterpret_cast<f32x4*>(&Fs[(16 + c16) * kLd + fb + 4 * kq]) = acc1;
      FB_T(1);
      __syncthreads();
      FB_T(7);
    }
    // ---- attention forward + backward in x_hat space: 8 lanes per token, all 32 rows in one pass ----
    if constexpr (VTAB) {
      FB_T(1);                                        // (this column is "stage + dZ product" in the other instances: the staging alone here)
      V8 q0, k0, v0;
      const int la = wave * 8 + (lane >> 3);
      const bool acta = la < n_real;
      int ia = 0;
      if (acta) { ia = tinfo[la]; attn_row8_v<ML>(Rs, Xs, Fs, Ds, xpad, ypad, Ps, dSs, la, ia & 255, ia >> 8, g.L - (ia >> 8), sub, inv_temp, q0, accK, accV); }
      __builtin_amdgcn_sched_barrier(0);
      FB_T(2);
      __syncthreads();                                // the y rows are dead from here: the column phase writes the U planes over them
      FB_T(7);
      if (acta) {
        attn_col8<ML>(Rs, Ds, Ps, dSs, la, ia & 255, ia >> 8, sub, k0, v0);      // GK_j = sum_i dS_ij r_i,  U_j = sum_i p_ij dDyn_i
        st8(&Gs[la * kLd + 8 * sub], k0);
      } else {
        ZR8(&Gs[la * kLd + 8 * sub]);
        v0 = zero8(); q0 = zero8();                   // rows past the tokens: zero planes (they are contraction slots of the weight gradients)
      }
      frag_store(FBp + la * kPS + 8 * sub, split8(v0));
      FB_T(3);
      __syncthreads();                                // every column phase is done with the r rows: they become the dR PLANES
      FB_T(7);
      frag_store(RBp + la * kPS + 8 * sub, split8(q0));
      accR.a += q0.a; accR.b += q0.b; accR.c += q0.c; accR.d += q0.d;
    } else {
      V8 o0, q0, k0, v0;
      const int la = wave * 8 + (lane >> 3);
      const bool acta = la < n_real;
      int ia = 0;
      if (acta) { ia = tinfo[la]; attn_row8_kv<ML>(Rs, Xs, Fs, xpad, Ps, dSs, la, ia & 255, ia >> 8, g.L - (ia >> 8), sub, inv_temp, o0, q0, accK, accV); }
      __builtin_amdgcn_sched_barrier(0);
      FB_T(2);
      __syncthreads();
      FB_T(7);
      if (acta) {
        attn_col8<ML>(Rs, Fs, Ps, dSs, la, ia & 255, ia >> 8, sub, k0, v0);
        k0.a += v0.a; k0.b += v0.b; k0.c += v0.c; k0.d += v0.d;      // the row is key AND value: d x_hat_j = sum_i dS_ij r_i + p_ij dz_i
        st8(&Gs[la * kLd + 8 * sub], k0);
      } else {
        ZR8(&Gs[la * kLd + 8 * sub]);
      }
      FB_T(3);
      __syncthreads();                                // every column phase is done with the r and dZ rows: they become the dR and Z PLANES
      FB_T(7);
      if (!acta) { o0 = zero8(); q0 = zero8(); }      // rows past the tokens: zero planes (they are contraction slots of the weight gradients)
      frag_store(FBp + la * kPS + 8 * sub, split8(o0));
      frag_store(RBp + la * kPS + 8 * sub, split8(q0));
      accR.a += q0.a; accR.b += q0.b; accR.c += q0.c; accR.d += q0.d;
    }
    FB_T(4);
    __syncthreads();
    FB_T(7);
    FBH_ROWS_GLOAD(mn, DXN);                          // next half tile's rows: in flight during the GEMMs below
    if constexpr (NODE) { if (r_tab) FBH_R_GLOAD(); FBH_KEY_GLOAD(0, mnn); FBH_KEY_GLOAD(1, mnn); }      // ... its r rows (r table), and the table rows of the one after
    if constexpr (DXN) { if (tile + 1 < tile_hi) FBH_RIMG_GLOAD(tile + 1); }      // ... and its probabilities IN FRONT of the adds (four registers across the d x_hat phase)
    // ---- this head's share of d x_hat = dR B_h + Gs ----
    if (DXN || g.dx_atomic) {                         // (the launcher admits dx_node only with dx_atomic)
      // rows = tokens 4 kq + reg (+ 16), columns = features fb + c16: one atomic instruction covers 4 token rows x 64 contiguous bytes.  Float
      // atomics execute at the memory side, not in an XCD's L2 (every 64-byte segment leaves L2 as one uncached request), so the eight heads' adds do
      // NOT meet on chip: 0.47 GB of added bytes per launch at the headline, a floor of ~0.36 ms at the chip-wide ~1.3 TB/s
      const float* gp = Gs + (4 * kq) * kLd + fb + c16;
      f32x4 dx0 = {gp[0], gp[kLd], gp[2 * kLd], gp[3 * kLd]};
      f32x4 dx1 = {gp[16 * kLd], gp[17 * kLd], gp[18 * kLd], gp[19 * kLd]};
      const short* arow = RBp + c16 * kPS + 8 * kq;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const Frag3 a0 = frag_row(arow + 32 * s), a1 = frag_row(arow + 16 * kPS + 32 * s);
        dx0 = mma6(dx0, a0, Bf[s]); dx1 = mma6(dx1, a1, Bf[s]);
      }
      if constexpr (VTAB) {                           // ... + U M_h: the value part of the attention's gradient, as a longer contraction
        const short* urow = FBp + c16 * kPS + 8 * kq;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const Frag3 a0 = frag_row(urow + 32 * s), a1 = frag_row(urow + 16 * kPS + 32 * s);
          dx0 = mma6(dx0, a0, Mf[s]); dx1 = mma6(dx1, a1, Mf[s]);
        }
      }
      if constexpr (DXN) {
        // per NODE, this head's replica: four 64-byte segments per instruction -- the row is the token's table row instead of the token.
        // EIGHT UNCONDITIONAL instructions (the compiler counts them when the staging waits) on a BUFFER descriptor of this head's replica:
        // a row past the tokens gets a byte offset past the descriptor's range, and the hardware DROPS an out-of-range lane of a buffer
        // atomic -- no request leaves the CU, which is what the `if` per row did, without the branch.  (The other unconditional form, adding
        // cond ? dx : 0.f to the last real token's row, is exact as well -- x + 0.0 = x for every x but -0.0, and a replica starts at +0.0 and
        // is only added to -- but it was measured: 9 % more 64-byte atomic requests, which are what the kernel waits for, cost the headline
        // step +20 us; profiles/r14_atomic_waits.md.)  buffer_atomic_add_f32 is the same memory-side add as global_atomic_add_f32.
        const int4 ka = *reinterpret_cast<const int4*>(&keys_s[4 * kq]), kb = *reinterpret_cast<const int4*>(&keys_s[16 + 4 * kq]);
        const int k0[4] = {ka.x, ka.y, ka.z, ka.w}, k1[4] = {kb.x, kb.y, kb.z, kb.w};
        const __amdgpu_buffer_rsrc_t ah = __builtin_amdgcn_make_buffer_rsrc(g.dx_node + (int64_t)head * g.rn_head, 0, (int)(g.rn_head * 4), kRsrcRaw32);
        const uint32_t col4 = 4u * (uint32_t)(fb + c16);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(dx0[reg], ah, 4 * kq + reg < n_real ? (uint32_t)k0[reg] * 256u + col4 : kOffPastAny, 0, 0);
          __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(dx1[reg], ah, 16 + 4 * kq + reg < n_real ? (uint32_t)k1[reg] * 256u + col4 : kOffPastAny, 0, 0);
        }
      } else {
      float* out = g.dxh + ((int64_t)t0 + 4 * kq) * 64 + fb + c16;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        if (4 * kq + reg < n_real) unsafeAtomicAdd(out + reg * 64, dx0[reg]);
        if (16 + 4 * kq + reg < n_real) unsafeAtomicAdd(out + (16 + reg) * 64, dx1[reg]);
      }
      }
    } else {
      f32x4 dx0 = *reinterpret_cast<const f32x4*>(&Gs[c16 * kLd + fb + 4 * kq]);
      f32x4 dx1 = *reinterpret_cast<const f32x4*>(&Gs[(16 + c16) * kLd + fb + 4 * kq]);
      const short* arow = RBp + c16 * kPS + 8 * kq;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const Frag3 a0 = frag_row(arow + 32 * s), a1 = frag_row(arow + 16 * kPS + 32 * s);
        dx0 = mma6(dx0, Bf[s], a0); dx1 = mma6(dx1, Bf[s], a1);
      }
      if constexpr (VTAB) {
        const short* urow = FBp + c16 * kPS + 8 * kq;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const Frag3 a0 = frag_row(urow + 32 * s), a1 = frag_row(urow + 16 * kPS + 32 * s);
          dx0 = mma6(dx0, Mf[s], a0); dx1 = mma6(dx1, Mf[s], a1);
        }
      }
      float* out = g.dxh + ((int64_t)head * g.tcap + t0 + c16) * 64 + fb + 4 * kq;
      if (c16 < n_real) *reinterpret_cast<f32x4*>(out) = dx0;
      if (16 + c16 < n_real) *reinterpret_cast<f32x4*>(out + 16 * 64) = dx1;
    }
    FB_T(5);
    if constexpr (!DXN) { if (tile + 1 < tile_hi) FBH_RIMG_GLOAD(tile + 1); }     // next half tile's r rows and probabilities: in flight during the weight-gradient GEMMs
    // ---- weight gradients: dB[a][b] += sum_t dR[t][a] x_hat[t][b];  dM[n][m] += sum_t dDyn[t][n] Z[t][m]: ONE 32-token step, column fragments ----
    {
      const int blk = ((4 * kq + ((lane & 15) >> 2)) * kPS) + 4 * (lane & 3);      // this lane's address inside a 4 x 16 transpose block
      const Frag3 xb = frag_col(Xp + blk + fb);
      Frag3 zb;
      if constexpr (!VTAB) zb = frag_col(FBp + blk + fb);
      {
        const Frag3 r0 = frag_col(RBp + blk), r1 = frag_col(RBp + blk + 16);
        ab0 = mma6(ab0, r0, xb); ab1 = mma6(ab1, r1, xb);
        const Frag3 r2 = frag_col(RBp + blk + 32), r3 = frag_col(RBp + blk + 48);
        ab2 = mma6(ab2, r2, xb); ab3 = mma6(ab3, r3, xb);
      }
      if constexpr (VTAB) {                           // dM[n][m] += sum_t U[t][n] x_hat[t][m]: the same x_hat column fragment
        const Frag3 u0 = frag_col(FBp + blk), u1 = frag_col(FBp + blk + 16);
        am0 = mma6(am0, u0, xb); am1 = mma6(am1, u1, xb);
        const Frag3 u2 = frag_col(FBp + blk + 32), u3 = frag_col(FBp + blk + 48);
        am2 = mma6(am2, u2, xb); am3 = mma6(am3, u3, xb);
      } else {
        const Frag3 d0 = frag_col(Dp + blk), d1 = frag_col(Dp + blk + 16);
        am0 = mma6(am0, d0, zb); am1 = mma6(am1, d1, zb);
        const Frag3 d2 = frag_col(Dp + blk + 32), d3 = frag_col(Dp + blk + 48);
        am2 = mma6(am2, d2, zb); am3 = mma6(am3, d3, zb);
      }
    }
    FB_T(6);
    mc = mn; mn = mnn;
    if (tile + 1 < tile_hi) {
      __syncthreads();                                // this half tile's GEMMs are done with every tile
      FB_T(7);
      FBH_STAGE(mc, DXN);                             // the next one's rows, fetched during those GEMMs
      FB_T(0);
    }
  }
  };
  if constexpr (VTAB) {
    if (g.dx_node) walk(std::true_type{}); else walk(std::false_type{});
  } else {
    walk(std::false_type{});
  }

  // ---- workgroup slab ----
  __syncthreads();
#ifdef FB_TIMING
  if (blockIdx.x == 0 && (tid == 0 || tid == 192))
    printf("fused_bwdh wg0 wave %d us: stage %.1f dZ %.1f attn-row %.1f attn-col %.1f attn-write %.1f dx %.1f tn %.1f barrier-wait %.1f (halves %d)\n", tid >> 6,
           tph[0] * 0.01, tph[1] * 0.01, tph[2] * 0.01, tph[3] * 0.01, tph[4] * 0.01, tph[5] * 0.01, tph[6] * 0.01, tph[7] * 0.01, tile_hi - tile_lo);
#endif
  float* slab = g.wslab + ((int64_t)head * g.nchunks + chunk) * kWgSlabM;
  {
    const int col = fb + c16;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = 4 * kq + reg;
      slab[0 * 4096 + row * 64 + col] = ab0[reg]; slab[0 * 4096 + (row + 16) * 64 + col] = ab1[reg];
      slab[0 * 4096 + (row + 32) * 64 + col] = ab2[reg]; slab[0 * 4096 + (row + 48) * 64 + col] = ab3[reg];
      if constexpr (!VTAB) {
        slab[1 * 4096 + row * 64 + col] = am0[reg]; slab[1 * 4096 + (row + 16) * 64 + col] = am1[reg];
        slab[1 * 4096 + (row + 32) * 64 + col] = am2[reg]; slab[1 * 4096 + (row + 48) * 64 + col] = am3[reg];
      }
    }
  }
  // column sums of dDyn: thread (srow, sc4) staged rows srow, srow + 16 of every half tile -- the four row groups of a wave in a fixed xor order,
  // then the four waves in order
  float* redd = lds;                    // [4][64]
  {
    const float cdv[4] = {cd0.x, cd0.y, cd1.x, cd1.y};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = cdv[i];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (lane < 16) redd[wave * 64 + 4 * lane + i] = v;
    }
  }
  // column sums of dR and d x_hat of the padding token: the 8 lanes with equal `sub` of a wave (fixed xor tree), then the 4 waves in order
  float* redr = lds + 4 * 64;           // [4][64]
  float* redp = lds + 8 * 64;           // [4][64]
  // VTAB: accV holds u_pad's partials; they are reduced on their own (redu), because u_pad enters dM_h and d x_hat_pad through products
  float* redu = lds + 12 * 64;          // [4][64]
  float* upad = lds + 16 * 64;          // [64]
  if constexpr (VTAB) {
    const float accu[8] = {accV.a.x, accV.a.y, accV.b.x, accV.b.y, accV.c.x, accV.c.y, accV.d.x, accV.d.y};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float v = accu[i];
      v += __shfl_xor(v, 8, 64);
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (lane < 8) redu[wave * 64 + 8 * lane + i] = v;
    }
    accV = zero8();
  }
  const float accp[16] = {accK.a.x + accV.a.x, accK.a.y + accV.a.y, accK.b.x + accV.b.x, accK.b.y + accV.b.y,
                          accK.c.x + accV.c.x, accK.c.y + accV.c.y, accK.d.x + accV.d.x, accK.d.y + accV.d.y,
                          accR.a.x, accR.a.y, accR.b.x, accR.b.y, accR.c.x, accR.c.y, accR.d.x, accR.d.y};
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float v = accp[i];
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (lane < 8) (i < 8 ? redp : redr)[wave * 64 + 8 * lane + (i & 7)] = v;
  }
  __syncthreads();
  if (tid < 64) {
    slab[kVecOffM + 64 + tid] = (redd[tid] + redd[64 + tid]) + (redd[128 + tid] + redd[192 + tid]);    // d bdyn partial
    slab[kVecOffM + tid] = (redr[tid] + redr[64 + tid]) + (redr[128 + tid] + redr[192 + tid]);         // db_h partial
    if constexpr (!VTAB) slab[kVecOffM + 128 + tid] = (redp[tid] + redp[64 + tid]) + (redp[128 + tid] + redp[192 + tid]);   // dxpad partial
  }
  if constexpr (VTAB) {
    // the two padding terms: dM_h += u_pad (x) x_hat_pad (rank one, into the accumulators before their store) and d x_hat_pad = accK + u_pad M_h
    if (tid < 64) upad[tid] = (redu[tid] + redu[64 + tid]) + (redu[128 + tid] + redu[192 + tid]);
    __syncthreads();
    {
      const float xc = xpad[fb + c16];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = 4 * kq + reg, col = fb + c16;
        slab[1 * 4096 + row * 64 + col] = am0[reg] + upad[row] * xc; slab[1 * 4096 + (row + 16) * 64 + col] = am1[reg] + upad[row + 16] * xc;
        slab[1 * 4096 + (row + 32) * 64 + col] = am2[reg] + upad[row + 32] * xc; slab[1 * 4096 + (row + 48) * 64 + col] = am3[reg] + upad[row + 48] * xc;
      }
    }
    if (tid < 64) {
      const float* mp = g.mM + (int64_t)head * 4096 + tid;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;         // four chains in a fixed order
#pragma unroll 4
      for (int n = 0; n < 64; n += 4) {
        s0 += upad[n] * mp[n * 64]; s1 += upad[n + 1] * mp[(n + 1) * 64]; s2 += upad[n + 2] * mp[(n + 2) * 64]; s3 += upad[n + 3] * mp[(n + 3) * 64];
      }
      slab[kVecOffM + 128 + tid] = ((redp[tid] + redp[64 + tid]) + (redp[128 + tid] + redp[192 + tid])) + ((s0 + s1) + (s2 + s3));
    }
  }
}

// Chain rule from the merged matrices back to the folded projections, one block per head: sums the chunk slabs in order, then
//   B_h = W'k^T W'q, b_h = W'k^T cq:   dW'q = W'k dB;   dW'k = W'q dB^T + cq (x) db;   dcq = W'k db;   dck = 0
//   M_h = Wf_h W'v, bdyn = fc1_b + sum_h Wf_h cv_h:   dWf_h = dM W'v^T + dbdyn (x) cv_h;   dW'v = Wf_h^T dM;   dcv_h = Wf_h^T dbdyn
// and writes ONE slab per head in fused_bwd8_kernel's format (dW'q dW'k dW'v dWfc1 | dcq dck dcv 0 0 dfc1_b), which fb_unfold_kernel /
// fb_unfold2_kernel turn into the gradients of the original parameters as before (nchunks = 1); dxpad is summed here.
struct ChainArgs {
  const float* wslab; int nchunks;           // merged slabs [8][nchunks][kWgSlabM]
  float* red;                                // [8][kWgSlabM] chunk sums (fbm_reduce_kernel)
  const float* wq; const float* wk; const float* wv; const float* cq; const float* cv;   // folded
  const float* fc1_w;
  float* out;                                // [8][kWgSlab]
  float* dxpad;                              // [64]
};
// chunk sums of every slab element in chunk order; dxpad = the sum over heads and chunks of the padding token's share.
// Block roles: blocks [0, kFbmReduceBlocks) sum the backward kernel's slabs; the blocks behind them sum the slabs of the TAIL's parameter
// gradients that the forward left (tail_reduce.hpp) -- independent sums that used to be two launches, one in front of the backward kernel and
// one behind it.
constexpr int kFbmReduceX = (kWgSlabM + 255) / 256;
constexpr int kFbmReduceBlocks = kFbmReduceX * MATCHA_N_HEAD;
__global__ __launch_bounds__(256) void fbm_reduce_kernel(ChainArgs a, TailReduceArgs tl, int tail_blocks) {
  __shared__ float4 part[8 * 32];
  if ((int)blockIdx.x >= kFbmReduceBlocks) {
    tail_reduce_role(tl, (int)blockIdx.x - kFbmReduceBlocks, part);
    return;
  }
  const int head = blockIdx.x / kFbmReduceX, i = (blockIdx.x % kFbmReduceX) * 256 + threadIdx.x;
  if (i >= kWgSlabM) return;
  const float* base = a.wslab + (int64_t)head * a.nchunks * kWgSlabM + i;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, s5 = 0.f, s6 = 0.f, s7 = 0.f;
  int c = 0;
  for (; c + 7 < a.nchunks; c += 8) {                  // eight chunk slabs in flight per thread
    s0 += base[(int64_t)c * kWgSlabM]; s1 += base[(int64_t)(c + 1) * kWgSlabM]; s2 += base[(int64_t)(c + 2) * kWgSlabM]; s3 += base[(int64_t)(c + 3) * kWgSlabM];
    s4 += base[(int64_t)(c + 4) * kWgSlabM]; s5 += base[(int64_t)(c + 5) * kWgSlabM]; s6 += base[(int64_t)(c + 6) * kWgSlabM]; s7 += base[(int64_t)(c + 7) * kWgSlabM];
  }
  for (; c < a.nchunks; ++c) s0 += base[(int64_t)c * kWgSlabM];
  a.red[(int64_t)head * kWgSlabM + i] = ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7));
}
// out[i][j] (16 rows of a 64 x 64 product per block) = sum_x A(i, x) B(x, j) [+ u[i] v[j]] with strided operands staged through LDS
// (lds_out, uniform over the block: the 16 rows are left in As[i * 65 + j] instead of `out` -- the paired body un-folds them from there)
__device__ __forceinline__ void mm64_slice(const float* __restrict__ A, int a_rs, int a_cs, const float* __restrict__ B, int b_rs, int b_cs,
                                           const float* __restrict__ u, const float* __restrict__ v, float* __restrict__ out, int slice,
                                           float* __restrict__ As, float* __restrict__ Bs, bool lds_out = false) {
  const int tid = threadIdx.x;
  {
    // every load of the two operand tiles in flight before the first LDS store (strided operands: scalar loads)
    float av[4], bv[16];
#pragma unroll
    for (int t = 0; t < 4; ++t) { const int i = tid + 256 * t; av[t] = A[(int64_t)(16 * slice + (i >> 6)) * a_rs + (int64_t)(i & 63) * a_cs]; }
#pragma unroll
    for (int t = 0; t < 16; ++t) { const int i = tid + 256 * t; bv[t] = B[(int64_t)(i >> 6) * b_rs + (int64_t)(i & 63) * b_cs]; }
#pragma unroll
    for (int t = 0; t < 4; ++t) { const int i = tid + 256 * t; As[(i >> 6) * 65 + (i & 63)] = av[t]; }
#pragma unroll
    for (int t = 0; t < 16; ++t) { const int i = tid + 256 * t; Bs[(i >> 6) * 65 + (i & 63)] = bv[t]; }
  }
  __syncthreads();
  // 16 x 64 outputs = one 16 x 16 tile per wavefront, 16 steps of v_mfma_f32_16x16x4_f32 over the contraction index
  const int lane = tid & 63, wave = tid >> 6, c16 = lane & 15, kq = lane >> 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) acc = MFMA16(As[c16 * 65 + 4 * kk + kq], Bs[(4 * kk + kq) * 65 + 16 * wave + c16], acc);
  const int j = 16 * wave + c16;
  const float vj = u ? v[j] : 0.f;
  if (lds_out) __syncthreads();                        // every wavefront's fragment reads of As are behind it
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int i = 4 * kq + reg;
    const float o = acc[reg] + (u ? u[16 * slice + i] * vj : 0.f);
    if (lds_out) As[i * 65 + j] = o; else out[(16 * slice + i) * 64 + j] = o;
  }
}
// the two vector gradients of the chain rule, element m: two chains over the contraction index, even and odd (ONE text for block (0, 0, head),
// which writes the vectors, and for the paired body's blocks, which need sixteen elements of one of them each)
__device__ __forceinline__ float chain_dcq(const float* __restrict__ Wk, const float* __restrict__ db, int m) {      // dcq[m] = sum_a W'k[m][a] db[a]
  float s0 = 0.f, s1 = 0.f;
#pragma unroll 8
  for (int x = 0; x < 64; x += 2) { s0 += Wk[m * 64 + x] * db[x]; s1 += Wk[m * 64 + x + 1] * db[x + 1]; }
  return s0 + s1;
}
__device__ __forceinline__ float chain_dcv(const float* __restrict__ Wf, const float* __restrict__ dbdyn, int m) {   // dcv[m] = sum_n Wf[n][m] dbdyn[n]
  float t0 = 0.f, t1 = 0.f;
#pragma unroll 8
  for (int x = 0; x < 64; x += 2) { t0 += Wf[x * 512 + m] * dbdyn[x]; t1 += Wf[(x + 1) * 512 + m] * dbdyn[x + 1]; }
  return t0 + t1;
}
// grid (4 row slices, 4 jobs, 8 heads): the four matrix gradients of a head in fused_bwd8_kernel's slab format; slice 0 also the vectors.
// paired (a launch parameter: the whole grid takes one body; StepRoute::paired): block (slice, job, head) of fb_unfold_kernel reads only the 16 rows
// that this block writes, plus 16 elements of dcq (job 0) or dcv (job 2) from block (0, 0, head) -- so the block keeps its rows in LDS, computes
// those elements itself in the same order, and un-folds them here (fb_unfold_rows, the text fb_unfold_kernel runs): one launch less, and the
// matrices never go to the slab.  What fb_unfold_kernel makes of the slab with one chunk: s = 0 + row, dc = 0 + dcq | dck (= 0) | dcv,
// dpad = 0 + dK_pad | dV_pad = 0 -- taken over literally, additions of zero included, so every gradient is the same bits.
// dxpad_final (with paired, where fb_unfold2 rides in node_scatter_kernel, which READS dxpad): the term fb_unfold2's vec 6 adds to dxpad is a sum
// of products with dpad = +0, which is +0 for finite weights, and dxpad + (+0) is what is stored here -- vec 6 is then not run at all.
__global__ __launch_bounds__(256) void fbm_chain_kernel(ChainArgs a, UnfoldArgs uf, int paired, int dxpad_final) {
  __shared__ float As[16 * 65];
  __shared__ float Bs[64 * 65];
  static_assert(sizeof(float) * 64 * 65 >= sizeof(float) * 16 * 3 * 64, "the un-folding's partials live in Bs");
  const int slice = blockIdx.x, job = blockIdx.y, head = blockIdx.z, tid = threadIdx.x;
  const float* red = a.red + (int64_t)head * kWgSlabM;
  const float* dB = red; const float* dM = red + 4096; const float* db = red + kVecOffM;
  const float* dbdyn = a.red + kVecOffM + 64;              // a sum over ALL tokens: every head saw the same dDyn -- take head 0's
  const float* Wq = a.wq + (int64_t)head * 4096; const float* Wk = a.wk + (int64_t)head * 4096; const float* Wv = a.wv + (int64_t)head * 4096;
  const float* Wf = a.fc1_w + head * 64;                  // Wf[n][m] = fc1_w[n * 512 + head * 64 + m]
  float* out = a.out + (int64_t)head * kWgSlab;
  const bool lds_out = paired != 0;
  if (job == 0) {          // dW'q[m][b] = sum_a W'k[m][a] dB[a][b]
    mm64_slice(Wk, 64, 1, dB, 64, 1, nullptr, nullptr, out + 0 * 4096, slice, As, Bs, lds_out);
  } else if (job == 1) {   // dW'k[m][a] = sum_b W'q[m][b] dB[a][b] + cq[m] db[a]
    mm64_slice(Wq, 64, 1, dB, 1, 64, a.cq + head * 64, db, out + 1 * 4096, slice, As, Bs, lds_out);
  } else if (job == 2) {   // dW'v[m][b] = sum_n Wf[n][m] dM[n][b]
    mm64_slice(Wf, 1, 512, dM, 64, 1, nullptr, nullptr, out + 2 * 4096, slice, As, Bs, lds_out);
  } else {                 // dWf[n][m] = sum_b dM[n][b] W'v[m][b] + dbdyn[n] cv[m]
    mm64_slice(dM, 64, 1, Wv, 1, 64, dbdyn, a.cv + head * 64, out + 3 * 4096, slice, As, Bs, lds_out);
  }
  if (slice == 0 && job == 0 && tid < 64) {
    const float s = chain_dcq(Wk, db, tid), t = chain_dcv(Wf, dbdyn, tid);
    out[kVecOff + tid] = s;                          // dcq[m] = sum_a W'k[m][a] db[a]
    out[kVecOff + 64 + tid] = 0.f;                   // dck: the K bias only shifts all scores of a query (no gradient)
    out[kVecOff + 128 + tid] = t;                    // dcv[m] = sum_n Wf[n][m] dbdyn[n]
    out[kVecOff + 192 + tid] = 0.f; out[kVecOff + 256 + tid] = 0.f;     // dK_pad / dV_pad do not exist here
    out[kVecOff + 320 + tid] = head == 0 ? dbdyn[tid] : 0.f;            // dfc1_b = d bdyn
    if (head == 0) {
      float p = 0.f;
      for (int hh = 0; hh < MATCHA_N_HEAD; ++hh) p += a.red[(int64_t)hh * kWgSlabM + kVecOffM + 128 + tid];
      a.dxpad[tid] = dxpad_final ? p + 0.f : p;
    }
  }
  if (!paired) return;
  const int rl = tid >> 4, c4 = (tid & 15) * 4, row = slice * 16 + rl;
  float dc = 0.f, dpad = 0.f;
  if (job == 0) dc += chain_dcq(Wk, db, row);        // (sixteen lanes per row compute the same element: loads of one address, no exchange)
  else if (job == 1) dc += 0.f;
  else if (job == 2) dc += chain_dcv(Wf, dbdyn, row);
  if (job == 1 || job == 2) dpad += 0.f;
  __syncthreads();                                   // the 16 rows are in As; nobody reads Bs any more
  float4 s;
  s.x = 0.f + As[rl * 65 + c4]; s.y = 0.f + As[rl * 65 + c4 + 1]; s.z = 0.f + As[rl * 65 + c4 + 2]; s.w = 0.f + As[rl * 65 + c4 + 3];
  fb_unfold_rows(uf, slice, job, head, s, dc, dpad, reinterpret_cast<float (*)[3][64]>(Bs));
}

// ---- slab reduction + un-folding of the LayerNorm affines (the per-row and per-vector texts: fb_unfold.hpp) --------------------------
// grid (4 row slices, 4 matrices {q, k, v, fc1}, 8 heads), 256 threads = 16 rows x 16 lanes (float4)
__global__ __launch_bounds__(256) void fb_unfold_kernel(UnfoldArgs a) {
  __shared__ float red[16][3][64];
  const int slice = blockIdx.x, mat = blockIdx.y, head = blockIdx.z;
  const int tid = threadIdx.x, rl = tid >> 4, c4 = (tid & 15) * 4;
  const int row = slice * 16 + rl;
  const float* base = a.wslab + (int64_t)head * a.nchunks * kWgSlab;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  {
    float4 t0 = s, t1 = s, t2 = s, t3 = s;             // four independent chains: four loads in flight per lane
    const float* pb = base + mat * 4096 + row * 64 + c4;
    int c = 0;
    for (; c + 3 < a.nchunks; c += 4) {
      const float4 v0 = *reinterpret_cast<const float4*>(pb + (int64_t)c * kWgSlab), v1 = *reinterpret_cast<const float4*>(pb + (int64_t)(c + 1) * kWgSlab);
      const float4 v2 = *reinterpret_cast<const float4*>(pb + (int64_t)(c + 2) * kWgSlab), v3 = *reinterpret_cast<const float4*>(pb + (int64_t)(c + 3) * kWgSlab);
      t0.x += v0.x; t0.y += v0.y; t0.z += v0.z; t0.w += v0.w;
      t1.x += v1.x; t1.y += v1.y; t1.z += v1.z; t1.w += v1.w;
      t2.x += v2.x; t2.y += v2.y; t2.z += v2.z; t2.w += v2.w;
      t3.x += v3.x; t3.y += v3.y; t3.z += v3.z; t3.w += v3.w;
    }
    for (; c < a.nchunks; ++c) {
      const float4 v = *reinterpret_cast<const float4*>(pb + (int64_t)c * kWgSlab);
      t0.x += v.x; t0.y += v.y; t0.z += v.z; t0.w += v.w;
    }
    s.x = (t0.x + t1.x) + (t2.x + t3.x); s.y = (t0.y + t1.y) + (t2.y + t3.y);
    s.z = (t0.z + t1.z) + (t2.z + t3.z); s.w = (t0.w + t1.w) + (t2.w + t3.w);
  }
  float dc = 0.f, dpad = 0.f;
  if (mat < 3)
    for (int c = 0; c < a.nchunks; ++c) {
      const float* vb = base + (int64_t)c * kWgSlab + kVecOff;
      dc += vb[mat * 64 + row];
      if (mat > 0) dpad += vb[192 + (mat - 1) * 64 + row];
    }
  fb_unfold_rows(a, slice, mat, head, s, dc, dpad, red);
}

// one block, 512 threads: eight 64-vectors
__global__ __launch_bounds__(512) void fb_unfold2_kernel(Unfold2Args a) {
  fb_unfold2_vec(a, threadIdx.x >> 6, threadIdx.x & 63);
}

// dZ0 = ( LNbwd_noaffine( sum_h dxh[h] ) + dXs ) * (1 - X^2)     (Modules.py:519-521 backward, :270 tanh')
__global__ __launch_bounds__(256) void lnhat_bwd_kernel(const float* __restrict__ X, const float* __restrict__ dxh, int64_t tcap,
                                                        const float* __restrict__ dxpad, const float* __restrict__ dXs,
                                                        float* __restrict__ dZ0, const int32_t* __restrict__ count, int nslab) {
  const int T = count[0];
  const int64_t t = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int c4 = (threadIdx.x & 15) * 4;
  if (t >= T) return;
  const float4 xv = *reinterpret_cast<const float4*>(X + t * 64 + c4);
  float m, rs;
  ln_row16(xv, m, rs);
  const float4 xh = make_float4((xv.x - m) * rs, (xv.y - m) * rs, (xv.z - m) * rs, (xv.w - m) * rs);
  float4 d;
  if (t < T - 1) {
    d = *reinterpret_cast<const float4*>(dxh + t * 64 + c4);
    for (int hd = 1; hd < nslab; ++hd) {
      const float4 v = *reinterpret_cast<const float4*>(dxh + ((int64_t)hd * tcap + t) * 64 + c4);
      d.x += v.x; d.y += v.y; d.z += v.z; d.w += v.w;
    }
  } else {
    d = *reinterpret_cast<const float4*>(dxpad + c4);
  }
  const float a = group_sum<16>((d.x + d.y) + (d.z + d.w)) * (1.f / 64.f);
  const float b = group_sum<16>((d.x * xh.x + d.y * xh.y) + (d.z * xh.z + d.w * xh.w)) * (1.f / 64.f);
  const float4 s = *reinterpret_cast<const float4*>(dXs + t * 64 + c4);
  float4 o;
  o.x = (rs * (d.x - a - xh.x * b) + s.x) * (1.f - xv.x * xv.x);
  o.y = (rs * (d.y - a - xh.y * b) + s.y) * (1.f - xv.y * xv.y);
  o.z = (rs * (d.z - a - xh.z * b) + s.z) * (1.f - xv.z * xv.z);
  o.w = (rs * (d.w - a - xh.w * b) + s.w) * (1.f - xv.w * xv.w);
  *reinterpret_cast<float4*>(dZ0 + t * 64 + c4) = o;
}

int chunks_for(int ntiles) {
  const int cus = device_cu_count();
  int c = cus / MATCHA_N_HEAD;
  if (c > kMaxChunks) c = kMaxChunks;
  if (c > ntiles) c = ntiles;
  return c < 1 ? 1 : c;
}

}  // namespace

const float* fused_bwd_dxpad(const float* ws) { return ws + (size_t)MATCHA_N_HEAD * kMaxChunks * kWgSlab + 32 * 3 * 3 * 64; }

size_t fused_bwd_ws_floats(int64_t B, int L) {
  (void)B; (void)L;
  return (size_t)MATCHA_N_HEAD * kMaxChunks * kWgSlab + (size_t)32 * 3 * 3 * 64 + 64;
}

// merged heads: fused_bwdh_kernel -> fbm_chain_kernel -> the LayerNorm un-folding of launch_fused_bwd (one slab per head)
int launch_fused_bwd_merged(const matcha_tensors& p, const Ragged& rg, int64_t B, int L, const FusedBwdLaunch& a, matcha_tensors& grads, hipStream_t st) {
  const int64_t tcap = B * L + 1;
  const float *folded = a.folded, *X = a.x.X, *xhatN = a.x.xhat, *rn = a.x.rn, *vn = a.x.vn, *dXs = a.dXs;
  const int32_t* xrow = a.x.xrow;
  const bool dx_atomic = a.dx_atomic;
  float *dxh = a.dxh, *ws = a.ws;
  MATCHA_CHECK_ARG(!xrow || xhatN, "fused backward: the node route needs the table of normalised rows");
  MATCHA_CHECK_ARG(!rn || xrow, "fused backward: the r table belongs to the node route");
  MATCHA_CHECK_ARG(!vn || rn, "fused backward: the value table needs the r table");
  MATCHA_CHECK_ARG(!a.dx_node || (vn && dx_atomic && a.dx_zeroed), "fused backward: per-node d x_hat sums need the value table, the atomics and a caller that zeroed them");
  MATCHA_CHECK_ARG(!a.dx_node || a.x.rows * 256 < ((int64_t)1 << 31), "fused backward: a head's replica of the per-node sums is addressed through a buffer descriptor of < 2^31 bytes");
  if (dx_atomic && !a.dx_zeroed) MATCHA_TRY(zero_async(dxh, (size_t)tcap * 64 * sizeof(float), st));
  int nchunks = 2 * chunks_for(rg.nhalves);                  // two four-wave workgroups per CU
  if (nchunks > kMaxChunks) nchunks = kMaxChunks;
  if (nchunks > rg.nhalves) nchunks = rg.nhalves > 0 ? rg.nhalves : 1;
  float* wslab = ws;                                                         // [8][nchunks][kWgSlabM]
  float* chain = ws + (size_t)MATCHA_N_HEAD * kMaxChunks * kWgSlabM;         // [8][kWgSlab]  (both inside the four-product kernel's slab area)
  float* part = ws + (size_t)MATCHA_N_HEAD * kMaxChunks * kWgSlab;
  float* dxpad = part + 32 * 3 * 3 * 64;
  const size_t wsz = (size_t)MATCHA_N_HEAD * 64 * 64, csz = (size_t)MATCHA_N_HEAD * 64;
  const MergedView mv = merged_view(a.merged);
  {
    FusedBwdHArgs g;
    g.X = xrow ? xhatN : X; g.dDyn = a.dDyn; g.count = rg.count; g.half_meta = rg.half_meta; g.tok_pos = rg.tok_pos; g.L = L; g.nhalves = rg.nhalves; g.nchunks = nchunks;
    g.mB = mv.B; g.mM = mv.M; g.dxh = dxh; g.tcap = tcap; g.dx_atomic = dx_atomic ? 1 : 0; g.wslab = wslab; g.rimg = a.rimg; g.xrow = xrow;
    g.rn = rn; g.rn_head = a.x.rows * 64; g.vn = vn; g.dx_node = a.dx_node ? dxh : nullptr;
    const size_t lds = kBwdLdsBytes;
    auto launch = [&](auto kfn) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
      hipLaunchKernelGGL(kfn, dim3(MATCHA_N_HEAD * nchunks), dim3(256), lds, st, g);
    };
    // algorithmic flops: the reference's formulation -- 8 heads x 8 GEMMs of 2*64*64 per token; this kernel EXECUTES half of them
    ProfScope ps(MATCHA_PROF_FUSED_BWD, (double)tcap * MATCHA_N_HEAD * 8.0 * 2.0 * 64.0 * 64.0, st);
    // ROUND-5 FINDING, kept here because it is a property of how this file must be built: compiled with the SLP vectoriser, the ML = 5 instance
    // produced TIMING-DEPENDENT dR rows for hyperedges of exactly 5 nodes when two workgroups shared a CU (~20-120 of 512 workgroups per launch
    // off by 1e-4 of dB_h; never with one workgroup per CU, never for k < 5, never with ML = 6 on the same batch; tools/debug/bwd_slab_diff.py,
    // probes in DESIGN.md 4.1c).  hipcc packs the leftover fifth iteration of the row phase's key loop into v_pk_*_f32 chains whose halves
    // interleave the sig accumulation with the DPP reduction of d_4.  Extra barriers, nops behind the MFMAs and in front of the DPP steps,
    // plain shuffles and unpinned loads did not cure it; -fno-slp-vectorize (no packed f32 in that loop) does -- 0 differing workgroups in
    // every run -- and is faster.  The Makefile sets the flag for the whole library; tests/test_hip_properties.py::test_full_size_train_step_is_reproducible
    // is the run-time guard.
    dispatch_ml(L, [&](auto ml) {       // <ML, NODE, VTAB>: per token, per node, per node with the value table
      constexpr int ML = decltype(ml)::value;
      if (vn) launch(fused_bwdh_kernel<ML, true, true>); else if (xrow) launch(fused_bwdh_kernel<ML, true>); else launch(fused_bwdh_kernel<ML, false>);
    });
    MATCHA_CHECK_LAUNCH("fused_bwdh_kernel");
  }
  {
    ChainArgs c;
    c.wslab = wslab; c.nchunks = nchunks; c.red = chain + (size_t)MATCHA_N_HEAD * kWgSlab;
    c.wq = folded; c.wk = folded + wsz; c.wv = folded + 2 * wsz; c.cq = folded + 3 * wsz; c.cv = c.cq + 2 * csz;
    c.fc1_w = p.fc1_w; c.out = chain; c.dxpad = dxpad;
    TailReduceArgs tl;
    if (a.tail) tl = *a.tail; else memset(&tl, 0, sizeof(tl));
    const int tail_blocks = a.tail ? kTailRoleBlocks : 0;
    hipLaunchKernelGGL(fbm_reduce_kernel, dim3((unsigned)(kFbmReduceBlocks + tail_blocks)), dim3(256), 0, st, c, tl, tail_blocks);
    MATCHA_CHECK_LAUNCH("fbm_reduce_kernel");
    UnfoldArgs u;
    u.wslab = chain; u.nchunks = 1; u.X = X; u.count = rg.count; u.x_pad_row0 = xrow ? 1 : 0;
    u.W[0] = p.w_q; u.W[1] = p.w_k; u.W[2] = p.w_v;
    u.g[0] = p.ln_q_g; u.g[1] = p.ln_k_g; u.g[2] = p.ln_v_g;
    u.b[0] = p.ln_q_b; u.b[1] = p.ln_k_b; u.b[2] = p.ln_v_b;
    u.gW[0] = grads.w_q; u.gW[1] = grads.w_k; u.gW[2] = grads.w_v; u.gfc1 = grads.fc1_w;
    u.part = part;
    // paired (the step's record): the chain rule's blocks un-fold their own rows -- no fb_unfold_kernel launch;  unfold2 != null on top of it: the
    // final vectors ride in the caller's node_scatter launch, which reads dxpad -- so the chain launch leaves dxpad final (fbm_chain_kernel says why it can)
    MATCHA_CHECK_ARG(!a.unfold2 || a.paired, "fused backward: handing the final vectors on belongs to the paired launches");
    hipLaunchKernelGGL(fbm_chain_kernel, dim3(4, 4, MATCHA_N_HEAD), dim3(256), 0, st, c, u, a.paired ? 1 : 0, a.unfold2 ? 1 : 0);
    MATCHA_CHECK_LAUNCH("fbm_chain_kernel");
    if (!a.paired) {
      hipLaunchKernelGGL(fb_unfold_kernel, dim3(4, 4, MATCHA_N_HEAD), dim3(256), 0, st, u);
      MATCHA_CHECK_LAUNCH("fb_unfold_kernel");
    }
    Unfold2Args b;
    b.part = part; b.wslab = chain; b.nchunks = 1;
    b.dg[0] = grads.ln_q_g; b.dg[1] = grads.ln_k_g; b.dg[2] = grads.ln_v_g;
    b.db[0] = grads.ln_q_b; b.db[1] = grads.ln_k_b; b.db[2] = grads.ln_v_b;
    b.dfc1_b = grads.fc1_b; b.dxpad = dxpad; b.dxpad_add = a.unfold2 ? 2 : 1;
    if (a.unfold2) {
      *a.unfold2 = b;
    } else {
      hipLaunchKernelGGL(fb_unfold2_kernel, dim3(1), dim3(512), 0, st, b);
      MATCHA_CHECK_LAUNCH("fb_unfold2_kernel");
    }
  }
  if (float* dZ0 = a.dZ0) {
    MATCHA_CHECK_ARG(!xrow, "fused backward: the node route has no dZ0 output");
    hipLaunchKernelGGL(lnhat_bwd_kernel, dim3((unsigned)cdiv(tcap, 16)), dim3(256), 0, st, X, dxh, tcap, dxpad, dXs, dZ0, rg.count, dx_atomic ? 1 : MATCHA_N_HEAD);
    MATCHA_CHECK_LAUNCH("lnhat_bwd_kernel");
  }
  return MATCHA_OK;
}

}  // namespace matcha
