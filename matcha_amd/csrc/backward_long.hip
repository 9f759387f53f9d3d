// matcha_backward_long: the backward of matcha_forward_long_train (forward_long.hip) for rows of up to MATCHA_MAX_LONG_L = 32 columns.
//
// It is the layer-by-layer chain of matcha_backward (model.hip, backward_impl) on the long rows' training layout (forward_long.hpp): head_bwd,
// the TN / NN GEMMs with their dropout epilogues, ln3_bwd, the next_w / attribute_nn products, embed_scatter and adj_backward work on token
// rows and the plan's device-side token count and do not care about L.  What is bound to L <= 8 there, the attention backward, is
// attention_long_bwd.hip here.  Both head formulations: merged where the forward ran it (its record says), the four products otherwise.
#include <string.h>

#include "forward_long.hpp"

using namespace matcha;

extern "C" int matcha_backward_long(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen, const matcha_step_opts* opts,
                                    const int64_t* x, int64_t B, int32_t L, const float* dlogits, const float* drecon, matcha_tensors* grads,
                                    int32_t* touched, void* ws, size_t ws_bytes, matcha_stream_t stream) {
  MATCHA_TRY(check_shape_long(shp, B, L, "matcha_backward_long"));
  MATCHA_CHECK_ARG(params && frozen && opts && x && ws && grads && dlogits, "matcha_backward_long: null pointer (dlogits is required)");
  MATCHA_CHECK_ARG(!opts->deterministic && !opts->sparse_table_grad && !opts->loss_in_forward && !opts->random_chrom_dev,
                   "matcha_backward_long: opts->deterministic, sparse_table_grad, loss_in_forward and random_chrom_dev belong to the L <= %d step", MATCHA_MAX_L);
  MATCHA_CHECK_ARG(frozen->attr_table, "matcha_backward_long: the attribute_nn backward gathers attr_table rows (also under attr_mode 1)");
  const matcha_shape& s = *shp;
  const matcha_tensors& p = *params;
  matcha_tensors& g_ = *grads;
  MATCHA_CHECK_ARG(s.mode == 1 || g_.table, "matcha_backward_long: table mode without a table gradient buffer");
  bool merged = false;
  {
    // the size is checked against both formulations' layouts before the record is consumed: a refusal leaves the forward's record in place
    LongTrainWs probe;
    const size_t least = carve_long_train(s, B, L, nullptr, probe, true);
    if (ws_bytes < least) { set_error("matcha_backward_long: workspace %zu < %zu bytes", ws_bytes, least); return MATCHA_ENOMEM; }
  }
  MATCHA_CHECK_ARG(long_take_forward(ws, &merged),
                   "matcha_backward_long: no matcha_forward_long_train on record for this workspace (one backward per forward, same ws pointer)");
  LongTrainWs w;
  const size_t need = carve_long_train(s, B, L, (char*)ws, w, merged);
  if (ws_bytes < need) { set_error("matcha_backward_long: workspace %zu < %zu bytes", ws_bytes, need); return MATCHA_ENOMEM; }
  hipStream_t st = (hipStream_t)stream;
  const int64_t Tn = B * L + 1;
  const int d = s.d;
  const int64_t hd = (int64_t)MATCHA_N_HEAD * d;
  const bool train = opts->training != 0;
  const bool drop_fc1 = train && opts->p_drop_fc1 > 0.f, drop_pff = train && opts->p_drop_pff > 0.f;
  const int32_t* cnt = w.rg.count;             // the plan (row_off, tok_id, tok_slot, count) is still in the workspace
  const int64_t* ids = w.rg.tok_id;

  // tail: dH2, dXs and the gradients of pff_n1.layer_norm, layer_norm1/2, pff_classifier
  HeadParams hp = {p.pff_ln_g, p.pff_ln_b, p.ln1_g, p.ln1_b, p.ln2_g, p.ln2_b, p.cls_w, p.cls_b};
  HeadParams ghp = {g_.pff_ln_g, g_.pff_ln_b, g_.ln1_g, g_.ln1_b, g_.ln2_g, g_.ln2_b, g_.cls_w, g_.cls_b};
  MATCHA_TRY(launch_head_bwd(w.rg.row_off, w.H2, w.X, B, L, d, hp, nullptr, nullptr, w.logits, dlogits, opts->alpha, w.dH2, w.dXs, w.slab, ghp, st));
  // pff_n1 conv1: dW1 += dH2^T H1 ; db1 += colsum(dH2) ; dZ1 = (dH2 W1) * dropmask * (1 - tanh^2)
  MATCHA_TRY(launch_gemm_tn(w.dH2, w.H1, g_.pff1_w, g_.pff1_b, d, d, Tn, d, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, st, cnt));
  {
    GemmArgs g = gemm_long(w.rg, w.dH2, p.pff1_w, w.dZ1, Tn, d, d, true);
    g.flags = MATCHA_EPI_DTANH; g.aux = w.H1;
    if (drop_pff) { g.flags |= MATCHA_EPI_DROPOUT; g.seed = opts->seed; g.stream_id = kStreamDropPff; g.p_drop = opts->p_drop_pff; g.aux_scale = 1.f - opts->p_drop_pff; }
    MATCHA_TRY(launch_gemm_rm(true, g, st));
  }
  // pff_n1 conv0: dW0 += dZ1^T Y ; ddyn0 = (dZ1 W0 + dH2[residual]) * dropmask_fc1 * non_pad
  MATCHA_TRY(launch_gemm_tn(w.dZ1, w.Y, g_.pff0_w, g_.pff0_b, d, d, Tn, d, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, st, cnt));
  {
    GemmArgs g = gemm_long(w.rg, w.dZ1, p.pff0_w, w.ddyn0, Tn, d, d, true);
    g.flags = MATCHA_EPI_RESIDUAL | MATCHA_EPI_ROWMASK; g.residual = w.dH2; g.row_ids = ids;
    if (drop_fc1) { g.flags |= MATCHA_EPI_DROPOUT; g.seed = opts->seed; g.stream_id = kStreamDropFc1; g.p_drop = opts->p_drop_fc1; }
    MATCHA_TRY(launch_gemm_rm(true, g, st));
  }
  if (merged) {
    // merged heads: dM_all = ddyn0^T Z ; d fc1_b += colsum ; dZ = ddyn0 M_all (the scratch gradients start from zero: the TN GEMM accumulates)
    MATCHA_TRY(zero_async(w.lwdM, (size_t)hd * d * sizeof(float), st));
    MATCHA_TRY(zero_async(w.lwdB, (size_t)hd * d * sizeof(float), st));
    MATCHA_TRY(launch_gemm_tn(w.ddyn0, w.O, w.lwdM, g_.fc1_b, d, hd, Tn, d, hd, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, st, cnt));
    {
      GemmArgs g = gemm_long(w.rg, w.ddyn0, w.lwM, w.dO, Tn, hd, d, true);
      MATCHA_TRY(launch_gemm_rm(true, g, st));
    }
    // attention backward on the shared key / value rows: dR per head, d kin / d vin = the sums over the heads, added inside the kernel
    MATCHA_TRY(launch_attn_long_bwd(w.Q, w.kin, w.vin, w.dO, w.rg.row_off, B, L, d, d, 0, w.dQ, w.dkin, w.dvin, w.slab, st));
    // dB_all = dR^T qin ; dqin = dR B_all ; then the chain rule to w_qs / w_ks / w_vs / fc1
    MATCHA_TRY(launch_gemm_tn(w.dQ, w.qin, w.lwdB, nullptr, hd, d, Tn, hd, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, st, cnt));
    {
      GemmArgs g = gemm_long(w.rg, w.dQ, w.lwB, w.dqin, Tn, d, hd, true);
      MATCHA_TRY(launch_gemm_rm(true, g, st));
    }
    const int64_t dd = (int64_t)d * d;
    const BmmProduct pr[4] = {
        {p.w_k, d, 1, dd, w.lwdB, d, 1, dd, g_.w_q, d, dd, 1},                   // dW_q[h][m][b] += sum_a W_k[h][m][a] dB_h[a][b]
        {p.w_q, d, 1, dd, w.lwdB, 1, d, dd, g_.w_k, d, dd, 1},                   // dW_k[h][m][a] += sum_b W_q[h][m][b] dB_h[a][b]
        {w.lwdM, hd, 1, d, p.w_v, 1, d, dd, g_.fc1_w, hd, d, 1},                 // dWfc1[n][h d + m] += sum_b dM[n][h d + b] W_v[h d + m][b]
        {p.fc1_w, 1, hd, d, w.lwdM, hd, 1, d, g_.w_v, d, dd, 1}};                // dW_v[h][m][b] += sum_n Wfc1[n][h d + m] dM[n][h d + b]
    MATCHA_TRY(launch_bmm_heads(pr, 4, d, st));
  } else {
    // fc1: dW += ddyn0^T O ; db += colsum ; dO = ddyn0 Wfc1
    MATCHA_TRY(launch_gemm_tn(w.ddyn0, w.O, g_.fc1_w, g_.fc1_b, d, hd, Tn, d, hd, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, st, cnt));
    {
      GemmArgs g = gemm_long(w.rg, w.ddyn0, p.fc1_w, w.dO, Tn, hd, d, true);
      MATCHA_TRY(launch_gemm_rm(true, g, st));
    }
    MATCHA_TRY(launch_attn_long_bwd(w.Q, w.K, w.V, w.dO, w.rg.row_off, B, L, d, hd, d, w.dQ, w.dK, w.dV, w.slab, st));
    // Q / K / V projections: dW += dQ^T qin ; dqin = dQ Wq  (batched x3)
    MATCHA_TRY(launch_gemm_tn(w.dQ, w.qin, g_.w_q, nullptr, hd, d, Tn, hd, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, st, cnt));
    MATCHA_TRY(launch_gemm_tn(w.dK, w.kin, g_.w_k, nullptr, hd, d, Tn, hd, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, st, cnt));
    MATCHA_TRY(launch_gemm_tn(w.dV, w.vin, g_.w_v, nullptr, hd, d, Tn, hd, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, st, cnt));
    {
      GemmArgs g = gemm_long(w.rg, w.dQ, p.w_q, w.dqin, Tn, d, hd, true);
      g.A[1] = w.dK; g.B[1] = p.w_k; g.C[1] = w.dkin;
      g.A[2] = w.dV; g.B[2] = p.w_v; g.C[2] = w.dvin;
      g.batch = 3;
      MATCHA_TRY(launch_gemm_rm(true, g, st));
    }
  }
  // LayerNorm x3 backward + static-branch gradient + tanh'
  MATCHA_TRY(launch_ln3_bwd(w.X, w.dqin, w.dkin, w.dvin, w.dXs, Tn, d, p.ln_q_g, p.ln_k_g, p.ln_v_g, w.dZ0, w.slab, g_.ln_q_g, g_.ln_q_b, g_.ln_k_g,
                            g_.ln_k_b, g_.ln_v_g, g_.ln_v_b, st, cnt));
  if (opts->encoder_done_event && hipEventRecord((hipEvent_t)opts->encoder_done_event, st) != hipSuccess) {
    set_error("matcha_backward_long: recording encoder_done_event failed"); return MATCHA_EHIP;
  }
  // next_w: dW += dZ0^T x0 ; db += colsum ; dX0 = dZ0 Wn
  MATCHA_TRY(launch_gemm_tn(w.dZ0, w.x0, g_.next_w, g_.next_b, d, d, Tn, d, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, st, cnt));
  {
    GemmArgs g = gemm_long(w.rg, w.dZ0, p.next_w, w.dX0, Tn, d, d, true);
    MATCHA_TRY(launch_gemm_rm(true, g, st));
  }
  // attribute_nn: dWa += dX0^T attr_table[id] ; dba += colsum(dX0)
  MATCHA_TRY(launch_gemm_tn(w.dX0, frozen->attr_table, g_.attr_w, g_.attr_b, d, s.n_attr, Tn, d, frozen->attr_ld > 0 ? frozen->attr_ld : s.n_attr, ids, true,
                            w.gemm_ws, w.gemm_ws_bytes, st, cnt));
  // node embedding
  if (s.mode == 0) {
    MATCHA_TRY(launch_embed_scatter(ids, Tn, d, w.dX0, g_.table, st, cnt));
    if (touched) MATCHA_TRY(launch_fill_i32(touched, 2, 1, st));
  } else {
    MATCHA_TRY(adj_backward(s, p, *frozen, *opts, ids, Tn, w.dX0, drecon, g_, touched, w.adj_ws, w.adj_ws_bytes, w.gemm_ws, w.gemm_ws_bytes, st, w.rg.tok_slot));
  }
  return MATCHA_OK;
}
