// The layer-by-layer token chain (layerwise.hpp): Classifier.forward (Modules.py:278-318) and its backward as a fixed sequence of kernel
// launches on the caller's stream -- no allocation, no host synchronisation, so a step stays hipGraph-capturable.  Every product of the chain
// is written here and nowhere else; model.hip and forward_long.hip bring the layout, the plan and the record and call the pieces.
#include <string.h>

#include <mutex>

#include "layerwise.hpp"

namespace matcha {

GemmArgs gemm1(const TokenChain& w, const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K, bool b_kn) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A[0] = A; g.B[0] = B; g.C[0] = C; g.batch = 1;
  g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = b_kn ? N : K; g.ldc = N;
  g.aux_scale = 1.f;
  g.m_dev = w.rg.count;            // true token count (Tr + 1) lives on the device
  g.rng_row_map = w.rg.tok_slot;   // dropout counters follow the original [B, L] slots
  return g;
}

// B_all[h d + a][b] = sum_m W_k[h d + m][a] W_q[h d + m][b];   M_all[n][h d + b] = sum_m Wfc1[n][h d + m] W_v[h d + m][b]   (16 small GEMMs)
int merged_weights(const matcha_shape& s, const matcha_tensors& p, const TokenChain& w, hipStream_t st) {
  const int64_t d = s.d, hd = (int64_t)MATCHA_N_HEAD * d;
  // both products, all heads, one launch (bmm_heads.hip; every embed_dim the merged heads take is a multiple of 64)
  const BmmProduct pr[2] = {
      {p.w_k, 1, d, d * d, p.w_q, d, 1, d * d, w.lwB, d, d * d, 0},            // B_h[a][b] = sum_m W_k[h d + m][a] W_q[h d + m][b]
      {p.fc1_w, hd, 1, d, p.w_v, d, 1, d * d, w.lwM, hd, d, 0}};               // M_all[n][h d + b] = sum_m Wfc1[n][h d + m] W_v[h d + m][b]
  return launch_bmm_heads(pr, 2, s.d, st);
}
// chain rule from dB_all, dM_all to the projections (accumulating):  dW_q[h] += W_k[h] dB_h;  dW_k[h] += W_q[h] dB_h^T;
//   dWfc1[:, h] += dM_h W_v[h]^T;  dW_v[h] += Wfc1[:, h]^T dM_h
int merged_chain(const matcha_shape& s, const matcha_tensors& p, matcha_tensors& g_, const TokenChain& w, hipStream_t st) {
  const int64_t d = s.d, hd = (int64_t)MATCHA_N_HEAD * d;
  const BmmProduct pr[4] = {
      {p.w_k, d, 1, d * d, w.lwdB, d, 1, d * d, g_.w_q, d, d * d, 1},          // dW_q[h][m][b] += sum_a W_k[h][m][a] dB_h[a][b]
      {p.w_q, d, 1, d * d, w.lwdB, 1, d, d * d, g_.w_k, d, d * d, 1},          // dW_k[h][m][a] += sum_b W_q[h][m][b] dB_h[a][b]
      {w.lwdM, hd, 1, d, p.w_v, 1, d, d * d, g_.fc1_w, hd, d, 1},              // dWfc1[n][h d + m] += sum_b dM[n][h d + b] W_v[h d + m][b]
      {p.fc1_w, 1, hd, d, w.lwdM, hd, 1, d, g_.w_v, d, d * d, 1}};             // dW_v[h][m][b] += sum_n Wfc1[n][h d + m] dM[n][h d + b]
  return launch_bmm_heads(pr, 4, s.d, st);
}

void chain_scratch_bytes(const matcha_shape& s, int64_t B, int L, bool long_attn, TokenChain& w) {
  const int64_t Tn = B * L + 1, d = s.d, hd = (int64_t)MATCHA_N_HEAD * d;
  size_t sb = colsum_slab_bytes(Tn, 6, (int)d);
  size_t sb2 = colsum_slab_bytes(B, 7, (int)d);
  if (sb2 > sb) sb = sb2;
  sb2 = long_attn ? attn_long_bwd_slab_bytes(B, (int)d) : attn_bwd_slab_bytes(B, (int)d);
  if (sb2 > sb) sb = sb2;
  w.slab_bytes = sb;
  size_t gb = gemm_tn_ws_bytes(hd, d, Tn);                       // dWq / dWk / dWv, dB_all
  size_t g2 = gemm_tn_ws_bytes(d, hd, Tn); if (g2 > gb) gb = g2; // dfc1, dM_all
  g2 = gemm_tn_ws_bytes(d, d, Tn); if (g2 > gb) gb = g2;
  g2 = gemm_tn_ws_bytes(d, s.n_attr, Tn); if (g2 > gb) gb = g2;
  if (s.mode == 1) {   // recon head gradient [n_r, d] for any chromosome r: the slab count depends on ceil(n_r / 64)
    for (int64_t m = 64;; m += 64) {
      const int64_t mm = m < s.max_bins ? m : s.max_bins;
      g2 = gemm_tn_ws_bytes(mm, d, Tn); if (g2 > gb) gb = g2;
      if (mm >= s.max_bins) break;
    }
  }
  w.gemm_ws_bytes = gb;
}

int check_shape_fields(const matcha_shape* s, const char* fn) {
  char pre[96] = "";
  if (fn) snprintf(pre, sizeof(pre), "%s: ", fn);
  MATCHA_CHECK_ARG(s, "%snull shape", pre);
  MATCHA_CHECK_ARG(s->d >= 8 && s->d <= 256 && s->d % 8 == 0 && (s->d <= 64 || s->d % 64 == 0),
                   "%sembed_dim d=%d unsupported (multiples of 8 up to 64, then 128, 192, 256)", pre, s->d);
  MATCHA_CHECK_ARG(s->n_nodes >= 1, "%sn_nodes=%d must be >= 1", pre, s->n_nodes);
  MATCHA_CHECK_ARG(s->mode == 0 || s->mode == 1, "%smode=%d must be 0 (table) or 1 (adj)", pre, s->mode);
  MATCHA_CHECK_ARG(s->n_attr >= 1 && (size_t)s->n_attr * s->d * 4 <= 160 * 1024, "%sn_attr=%d does not fit the LDS staging", pre, s->n_attr);
  return MATCHA_OK;
}

int check_chain_params(const matcha_tensors& p, const matcha_frozen& f, const char* fn) {
  MATCHA_CHECK_ARG((f.attr_table || f.attr_mode == 1) && p.attr_w && p.attr_b && p.next_w && p.next_b && p.w_q && p.w_k && p.w_v && p.fc1_w &&
                       p.fc1_b && p.pff0_w && p.pff0_b && p.pff1_w && p.pff1_b && p.pff_ln_g && p.pff_ln_b && p.ln1_g && p.ln1_b &&
                       p.ln2_g && p.ln2_b && p.cls_w && p.cls_b && p.ln_q_g && p.ln_q_b && p.ln_k_g && p.ln_k_b && p.ln_v_g && p.ln_v_b,
                   "%s: a parameter pointer is null", fn);
  return MATCHA_OK;
}

int table_gradient(const matcha_shape& s, const matcha_step_opts& o, const TokenChain& w, int64_t Tn, matcha_tensors& g, hipStream_t st) {
  if (o.sparse_table_grad) return MATCHA_OK;
  if (!o.deterministic) return MATCHA_OK;                 // the front-end kernel already added the rows with float atomics
  return launch_table_grad(w.rg.tok_key, w.dX0, Tn, s.d, s.n_nodes, g.table, w.tg_ws, w.tg_ws_bytes, st);
}

int encoder_done(const matcha_step_opts& o, hipStream_t st, const char* fn) {
  if (o.encoder_done_event && hipEventRecord((hipEvent_t)o.encoder_done_event, st) != hipSuccess) {
    set_error("%s: recording encoder_done_event failed", fn); return MATCHA_EHIP;
  }
  return MATCHA_OK;
}

// (it found reads of uninitialised workspace rows)
__global__ void nan_count_kernel(const float* __restrict__ p, const int32_t* __restrict__ rows_dev, int64_t rows, int64_t width, int* __restrict__ out) {
  if (rows_dev) rows = *rows_dev;
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows * width; i += (int64_t)gridDim.x * blockDim.x)
    bad += isfinite(p[i]) ? 0 : 1;
  if (bad) atomicAdd(out, bad);
}
void nan_check(const char* name, const float* p, const int32_t* rows_dev, int64_t rows, int64_t width, hipStream_t st) {
  if (!options().debug_nan || !p) return;
  int* d = nullptr;
  int h = 0;
  if (hipMalloc(&d, sizeof(int)) != hipSuccess) return;
  (void)hipMemsetAsync(d, 0, sizeof(int), st);
  hipLaunchKernelGGL(nan_count_kernel, dim3(256), dim3(256), 0, st, p, rows_dev, rows, width, d);
  (void)hipMemcpyAsync(&h, d, sizeof(int), hipMemcpyDeviceToHost, st);
  (void)hipStreamSynchronize(st);
  (void)hipFree(d);
  fprintf(stderr, "[matcha nan-check] %-10s %d non-finite values in the valid rows\n", name, h);
}

// row *row_dev of a [rows, width] tensor = 0 (the shared padding token's row, whose index lives on the device)
__global__ __launch_bounds__(256) void long_zero_row_kernel(float* __restrict__ p, const int32_t* __restrict__ row_dev, int64_t width) {
  float* row = p + (int64_t)*row_dev * width;
  for (int64_t i = threadIdx.x; i < width; i += 256) row[i] = 0.f;
}
static int launch_long_zero_row(float* p, const int32_t* row_dev, int64_t width, hipStream_t st) {
  hipLaunchKernelGGL(long_zero_row_kernel, dim3(1), dim3(256), 0, st, p, row_dev, width);
  MATCHA_CHECK_LAUNCH("long_zero_row_kernel");
  return MATCHA_OK;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
// front end: node rows (K1) + attribute path (K6) + add (Modules.py:263-269), X = tanh(next_w(x0)) (:270)
int chain_front_fwd(const ChainCall& c, const TokenChain& w, float* recon_out, bool zero_recon) {
  const matcha_shape& s = c.s;
  const matcha_tensors& p = c.p;
  const int64_t Tn = c.Tn();
  const int d = s.d;
  if (s.mode == 0) {
    if (recon_out && zero_recon) MATCHA_TRY(zero_async(recon_out, 2 * sizeof(float), c.st));
  } else {
    MATCHA_TRY(adj_forward(s, p, c.f, c.o, w.rg.tok_id, Tn, w.node, recon_out, w.adj_ws, w.adj_ws_bytes, c.st, w.rg.count, w.rg.tok_slot));
  }
  MATCHA_TRY(launch_embed_fwd(w.rg.tok_id, Tn, d, s.mode == 0 ? p.table : nullptr, s.mode == 0 ? nullptr : w.node, c.f, s.n_attr, p.attr_w, p.attr_b, w.x0,
                              c.st, w.rg.count));
  GemmArgs g = gemm1(w, w.x0, p.next_w, w.X, Tn, d, d);
  g.flags = MATCHA_EPI_BIAS | MATCHA_EPI_TANH; g.bias[0] = p.next_b;
  MATCHA_TRY(launch_gemm_rm(false, g, c.st));
  nan_check("x0", w.x0, w.rg.count, 0, d, c.st);
  nan_check("X", w.X, w.rg.count, 0, d, c.st);
  return MATCHA_OK;
}

int chain_attn_fwd(const ChainCall& c, const TokenChain& w) {
  const matcha_shape& s = c.s;
  const matcha_tensors& p = c.p;
  const int64_t Tn = c.Tn(), B = c.B;
  const int d = s.d, L = c.L;
  const int64_t hd = (int64_t)MATCHA_N_HEAD * d;
  const int32_t* cnt = w.rg.count;
  const bool train = c.o.training != 0;
  // three LayerNorms on the same row (Modules.py:519-521), then the heads' projections (:527-529), one batched launch
  MATCHA_TRY(launch_ln3_fwd(w.X, Tn, d, p.ln_q_g, p.ln_q_b, p.ln_k_g, p.ln_k_b, p.ln_v_g, p.ln_v_b, w.qin, w.kin, w.vin, w.stats, c.st, cnt));
  if (c.c.merged) {
    MATCHA_TRY(merged_weights(s, p, w, c.st));
    GemmArgs g = gemm1(w, w.qin, w.lwB, w.Q, Tn, hd, d);                        // r = qin B_all^T  (in Q's buffer)
    MATCHA_TRY(launch_gemm_rm(false, g, c.st));
  } else {
    GemmArgs g = gemm1(w, w.qin, p.w_q, w.Q, Tn, hd, d);
    g.A[1] = w.kin; g.B[1] = p.w_k; g.C[1] = w.K;
    g.A[2] = w.vin; g.B[2] = p.w_v; g.C[2] = w.V;
    g.batch = 3;
    MATCHA_TRY(launch_gemm_rm(false, g, c.st));
  }
  nan_check("qin", w.qin, cnt, 0, d, c.st);
  nan_check("Q", w.Q, cnt, 0, hd, c.st);
  nan_check("K", w.K, cnt, 0, hd, c.st);
  nan_check("V", w.V, cnt, 0, hd, c.st);
  // merged heads: every head attends the shared rows kin / vin, O = Z = P . vin per head
  if (c.c.long_attn) {
    // (w.P, null in every long layout, is the caller's padded attention tensor when matcha_get_embedding_long set it: the kernel's other instance)
    if (c.c.merged) MATCHA_TRY(launch_attn_long(w.Q, w.kin, w.vin, w.rg.row_off, B, L, d, d, 0, w.O, c.st, w.mask, w.P));
    else MATCHA_TRY(launch_attn_long(w.Q, w.K, w.V, w.rg.row_off, B, L, d, hd, d, w.O, c.st, w.mask, w.P));
    // that attention writes the real tokens' O rows only.  The padding token's row feeds fc1 under a row mask -- which selects zero whatever
    // finite row stands there (without `keep`: the projection's) -- and, with a backward, dM / dWfc1 as a factor of a zero gradient row
    if (c.c.keep) MATCHA_TRY(launch_long_zero_row(w.O, w.rg.row_off + B, hd, c.st));
  } else {
    if (c.c.merged) MATCHA_TRY(launch_attn_fwd(w.Q, w.kin, w.vin, w.rg.row_off, B, L, d, w.O, w.P, c.st, true));
    else MATCHA_TRY(launch_attn_fwd(w.Q, w.K, w.V, w.rg.row_off, B, L, d, w.O, w.P, c.st));
  }
  nan_check("O", w.O, cnt + 1, 0, hd, c.st);
  // Y = (dropout(fc1(O))) * non_pad_mask    (Modules.py:572, :614); the mask only zeroes the shared padding token's row
  GemmArgs g = gemm1(w, w.O, c.c.merged ? w.lwM : p.fc1_w, w.Y, Tn, d, hd);
  g.flags = MATCHA_EPI_BIAS | MATCHA_EPI_ROWMASK; g.bias[0] = p.fc1_b; g.row_ids = w.rg.tok_id;
  if (train && c.o.p_drop_fc1 > 0.f) { g.flags |= MATCHA_EPI_DROPOUT; g.seed = c.o.seed; g.stream_id = kStreamDropFc1; g.p_drop = c.o.p_drop_fc1; }
  return launch_gemm_rm(false, g, c.st);
}

int chain_tail_fwd(const ChainCall& c, const TokenChain& w, const float* y, const float* w_bce, float* logits, float* losses, int objective,
                   bool stop_before_head) {
  const matcha_tensors& p = c.p;
  const int64_t Tn = c.Tn();
  const int d = c.s.d;
  const bool train = c.o.training != 0;
  // pff_n1: H1 = dropout(tanh(conv0(Y)));  H2 = conv1(H1) + Y      (Modules.py:353-371)
  {
    GemmArgs g = gemm1(w, w.Y, p.pff0_w, w.H1, Tn, d, d);
    g.flags = MATCHA_EPI_BIAS | MATCHA_EPI_TANH; g.bias[0] = p.pff0_b;
    if (train && c.o.p_drop_pff > 0.f) { g.flags |= MATCHA_EPI_DROPOUT; g.seed = c.o.seed; g.stream_id = kStreamDropPff; g.p_drop = c.o.p_drop_pff; }
    MATCHA_TRY(launch_gemm_rm(false, g, c.st));
  }
  {
    GemmArgs g = gemm1(w, w.H1, p.pff1_w, w.H2, Tn, d, d);
    g.flags = MATCHA_EPI_BIAS | MATCHA_EPI_RESIDUAL; g.bias[0] = p.pff1_b; g.residual = w.Y;
    MATCHA_TRY(launch_gemm_rm(false, g, c.st));
  }
  nan_check("Y", w.Y, w.rg.count, 0, d, c.st);
  nan_check("H1", w.H1, w.rg.count, 0, d, c.st);
  nan_check("H2", w.H2, w.rg.count, 0, d, c.st);
  if (stop_before_head) return MATCHA_OK;
  // LayerNorms, (dynamic - static)^2, Conv1d(d -> 1), masked mean over the row's k real tokens / (k + 1e-15), the objective's loss
  // (Modules.py:373-374, :290-311; main.py:56)
  HeadParams hp = {p.pff_ln_g, p.pff_ln_b, p.ln1_g, p.ln1_b, p.ln2_g, p.ln2_b, p.cls_w, p.cls_b};
  MATCHA_TRY(launch_head_fwd(w.rg.row_off, w.H2, w.X, c.B, c.L, d, hp, y, w_bce, w.logits ? w.logits : logits, w.row_loss, losses, c.st, objective));
  if (w.logits && logits && hipMemcpyAsync(logits, w.logits, c.B * sizeof(float), hipMemcpyDeviceToDevice, c.st) != hipSuccess) {
    set_error("%s: logits copy failed", c.fn); return MATCHA_EHIP;
  }
  return MATCHA_OK;
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// tail: dH2, dXs and the gradients of pff_n1.layer_norm, layer_norm1/2, pff_classifier; then pff_n1's two convolutions
int chain_tail_bwd(const ChainCall& c, const TokenChain& w, const float* X, const int32_t* xrow, const float* y, const float* w_bce, const float* dlogits,
                   int objective, matcha_tensors& g_) {
  const matcha_tensors& p = c.p;
  const int64_t Tn = c.Tn();
  const int d = c.s.d;
  const int32_t* cnt = w.rg.count;             // the plan (row_off, tok_id, tok_slot, count) is still in the workspace
  const bool train = c.o.training != 0;
  const bool drop_fc1 = train && c.o.p_drop_fc1 > 0.f, drop_pff = train && c.o.p_drop_pff > 0.f;
  HeadParams hp = {p.pff_ln_g, p.pff_ln_b, p.ln1_g, p.ln1_b, p.ln2_g, p.ln2_b, p.cls_w, p.cls_b};
  HeadParams ghp = {g_.pff_ln_g, g_.pff_ln_b, g_.ln1_g, g_.ln1_b, g_.ln2_g, g_.ln2_b, g_.cls_w, g_.cls_b};
  MATCHA_TRY(launch_head_bwd(w.rg.row_off, w.H2, X, c.B, c.L, d, hp, y, w_bce, w.logits, dlogits, c.o.alpha, w.dH2, w.dXs, w.slab, ghp, c.st, objective, xrow));
  // pff_n1 conv1: dW1 += dH2^T H1 ; db1 += colsum(dH2) ; dZ1 = (dH2 W1) * dropmask * (1 - tanh^2)
  MATCHA_TRY(launch_gemm_tn(w.dH2, w.H1, g_.pff1_w, g_.pff1_b, d, d, Tn, d, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, c.st, cnt));
  {
    GemmArgs g = gemm1(w, w.dH2, p.pff1_w, w.dZ1, Tn, d, d, true);
    g.flags = MATCHA_EPI_DTANH; g.aux = w.H1;
    if (drop_pff) { g.flags |= MATCHA_EPI_DROPOUT; g.seed = c.o.seed; g.stream_id = kStreamDropPff; g.p_drop = c.o.p_drop_pff; g.aux_scale = 1.f - c.o.p_drop_pff; }
    MATCHA_TRY(launch_gemm_rm(true, g, c.st));
  }
  // pff_n1 conv0: dW0 += dZ1^T Y ; ddyn0 = (dZ1 W0 + dH2[residual]) * dropmask_fc1 * non_pad
  MATCHA_TRY(launch_gemm_tn(w.dZ1, w.Y, g_.pff0_w, g_.pff0_b, d, d, Tn, d, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, c.st, cnt));
  GemmArgs g = gemm1(w, w.dZ1, p.pff0_w, w.ddyn0, Tn, d, d, true);
  g.flags = MATCHA_EPI_RESIDUAL | MATCHA_EPI_ROWMASK; g.residual = w.dH2; g.row_ids = w.rg.tok_id;
  if (drop_fc1) { g.flags |= MATCHA_EPI_DROPOUT; g.seed = c.o.seed; g.stream_id = kStreamDropFc1; g.p_drop = c.o.p_drop_fc1; }
  return launch_gemm_rm(true, g, c.st);
}

int chain_attn_bwd(const ChainCall& c, const TokenChain& w, matcha_tensors& g_) {
  const matcha_shape& s = c.s;
  const matcha_tensors& p = c.p;
  const int64_t Tn = c.Tn(), B = c.B;
  const int d = s.d, L = c.L;
  const int64_t hd = (int64_t)MATCHA_N_HEAD * d;
  const int32_t* cnt = w.rg.count;
  if (c.c.merged) {
    // merged heads: dM_all = ddyn0^T Z ; d fc1_b += colsum ; dZ = ddyn0 M_all   (the scratch gradients start from zero: the TN GEMM
    // accumulates C and the column sums alike, and fc1_b's gradient must accumulate)
    MATCHA_TRY(zero_async(w.lwdM, (size_t)hd * d * sizeof(float), c.st));
    MATCHA_TRY(zero_async(w.lwdB, (size_t)hd * d * sizeof(float), c.st));
    MATCHA_TRY(launch_gemm_tn(w.ddyn0, w.O, w.lwdM, g_.fc1_b, d, hd, Tn, d, hd, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, c.st, cnt));
    {
      GemmArgs g = gemm1(w, w.ddyn0, w.lwM, w.dO, Tn, hd, d, true);
      MATCHA_TRY(launch_gemm_rm(true, g, c.st));
    }
    // attention backward on the shared key / value rows: dR per head in dQ; d kin / d vin = the sums over the heads, added inside the kernel
    // (the short kernel also leaves dK / dV per head; kin / vin themselves are read by it)
    if (c.c.long_attn) MATCHA_TRY(launch_attn_long_bwd(w.Q, w.kin, w.vin, w.dO, w.rg.row_off, B, L, d, d, 0, w.dQ, w.dkin, w.dvin, w.slab, c.st));
    else MATCHA_TRY(launch_attn_bwd(w.Q, w.kin, w.vin, w.P, w.dO, w.rg.row_off, B, L, d, w.dQ, w.dK, w.dV, w.slab, c.st, true, w.dkin, w.dvin));
    // dB_all = dR^T qin ; dqin = dR B_all ; then the chain rule to w_qs / w_ks / w_vs / fc1
    MATCHA_TRY(launch_gemm_tn(w.dQ, w.qin, w.lwdB, nullptr, hd, d, Tn, hd, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, c.st, cnt));
    {
      GemmArgs g = gemm1(w, w.dQ, w.lwB, w.dqin, Tn, d, hd, true);
      MATCHA_TRY(launch_gemm_rm(true, g, c.st));
    }
    MATCHA_TRY(merged_chain(s, p, g_, w, c.st));
  } else {
    // fc1: dW += ddyn0^T O ; db += colsum ; dO = ddyn0 Wfc1
    MATCHA_TRY(launch_gemm_tn(w.ddyn0, w.O, g_.fc1_w, g_.fc1_b, d, hd, Tn, d, hd, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, c.st, cnt));
    {
      GemmArgs g = gemm1(w, w.ddyn0, p.fc1_w, w.dO, Tn, hd, d, true);
      MATCHA_TRY(launch_gemm_rm(true, g, c.st));
    }
    if (c.c.long_attn) MATCHA_TRY(launch_attn_long_bwd(w.Q, w.K, w.V, w.dO, w.rg.row_off, B, L, d, hd, d, w.dQ, w.dK, w.dV, w.slab, c.st));
    else MATCHA_TRY(launch_attn_bwd(w.Q, w.K, w.V, w.P, w.dO, w.rg.row_off, B, L, d, w.dQ, w.dK, w.dV, w.slab, c.st));
    // Q / K / V projections: dW += dQ^T qin ; dqin = dQ Wq  (batched x3)
    MATCHA_TRY(launch_gemm_tn(w.dQ, w.qin, g_.w_q, nullptr, hd, d, Tn, hd, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, c.st, cnt));
    MATCHA_TRY(launch_gemm_tn(w.dK, w.kin, g_.w_k, nullptr, hd, d, Tn, hd, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, c.st, cnt));
    MATCHA_TRY(launch_gemm_tn(w.dV, w.vin, g_.w_v, nullptr, hd, d, Tn, hd, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, c.st, cnt));
    GemmArgs g = gemm1(w, w.dQ, p.w_q, w.dqin, Tn, d, hd, true);
    g.A[1] = w.dK; g.B[1] = p.w_k; g.C[1] = w.dkin;
    g.A[2] = w.dV; g.B[2] = p.w_v; g.C[2] = w.dvin;
    g.batch = 3;
    MATCHA_TRY(launch_gemm_rm(true, g, c.st));
  }
  // LayerNorm x3 backward + static-branch gradient + tanh'
  MATCHA_TRY(launch_ln3_bwd(w.X, w.dqin, w.dkin, w.dvin, w.dXs, Tn, d, p.ln_q_g, p.ln_k_g, p.ln_v_g, w.dZ0, w.slab, g_.ln_q_g, g_.ln_q_b, g_.ln_k_g,
                            g_.ln_k_b, g_.ln_v_g, g_.ln_v_b, c.st, cnt));
  return encoder_done(c.o, c.st, c.fn);
}

int chain_front_bwd(const ChainCall& c, const TokenChain& w, const float* drecon, matcha_tensors& g_, int32_t* touched) {
  const matcha_shape& s = c.s;
  const int64_t Tn = c.Tn();
  const int d = s.d;
  const int32_t* cnt = w.rg.count;
  const int64_t* ids = w.rg.tok_id;
  // next_w: dW += dZ0^T x0 ; db += colsum ; dX0 = dZ0 Wn
  MATCHA_TRY(launch_gemm_tn(w.dZ0, w.x0, g_.next_w, g_.next_b, d, d, Tn, d, d, nullptr, true, w.gemm_ws, w.gemm_ws_bytes, c.st, cnt));
  {
    GemmArgs g = gemm1(w, w.dZ0, c.p.next_w, w.dX0, Tn, d, d, true);
    MATCHA_TRY(launch_gemm_rm(true, g, c.st));
  }
  // attribute_nn: dWa += dX0^T attr_table[id] ; dba += colsum(dX0)
  MATCHA_CHECK_ARG(c.f.attr_table, "%s: the layer-by-layer attribute_nn backward gathers attr_table rows (also under attr_mode 1)", c.fn);
  MATCHA_TRY(launch_gemm_tn(w.dX0, c.f.attr_table, g_.attr_w, g_.attr_b, d, s.n_attr, Tn, d, c.f.attr_ld > 0 ? c.f.attr_ld : s.n_attr, ids, true,
                            w.gemm_ws, w.gemm_ws_bytes, c.st, cnt));
  // node embedding
  if (s.mode == 0) {
    MATCHA_CHECK_ARG(g_.table, "%s: table mode without a table gradient buffer", c.fn);
    if (c.o.deterministic || c.o.sparse_table_grad) MATCHA_TRY(table_gradient(s, c.o, w, Tn, g_, c.st));
    else MATCHA_TRY(launch_embed_scatter(ids, Tn, d, w.dX0, g_.table, c.st, cnt));
    if (touched) MATCHA_TRY(launch_fill_i32(touched, 2, 1, c.st));
    return MATCHA_OK;
  }
  return adj_backward(s, c.p, c.f, c.o, ids, Tn, w.dX0, drecon, g_, touched, w.adj_ws, w.adj_ws_bytes, w.gemm_ws, w.gemm_ws_bytes, c.st, w.rg.tok_slot);
}

// ---- the forward record ----------------------------------------------------------------------------------------------------------------
static std::mutex g_fwd_mu;
std::unordered_map<const void*, std::pair<StepRoute, uint64_t>> g_fwd_state;
static uint64_t g_fwd_clock = 0;
void note_forward(const void* ws, const StepRoute& route) {
  std::lock_guard<std::mutex> lk(g_fwd_mu);
  if (g_fwd_state.size() >= 4096 && g_fwd_state.find(ws) == g_fwd_state.end()) {
    auto old = g_fwd_state.begin();
    for (auto it = g_fwd_state.begin(); it != g_fwd_state.end(); ++it)
      if (it->second.second < old->second.second) old = it;
    g_fwd_state.erase(old);
  }
  g_fwd_state[ws] = std::make_pair(route, ++g_fwd_clock);
}
bool recorded_route(const void* ws, StepRoute& route) {
  std::lock_guard<std::mutex> lk(g_fwd_mu);
  auto it = g_fwd_state.find(ws);
  if (it != g_fwd_state.end()) route = it->second.first;
  return it != g_fwd_state.end();
}
void forget_forward(const void* ws) {
  std::lock_guard<std::mutex> lk(g_fwd_mu);
  g_fwd_state.erase(ws);
}

}  // namespace matcha
