// matcha_forward_long: the inference forward for LONG rows, x [B, L] with L <= MATCHA_MAX_LONG_L = 32 (include/matcha_hip.h).
//
// The token-level layers do not care about L: the front end, the three LayerNorms, the projections, fc1 and pff_n1 are the layer-by-layer
// kernels matcha_forward runs at embed_dim != 64 (model.hip), on the Tr real tokens + ONE shared padding token of the plan, and the classifier
// tail (head_fwd_kernel) walks a row's token range whatever its length.  What is bound to L <= 8 there has its long counterpart here: the
// plan (ragged_long.hip) and the attention (attention_long.hip).  embed_dim a multiple of 64 runs the merged heads (r = qin B_all^T, every
// head attends the shared rows kin / vin, dyn = Z M_all^T: model.hip, merged_weights), every other the reference's four products.
//
// Workspace: a forward-only layout.  Per token: the plan (20 B, and 8 B per row), X, three [d] rows that are reused along the chain -- x0 / qin / Y, kin / H1,
// vin / H2 -- the LayerNorm statistics and the heads' rows: r alone with merged heads, Q, K, V without; the attention writes O over Q in
// place.  That is 12 d floats per token merged (3 KB at embed_dim 64), 28 d otherwise (1.75 KB at embed_dim 16), + d in adj mode, against ~80 d
// of the training layout.
//
// matcha_forward_long_train is the same chain with every activation the backward needs kept (forward_long.hpp: LongTrainWs) and dropout through
// the GEMM epilogues; matcha_backward_long (backward_long.hip) consumes what it leaves.
#include <string.h>

#include <mutex>
#include <unordered_map>

#include "forward_long.hpp"

namespace matcha {

namespace {

struct LongWs {
  Ragged rg; uint32_t* mask;
  float *X, *a, *b, *c;          // a: x0, then qin, then Y;  b: kin, then H1;  c: vin, then H2
  float *stats, *Q, *K, *V;      // merged heads: Q holds r and K / V do not exist
  float *lwB, *lwM;              // merged heads: B_all [8 d, d], M_all [d, 8 d]
  float* node; void* adj_ws; size_t adj_ws_bytes;
};

size_t carve_long(const matcha_shape& s, int64_t B, int L, char* base, LongWs& w, bool merged) {
  const int64_t Tn = B * L + 1, d = s.d, hd = (int64_t)MATCHA_N_HEAD * d;
  size_t off = 0;
  auto take = [&](size_t n_floats) {
    float* p = base ? (float*)(base + off) : nullptr;
    off += align_up(n_floats * sizeof(float), 256);
    return p;
  };
  if (base) long_plan_carve(B, L, base, w.rg, &w.mask);
  off += align_up(long_plan_bytes(B, L), 256);
  w.X = take(Tn * d); w.a = take(Tn * d); w.b = take(Tn * d); w.c = take(Tn * d);
  w.stats = take(Tn * 2);
  w.Q = take(Tn * hd);
  w.K = take(merged ? 0 : Tn * hd); w.V = take(merged ? 0 : Tn * hd);
  w.lwB = take(merged ? (size_t)hd * d : 0); w.lwM = take(merged ? (size_t)hd * d : 0);
  w.node = take(s.mode == 1 ? Tn * d : 0);
  w.adj_ws_bytes = s.mode == 1 ? adj_workspace_bytes(s, Tn) : 0;
  w.adj_ws = take(w.adj_ws_bytes / sizeof(float));
  return off;
}

}  // namespace

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

bool long_merged(const matcha_shape& s) { return bmm_heads_supported(s.d) && !options().disable_merged; }

int check_shape_long(const matcha_shape* s, int64_t B, int32_t L, const char* fn) {
  MATCHA_CHECK_ARG(s, "%s: null shape", fn);
  MATCHA_CHECK_ARG(s->d >= 8 && s->d <= 256 && s->d % 8 == 0 && (s->d <= 64 || s->d % 64 == 0),
                   "%s: embed_dim d=%d unsupported (multiples of 8 up to 64, then 128, 192, 256)", fn, s->d);
  MATCHA_CHECK_ARG(L >= 2 && L <= MATCHA_MAX_LONG_L, "%s: L=%d outside 2..%d", fn, L, MATCHA_MAX_LONG_L);
  MATCHA_CHECK_ARG(B >= 1 && B * (int64_t)L < (1ll << 31) - 2, "%s: B=%lld must be >= 1 and B*L < 2^31 - 2", fn, (long long)B);
  // the layer-by-layer kernels put token tiles on grid.y (<= 65 535 tiles of 128 tokens): 8.38 M token rows is what they launch
  MATCHA_CHECK_ARG(B * (int64_t)L + 1 <= 65535ll * 128, "%s: B*L=%lld exceeds the %lld token rows the layer-by-layer kernels launch", fn,
                   (long long)(B * (int64_t)L), 65535ll * 128);
  MATCHA_CHECK_ARG(s->n_nodes >= 1, "%s: n_nodes=%d must be >= 1", fn, s->n_nodes);
  MATCHA_CHECK_ARG(s->mode == 0 || s->mode == 1, "%s: mode=%d must be 0 (table) or 1 (adj)", fn, s->mode);
  MATCHA_CHECK_ARG(s->n_attr >= 1 && (size_t)s->n_attr * s->d * 4 <= 160 * 1024, "%s: n_attr=%d does not fit the LDS staging", fn, s->n_attr);
  return MATCHA_OK;
}

GemmArgs gemm_long(const Ragged& rg, const float* A, const float* Bm, float* Cm, int64_t M, int64_t N, int64_t K, bool b_kn) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A[0] = A; g.B[0] = Bm; g.C[0] = Cm; g.batch = 1;
  g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = b_kn ? N : K; g.ldc = N;
  g.aux_scale = 1.f;
  g.m_dev = rg.count;            // true token count (Tr + 1) lives on the device
  g.rng_row_map = rg.tok_slot;
  return g;
}


size_t carve_long_train(const matcha_shape& s, int64_t B, int L, char* base, LongTrainWs& w, bool merged) {
  const int64_t Tn = B * L + 1, d = s.d, hd = (int64_t)MATCHA_N_HEAD * d;
  size_t off = 0;
  auto take = [&](size_t n_floats) {
    float* p = base ? (float*)(base + off) : nullptr;
    off += align_up(n_floats * sizeof(float), 256);
    return p;
  };
  if (base) long_plan_carve(B, L, base, w.rg, &w.mask);
  off += align_up(long_plan_bytes(B, L), 256);
  w.x0 = take(Tn * d); w.X = take(Tn * d); w.qin = take(Tn * d); w.kin = take(Tn * d); w.vin = take(Tn * d);
  w.stats = take(Tn * 2);
  w.Q = take(Tn * hd); w.K = take(merged ? 0 : Tn * hd); w.V = take(merged ? 0 : Tn * hd); w.O = take(Tn * hd);
  w.Y = take(Tn * d); w.H1 = take(Tn * d); w.H2 = take(Tn * d);
  w.logits = take(B);
  w.node = take(s.mode == 1 ? Tn * d : 0);
  w.dH2 = take(Tn * d); w.dXs = take(Tn * d); w.dZ1 = take(Tn * d); w.ddyn0 = take(Tn * d); w.dZ0 = take(Tn * d); w.dX0 = take(Tn * d);
  w.dO = w.O;                                   // dO takes O's place once the fc1 weight gradient has read it
  w.dQ = take(Tn * hd); w.dK = take(merged ? 0 : Tn * hd); w.dV = take(merged ? 0 : Tn * hd);
  w.dqin = take(Tn * d); w.dkin = take(Tn * d); w.dvin = take(Tn * d);
  size_t sb = colsum_slab_bytes(Tn, 6, (int)d);
  size_t sb2 = colsum_slab_bytes(B, 7, (int)d);
  if (sb2 > sb) sb = sb2;
  sb2 = attn_long_bwd_slab_bytes(B, (int)d);
  if (sb2 > sb) sb = sb2;
  w.slab_bytes = sb; w.slab = take(sb / sizeof(float));
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
  w.gemm_ws_bytes = gb; w.gemm_ws = take(gb / sizeof(float));
  w.adj_ws_bytes = s.mode == 1 ? adj_workspace_bytes(s, Tn) : 0;
  w.adj_ws = take(w.adj_ws_bytes / sizeof(float));
  const size_t nm = merged ? (size_t)hd * d : 0;
  w.lwB = take(nm); w.lwM = take(nm); w.lwdB = take(nm); w.lwdM = take(nm);
  return off;
}

namespace {
std::mutex g_long_mu;
std::unordered_map<const void*, std::pair<bool, uint64_t>> g_long_state;     // ws -> (merged, age)
uint64_t g_long_clock = 0;
}  // namespace
void long_note_forward(const void* ws, bool merged) {
  std::lock_guard<std::mutex> lk(g_long_mu);
  if (g_long_state.size() >= 4096 && g_long_state.find(ws) == g_long_state.end()) {
    auto old = g_long_state.begin();
    for (auto it = g_long_state.begin(); it != g_long_state.end(); ++it)
      if (it->second.second < old->second.second) old = it;
    g_long_state.erase(old);
  }
  g_long_state[ws] = std::make_pair(merged, ++g_long_clock);
}
bool long_take_forward(const void* ws, bool* merged) {
  std::lock_guard<std::mutex> lk(g_long_mu);
  auto it = g_long_state.find(ws);
  if (it == g_long_state.end()) return false;
  *merged = it->second.first;
  g_long_state.erase(it);
  return true;
}

}  // namespace matcha

using namespace matcha;

extern "C" size_t matcha_workspace_bytes_long(const matcha_shape* shp, int64_t B, int32_t L) {
  if (check_shape_long(shp, B, L, "matcha_workspace_bytes_long") != MATCHA_OK) return 0;
  LongWs w;
  // (follows the option table like matcha_workspace_bytes_forward: a forward under another disable_merged than its query is refused, MATCHA_ENOMEM)
  return carve_long(*shp, B, L, nullptr, w, long_merged(*shp));
}

extern "C" int matcha_forward_long(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen, const matcha_step_opts* opts,
                                   const int64_t* x, int64_t B, int32_t L, float* logits, float* losses, void* ws, size_t ws_bytes,
                                   matcha_stream_t stream) {
  MATCHA_TRY(check_shape_long(shp, B, L, "matcha_forward_long"));
  MATCHA_CHECK_ARG(params && frozen && opts && x && ws && logits, "matcha_forward_long: null pointer");
  MATCHA_CHECK_ARG(opts->training == 0 && opts->forward_only == 1,
                   "matcha_forward_long: long rows are inference-only (opts->training must be 0 and opts->forward_only 1; got %d, %d)",
                   (int)opts->training, (int)opts->forward_only);
  MATCHA_CHECK_ARG(!opts->random_chrom_dev, "matcha_forward_long: opts->random_chrom_dev needs the fused adj front end; pass opts->random_chrom");
  MATCHA_CHECK_ARG(((uintptr_t)ws) % 256 == 0, "matcha_forward_long: workspace must be 256-byte aligned");
  const matcha_shape& s = *shp;
  const matcha_tensors& p = *params;
  MATCHA_CHECK_ARG((frozen->attr_table || frozen->attr_mode == 1) && p.attr_w && p.attr_b && p.next_w && p.next_b && p.w_q && p.w_k && p.w_v && p.fc1_w &&
                       p.fc1_b && p.pff0_w && p.pff0_b && p.pff1_w && p.pff1_b && p.pff_ln_g && p.pff_ln_b && p.ln1_g && p.ln1_b &&
                       p.ln2_g && p.ln2_b && p.cls_w && p.cls_b && p.ln_q_g && p.ln_q_b && p.ln_k_g && p.ln_k_b && p.ln_v_g && p.ln_v_b,
                   "matcha_forward_long: a parameter pointer is null");
  MATCHA_CHECK_ARG(s.mode == 1 || p.table, "matcha_forward_long: table mode without table");
  const bool merged = long_merged(s);
  LongWs w;
  const size_t need = carve_long(s, B, L, (char*)ws, w, merged);
  if (ws_bytes < need) { set_error("matcha_forward_long: workspace %zu < %zu bytes", ws_bytes, need); return MATCHA_ENOMEM; }
  hipStream_t st = (hipStream_t)stream;
  const int64_t Tn = B * L + 1;                 // upper bound; the true count is *w.rg.count
  const int d = s.d;
  const int64_t hd = (int64_t)MATCHA_N_HEAD * d;
  const int32_t* cnt = w.rg.count;
  const int64_t* ids = w.rg.tok_id;

  { bool was; (void)long_take_forward(ws, &was); }      // (a training forward's record on this pointer is void: its activations are being overwritten)
  MATCHA_TRY(launch_long_plan(x, B, L, s.n_nodes, opts->status, w.rg, w.mask, st));
  // front end (Modules.py:263-270): node rows + attribute path, X = tanh(next_w(x0))
  float* recon_out = losses ? losses + 1 : nullptr;
  if (s.mode == 0) {
    if (recon_out) MATCHA_TRY(zero_async(recon_out, 2 * sizeof(float), st));
  } else {
    MATCHA_TRY(adj_forward(s, p, *frozen, *opts, ids, Tn, w.node, recon_out, w.adj_ws, w.adj_ws_bytes, st, cnt, w.rg.tok_slot));
  }
  float* x0 = w.a;
  MATCHA_TRY(launch_embed_fwd(ids, Tn, d, s.mode == 0 ? p.table : nullptr, s.mode == 0 ? nullptr : w.node, *frozen, s.n_attr, p.attr_w, p.attr_b, x0, st, cnt));
  {
    GemmArgs g = gemm_long(w.rg, x0, p.next_w, w.X, Tn, d, d);
    g.flags = MATCHA_EPI_BIAS | MATCHA_EPI_TANH; g.bias[0] = p.next_b;
    MATCHA_TRY(launch_gemm_rm(false, g, st));
  }
  // three LayerNorms on the same row (Modules.py:519-521), the heads' projections (:527-529), the attention
  float *qin = w.a, *kin = w.b, *vin = w.c;
  MATCHA_TRY(launch_ln3_fwd(w.X, Tn, d, p.ln_q_g, p.ln_q_b, p.ln_k_g, p.ln_k_b, p.ln_v_g, p.ln_v_b, qin, kin, vin, w.stats, st, cnt));
  if (merged) {
    const BmmProduct pr[2] = {
        {p.w_k, 1, d, (int64_t)d * d, p.w_q, d, 1, (int64_t)d * d, w.lwB, d, (int64_t)d * d, 0},      // B_h[a][b] = sum_m W_k[h d + m][a] W_q[h d + m][b]
        {p.fc1_w, hd, 1, d, p.w_v, d, 1, (int64_t)d * d, w.lwM, hd, d, 0}};                           // M_all[n][h d + b] = sum_m Wfc1[n][h d + m] W_v[h d + m][b]
    MATCHA_TRY(launch_bmm_heads(pr, 2, d, st));
    GemmArgs g = gemm_long(w.rg, qin, w.lwB, w.Q, Tn, hd, d);                                            // r = qin B_all^T
    MATCHA_TRY(launch_gemm_rm(false, g, st));
    MATCHA_TRY(launch_attn_long(w.Q, kin, vin, w.rg.row_off, B, L, d, d, 0, w.Q, st));                // Z = P . vin per head, over r
  } else {
    GemmArgs g = gemm_long(w.rg, qin, p.w_q, w.Q, Tn, hd, d);
    g.A[1] = kin; g.B[1] = p.w_k; g.C[1] = w.K;
    g.A[2] = vin; g.B[2] = p.w_v; g.C[2] = w.V;
    g.batch = 3;
    MATCHA_TRY(launch_gemm_rm(false, g, st));
    MATCHA_TRY(launch_attn_long(w.Q, w.K, w.V, w.rg.row_off, B, L, d, hd, d, w.Q, st));               // O over Q
  }
  // Y = fc1(O) * non_pad_mask (Modules.py:572, :614); the mask only zeroes the shared padding token's row -- whose O row the attention never
  // writes: it still holds the projection's (finite) row, and the row mask selects zero there
  float *Y = w.a, *H1 = w.b, *H2 = w.c;
  {
    GemmArgs g = gemm_long(w.rg, w.Q, merged ? w.lwM : p.fc1_w, Y, Tn, d, hd);
    g.flags = MATCHA_EPI_BIAS | MATCHA_EPI_ROWMASK; g.bias[0] = p.fc1_b; g.row_ids = ids;
    MATCHA_TRY(launch_gemm_rm(false, g, st));
  }
  // pff_n1: H1 = tanh(conv0(Y));  H2 = conv1(H1) + Y      (Modules.py:353-371)
  {
    GemmArgs g = gemm_long(w.rg, Y, p.pff0_w, H1, Tn, d, d);
    g.flags = MATCHA_EPI_BIAS | MATCHA_EPI_TANH; g.bias[0] = p.pff0_b;
    MATCHA_TRY(launch_gemm_rm(false, g, st));
  }
  {
    GemmArgs g = gemm_long(w.rg, H1, p.pff1_w, H2, Tn, d, d);
    g.flags = MATCHA_EPI_BIAS | MATCHA_EPI_RESIDUAL; g.bias[0] = p.pff1_b; g.residual = Y;
    MATCHA_TRY(launch_gemm_rm(false, g, st));
  }
  // LayerNorms, (dynamic - static)^2, Conv1d(d -> 1), masked mean over the row's k real tokens / (k + 1e-15)   (Modules.py:373-374, :290-311)
  HeadParams hp = {p.pff_ln_g, p.pff_ln_b, p.ln1_g, p.ln1_b, p.ln2_g, p.ln2_b, p.cls_w, p.cls_b};
  return launch_head_fwd(w.rg.row_off, H2, w.X, B, L, d, hp, nullptr, nullptr, logits, nullptr, nullptr, st);
}

extern "C" size_t matcha_workspace_bytes_long_train(const matcha_shape* shp, int64_t B, int32_t L) {
  if (check_shape_long(shp, B, L, "matcha_workspace_bytes_long_train") != MATCHA_OK) return 0;
  LongTrainWs w;
  return carve_long_train(*shp, B, L, nullptr, w, long_merged(*shp));
}

extern "C" int matcha_forward_long_train(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen, const matcha_step_opts* opts,
                                         const int64_t* x, int64_t B, int32_t L, float* logits, float* losses, void* ws, size_t ws_bytes,
                                         matcha_stream_t stream) {
  MATCHA_TRY(check_shape_long(shp, B, L, "matcha_forward_long_train"));
  MATCHA_CHECK_ARG(params && frozen && opts && x && ws && logits, "matcha_forward_long_train: null pointer");
  MATCHA_CHECK_ARG(!opts->deterministic && !opts->sparse_table_grad && !opts->loss_in_forward && !opts->random_chrom_dev,
                   "matcha_forward_long_train: opts->deterministic, sparse_table_grad, loss_in_forward and random_chrom_dev belong to the L <= %d step "
                   "(got %d, %d, %d, %s)", MATCHA_MAX_L, (int)opts->deterministic, (int)opts->sparse_table_grad, (int)opts->loss_in_forward,
                   opts->random_chrom_dev ? "set" : "null");
  MATCHA_CHECK_ARG(((uintptr_t)ws) % 256 == 0, "matcha_forward_long_train: workspace must be 256-byte aligned");
  const matcha_shape& s = *shp;
  const matcha_tensors& p = *params;
  const bool train = opts->training != 0;
  MATCHA_CHECK_ARG(!train || opts->seed || (opts->p_drop_adj <= 0 && opts->p_drop_fc1 <= 0 && opts->p_drop_pff <= 0),
                   "matcha_forward_long_train: training with dropout needs opts->seed");
  MATCHA_CHECK_ARG((frozen->attr_table || frozen->attr_mode == 1) && p.attr_w && p.attr_b && p.next_w && p.next_b && p.w_q && p.w_k && p.w_v && p.fc1_w &&
                       p.fc1_b && p.pff0_w && p.pff0_b && p.pff1_w && p.pff1_b && p.pff_ln_g && p.pff_ln_b && p.ln1_g && p.ln1_b &&
                       p.ln2_g && p.ln2_b && p.cls_w && p.cls_b && p.ln_q_g && p.ln_q_b && p.ln_k_g && p.ln_k_b && p.ln_v_g && p.ln_v_b,
                   "matcha_forward_long_train: a parameter pointer is null");
  MATCHA_CHECK_ARG(s.mode == 1 || p.table, "matcha_forward_long_train: table mode without table");
  const bool merged = long_merged(s);
  LongTrainWs w;
  const size_t need = carve_long_train(s, B, L, (char*)ws, w, merged);
  if (ws_bytes < need) { set_error("matcha_forward_long_train: workspace %zu < %zu bytes", ws_bytes, need); return MATCHA_ENOMEM; }
  hipStream_t st = (hipStream_t)stream;
  const int64_t Tn = B * L + 1;                 // upper bound; the true count is *w.rg.count
  const int d = s.d;
  const int64_t hd = (int64_t)MATCHA_N_HEAD * d;
  const int32_t* cnt = w.rg.count;
  const int64_t* ids = w.rg.tok_id;

  MATCHA_TRY(launch_long_plan(x, B, L, s.n_nodes, opts->status, w.rg, w.mask, st));
  float* recon_out = losses ? losses + 1 : nullptr;
  if (s.mode == 0) {
    if (recon_out) MATCHA_TRY(zero_async(recon_out, 2 * sizeof(float), st));
  } else {
    MATCHA_TRY(adj_forward(s, p, *frozen, *opts, ids, Tn, w.node, recon_out, w.adj_ws, w.adj_ws_bytes, st, cnt, w.rg.tok_slot));
  }
  MATCHA_TRY(launch_embed_fwd(ids, Tn, d, s.mode == 0 ? p.table : nullptr, s.mode == 0 ? nullptr : w.node, *frozen, s.n_attr, p.attr_w, p.attr_b, w.x0, st, cnt));
  {
    GemmArgs g = gemm_long(w.rg, w.x0, p.next_w, w.X, Tn, d, d);
    g.flags = MATCHA_EPI_BIAS | MATCHA_EPI_TANH; g.bias[0] = p.next_b;
    MATCHA_TRY(launch_gemm_rm(false, g, st));
  }
  long_note_forward(ws, merged);                // the backward on this workspace follows the same head formulation
  MATCHA_TRY(launch_ln3_fwd(w.X, Tn, d, p.ln_q_g, p.ln_q_b, p.ln_k_g, p.ln_k_b, p.ln_v_g, p.ln_v_b, w.qin, w.kin, w.vin, w.stats, st, cnt));
  if (merged) {
    const BmmProduct pr[2] = {
        {p.w_k, 1, d, (int64_t)d * d, p.w_q, d, 1, (int64_t)d * d, w.lwB, d, (int64_t)d * d, 0},      // B_h[a][b] = sum_m W_k[h d + m][a] W_q[h d + m][b]
        {p.fc1_w, hd, 1, d, p.w_v, d, 1, (int64_t)d * d, w.lwM, hd, d, 0}};                           // M_all[n][h d + b] = sum_m Wfc1[n][h d + m] W_v[h d + m][b]
    MATCHA_TRY(launch_bmm_heads(pr, 2, d, st));
    GemmArgs g = gemm_long(w.rg, w.qin, w.lwB, w.Q, Tn, hd, d);                                       // r = qin B_all^T
    MATCHA_TRY(launch_gemm_rm(false, g, st));
    MATCHA_TRY(launch_attn_long(w.Q, w.kin, w.vin, w.rg.row_off, B, L, d, d, 0, w.O, st));            // Z = P . vin per head, r is kept
  } else {
    GemmArgs g = gemm_long(w.rg, w.qin, p.w_q, w.Q, Tn, hd, d);
    g.A[1] = w.kin; g.B[1] = p.w_k; g.C[1] = w.K;
    g.A[2] = w.vin; g.B[2] = p.w_v; g.C[2] = w.V;
    g.batch = 3;
    MATCHA_TRY(launch_gemm_rm(false, g, st));
    MATCHA_TRY(launch_attn_long(w.Q, w.K, w.V, w.rg.row_off, B, L, d, hd, d, w.O, st));
  }
  // the attention writes the real tokens' O rows only: the padding token's row feeds fc1 under a row mask and dM / dWfc1 as a factor of a zero
  // gradient row -- it must be finite, so it is zeroed here (the forward-only chain reads the projection's row there)
  MATCHA_TRY(launch_long_zero_row(w.O, w.rg.row_off + B, hd, st));
  // Y = dropout(fc1(O)) * non_pad_mask (Modules.py:572, :614)
  {
    GemmArgs g = gemm_long(w.rg, w.O, merged ? w.lwM : p.fc1_w, w.Y, Tn, d, hd);
    g.flags = MATCHA_EPI_BIAS | MATCHA_EPI_ROWMASK; g.bias[0] = p.fc1_b; g.row_ids = ids;
    if (train && opts->p_drop_fc1 > 0.f) { g.flags |= MATCHA_EPI_DROPOUT; g.seed = opts->seed; g.stream_id = kStreamDropFc1; g.p_drop = opts->p_drop_fc1; }
    MATCHA_TRY(launch_gemm_rm(false, g, st));
  }
  // pff_n1: H1 = dropout(tanh(conv0(Y)));  H2 = conv1(H1) + Y      (Modules.py:353-371)
  {
    GemmArgs g = gemm_long(w.rg, w.Y, p.pff0_w, w.H1, Tn, d, d);
    g.flags = MATCHA_EPI_BIAS | MATCHA_EPI_TANH; g.bias[0] = p.pff0_b;
    if (train && opts->p_drop_pff > 0.f) { g.flags |= MATCHA_EPI_DROPOUT; g.seed = opts->seed; g.stream_id = kStreamDropPff; g.p_drop = opts->p_drop_pff; }
    MATCHA_TRY(launch_gemm_rm(false, g, st));
  }
  {
    GemmArgs g = gemm_long(w.rg, w.H1, p.pff1_w, w.H2, Tn, d, d);
    g.flags = MATCHA_EPI_BIAS | MATCHA_EPI_RESIDUAL; g.bias[0] = p.pff1_b; g.residual = w.Y;
    MATCHA_TRY(launch_gemm_rm(false, g, st));
  }
  HeadParams hp = {p.pff_ln_g, p.pff_ln_b, p.ln1_g, p.ln1_b, p.ln2_g, p.ln2_b, p.cls_w, p.cls_b};
  MATCHA_TRY(launch_head_fwd(w.rg.row_off, w.H2, w.X, B, L, d, hp, nullptr, nullptr, w.logits, nullptr, nullptr, st));
  if (hipMemcpyAsync(logits, w.logits, B * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
    set_error("matcha_forward_long_train: logits copy failed"); return MATCHA_EHIP;
  }
  return MATCHA_OK;
}
