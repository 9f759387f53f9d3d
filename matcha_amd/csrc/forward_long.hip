// Rows of up to MATCHA_MAX_LONG_L = 32 columns (include/matcha_hip.h): matcha_forward_long, the inference forward, matcha_get_embedding_long,
// the same chain stopped in front of the classifier head with the attention probabilities written out, and the training pair
// matcha_forward_long_train / matcha_backward_long.
//
// The token-level layers do not care about L: all four entry points run the layer-by-layer chain of layerwise.hip -- the one matcha_forward /
// matcha_backward run at embed_dim != 64 -- on the Tr real tokens + ONE shared padding token of the plan.  What is bound to L <= 8 there has
// its long counterpart: the plan (ragged_long.hip) and the attention (attention_long.hip, attention_long_bwd.hip; ChainOpts::long_attn).
// embed_dim a multiple of 64 runs the merged heads (r = qin B_all^T, every head attends the shared rows kin / vin, dyn = Z M_all^T), every
// other the reference's four products.  So this file holds what is the long rows' own: the argument checks, the two workspace layouts,
// the plan's launch and the forward record's use.
//
// Inference layout (carve_long).  Per token: the plan (20 B, and 8 B per row), X, three [d] rows that are reused along the chain -- x0 / qin / Y,
// kin / H1, vin / H2 -- the LayerNorm statistics and the heads' rows: r alone with merged heads, Q, K, V without; the attention writes O over Q
// in place.  That is 12 d floats per token merged (3 KB at embed_dim 64), 28 d otherwise (1.75 KB at embed_dim 16), + d in adj mode, against
// ~80 d of the L <= 8 training layout.
//
// Training layout (carve_long_train).  Every activation the backward reads is kept in a buffer of its own (O is NOT written over Q), the
// gradients of the 8 d-wide tensors too, except dO, which takes O's place once the fc1 weight gradient has read it.  Per token, in floats:
// x0, X, qin, kin, vin, Y, H1, H2, dH2, dXs, dZ1, ddyn0, dZ0, dX0, dqin, dkin, dvin (17 d), the LayerNorm statistics (2), r / Z / dR with merged
// heads (24 d: 41 d in all), Q, K, V, O, dQ, dK, dV without (56 d: 73 d in all), + d on the adj front end; + the plan's 20 B (8 B per row).
#include "layerwise.hpp"

namespace matcha {

namespace {

typedef TokenChain LongWs;      // (the plan's scratch `mask` is a field of the chain: the attention's probability instance reads it)

// one bump allocator for both layouts: 256-byte granules, null for a buffer the layout does not have (and while the layout is only being sized)
struct Bump {
  char* base; size_t off;
  float* operator()(size_t n_floats) {
    float* p = (base && n_floats) ? (float*)(base + off) : nullptr;
    off += align_up(n_floats * sizeof(float), 256);
    return p;
  }
};

size_t carve_long(const matcha_shape& s, int64_t B, int L, char* base, LongWs& w, bool merged) {
  const int64_t Tn = B * L + 1, d = s.d, hd = (int64_t)MATCHA_N_HEAD * d;
  w = LongWs();
  if (base) long_plan_carve(B, L, base, w.rg, &w.mask);
  Bump take{base, align_up(long_plan_bytes(B, L), 256)};
  w.X = take(Tn * d);
  w.x0 = w.qin = w.Y = take(Tn * d);      // x0, then qin, then Y
  w.kin = w.H1 = take(Tn * d);
  w.vin = w.H2 = take(Tn * d);
  w.stats = take(Tn * 2);
  w.Q = w.O = take(Tn * hd);              // merged heads: Q holds r and K / V do not exist;  the attention writes O over Q
  w.K = take(merged ? 0 : Tn * hd); w.V = take(merged ? 0 : Tn * hd);
  w.lwB = take(merged ? (size_t)hd * d : 0); w.lwM = take(merged ? (size_t)hd * d : 0);
  w.node = take(s.mode == 1 ? Tn * d : 0);
  w.adj_ws_bytes = s.mode == 1 ? adj_workspace_bytes(s, Tn) : 0;
  w.adj_ws = take(w.adj_ws_bytes / sizeof(float));
  return take.off;      // (no logits buffer: the head writes the caller's;  no backward buffers)
}

size_t carve_long_train(const matcha_shape& s, int64_t B, int L, char* base, LongWs& w, bool merged) {
  const int64_t Tn = B * L + 1, d = s.d, hd = (int64_t)MATCHA_N_HEAD * d;
  w = LongWs();
  if (base) long_plan_carve(B, L, base, w.rg, &w.mask);
  Bump take{base, align_up(long_plan_bytes(B, L), 256)};
  w.x0 = take(Tn * d); w.X = take(Tn * d); w.qin = take(Tn * d); w.kin = take(Tn * d); w.vin = take(Tn * d);
  w.stats = take(Tn * 2);
  w.Q = take(Tn * hd); w.K = take(merged ? 0 : Tn * hd); w.V = take(merged ? 0 : Tn * hd); w.O = take(Tn * hd);      // merged: Q = r, O = Z, no K / V
  w.Y = take(Tn * d); w.H1 = take(Tn * d); w.H2 = take(Tn * d);
  w.logits = take(B);
  w.node = take(s.mode == 1 ? Tn * d : 0);
  w.dH2 = take(Tn * d); w.dXs = take(Tn * d); w.dZ1 = take(Tn * d); w.ddyn0 = take(Tn * d); w.dZ0 = take(Tn * d); w.dX0 = take(Tn * d);
  w.dO = w.O;                                   // dO takes O's place once the fc1 weight gradient has read it
  w.dQ = take(Tn * hd); w.dK = take(merged ? 0 : Tn * hd); w.dV = take(merged ? 0 : Tn * hd);                          // merged: dQ = dR, no dK / dV
  w.dqin = take(Tn * d); w.dkin = take(Tn * d); w.dvin = take(Tn * d);
  chain_scratch_bytes(s, B, L, true, w);
  w.slab = take(w.slab_bytes / sizeof(float));
  w.gemm_ws = take(w.gemm_ws_bytes / sizeof(float));
  w.adj_ws_bytes = s.mode == 1 ? adj_workspace_bytes(s, Tn) : 0;
  w.adj_ws = take(w.adj_ws_bytes / sizeof(float));
  const size_t nm = merged ? (size_t)hd * d : 0;
  w.lwB = take(nm); w.lwM = take(nm); w.lwdB = take(nm); w.lwdM = take(nm);
  return take.off;
}

// merged heads where embed_dim is a multiple of 64, unless the option table says otherwise
bool long_merged(const matcha_shape& s) { return bmm_heads_supported(s.d) && !options().disable_merged; }

int check_shape_long(const matcha_shape* s, int64_t B, int32_t L, const char* fn) {
  MATCHA_TRY(check_shape_fields(s, fn));
  MATCHA_CHECK_ARG(L >= 2 && L <= MATCHA_MAX_LONG_L, "%s: L=%d outside 2..%d", fn, L, MATCHA_MAX_LONG_L);
  MATCHA_CHECK_ARG(B >= 1 && B * (int64_t)L < (1ll << 31) - 2, "%s: B=%lld must be >= 1 and B*L < 2^31 - 2", fn, (long long)B);
  // the layer-by-layer kernels put token tiles on grid.y (<= 65 535 tiles of 128 tokens): 8.38 M token rows is what they launch
  MATCHA_CHECK_ARG(B * (int64_t)L + 1 <= 65535ll * 128, "%s: B*L=%lld exceeds the %lld token rows the layer-by-layer kernels launch", fn,
                   (long long)(B * (int64_t)L), 65535ll * 128);
  return MATCHA_OK;
}

// what both forwards ask of their (non-null) arguments behind the shape and their own option rules
int check_forward_long(const matcha_shape& s, const matcha_tensors& p, const matcha_frozen& f, const matcha_step_opts& o, const void* ws, const char* fn) {
  MATCHA_CHECK_ARG(((uintptr_t)ws) % 256 == 0, "%s: workspace must be 256-byte aligned", fn);
  MATCHA_CHECK_ARG(!o.training || o.seed || (o.p_drop_adj <= 0 && o.p_drop_fc1 <= 0 && o.p_drop_pff <= 0), "%s: training with dropout needs opts->seed", fn);
  MATCHA_TRY(check_chain_params(p, f, fn));
  MATCHA_CHECK_ARG(s.mode == 1 || p.table, "%s: table mode without table", fn);
  return MATCHA_OK;
}

}  // namespace

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
  static const char fn[] = "matcha_forward_long";
  MATCHA_TRY(check_shape_long(shp, B, L, fn));
  MATCHA_CHECK_ARG(params && frozen && opts && x && ws && logits, "%s: null pointer", fn);
  MATCHA_CHECK_ARG(opts->training == 0 && opts->forward_only == 1,
                   "matcha_forward_long: long rows are inference-only (opts->training must be 0 and opts->forward_only 1; got %d, %d)",
                   (int)opts->training, (int)opts->forward_only);
  MATCHA_CHECK_ARG(!opts->random_chrom_dev, "matcha_forward_long: opts->random_chrom_dev needs the fused adj front end; pass opts->random_chrom");
  const matcha_shape& s = *shp;
  MATCHA_TRY(check_forward_long(s, *params, *frozen, *opts, ws, fn));
  const bool merged = long_merged(s);
  LongWs w;
  const size_t need = carve_long(s, B, L, (char*)ws, w, merged);
  if (ws_bytes < need) { set_error("matcha_forward_long: workspace %zu < %zu bytes", ws_bytes, need); return MATCHA_ENOMEM; }
  hipStream_t st = (hipStream_t)stream;
  const ChainCall chain{s, *params, *frozen, *opts, B, L, st, {merged, true, false}, fn};

  forget_forward(ws);      // (a training forward's record on this pointer, of either kind, is void: its activations are being overwritten)
  MATCHA_TRY(launch_long_plan(x, B, L, s.n_nodes, opts->status, w.rg, w.mask, st));
  MATCHA_TRY(chain_front_fwd(chain, w, losses ? losses + 1 : nullptr, true));
  // (keep off: the padding token's O row, which the attention never writes, still holds the projection's finite row under fc1's row mask)
  MATCHA_TRY(chain_attn_fwd(chain, w));
  return chain_tail_fwd(chain, w, nullptr, nullptr, logits, nullptr, MATCHA_OBJECTIVE_BCE, false);
}

// Classifier.get_embedding at up to 32 columns: the inference chain up to pff_n1's convolutions (X and H2 live in the inference layout), the
// attention's probability instance writing the caller's padded `attn` completely (null: the plain kernel), then expand_embedding_kernel.
extern "C" int matcha_get_embedding_long(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen, const matcha_step_opts* opts,
                                         const int64_t* x, int64_t B, int32_t L, float* dynamic, float* static_, float* attn, float* losses, void* ws,
                                         size_t ws_bytes, matcha_stream_t stream) {
  static const char fn[] = "matcha_get_embedding_long";
  MATCHA_TRY(check_shape_long(shp, B, L, fn));
  MATCHA_CHECK_ARG(params && frozen && opts && x && ws && dynamic && static_, "%s: null pointer (only attn and losses are optional)", fn);
  MATCHA_CHECK_ARG(opts->training == 0 && opts->forward_only == 1,
                   "matcha_get_embedding_long: inference-only (opts->training must be 0 and opts->forward_only 1; got %d, %d)",
                   (int)opts->training, (int)opts->forward_only);
  MATCHA_CHECK_ARG(!opts->random_chrom_dev, "matcha_get_embedding_long: opts->random_chrom_dev needs the fused adj front end; pass opts->random_chrom");
  const matcha_shape& s = *shp;
  MATCHA_TRY(check_forward_long(s, *params, *frozen, *opts, ws, fn));
  const bool merged = long_merged(s);
  LongWs w;
  const size_t need = carve_long(s, B, L, (char*)ws, w, merged);
  MATCHA_CHECK_ARG(ws_bytes >= need, "matcha_get_embedding_long: workspace %zu < %zu bytes", ws_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const ChainCall chain{s, *params, *frozen, *opts, B, L, st, {merged, true, false}, fn};
  w.P = attn;              // the caller's [8 B, L, L]: chain_attn_fwd launches attn_long_prob_kernel when it is there

  forget_forward(ws);
  MATCHA_TRY(launch_long_plan(x, B, L, s.n_nodes, opts->status, w.rg, w.mask, st));
  MATCHA_TRY(chain_front_fwd(chain, w, losses ? losses + 1 : nullptr, true));
  MATCHA_TRY(chain_attn_fwd(chain, w));
  MATCHA_TRY(chain_tail_fwd(chain, w, nullptr, nullptr, nullptr, nullptr, MATCHA_OBJECTIVE_BCE, true));
  return launch_expand_embedding(x, B, L, s.d, w.rg.row_off, w.H2, w.X, params->pff_ln_g, params->pff_ln_b, dynamic, static_, st);
}

// Per-locus scores: matcha_forward_long's chain up to pff_n1's convolutions (same checks, same workspace), then the head that keeps the
// per-token value (locus.hip: head_scores_kernel writes scores, logits and order completely).
extern "C" int matcha_locus_scores(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen, const matcha_step_opts* opts,
                                   const int64_t* x, int64_t B, int32_t L, float* scores, float* logits, int32_t lowest, int64_t* order,
                                   float* losses, void* ws, size_t ws_bytes, matcha_stream_t stream) {
  static const char fn[] = "matcha_locus_scores";
  MATCHA_TRY(check_shape_long(shp, B, L, fn));
  MATCHA_CHECK_ARG(params && frozen && opts && x && ws && scores, "%s: null pointer (only logits, order and losses are optional)", fn);
  MATCHA_CHECK_ARG(lowest >= 0 && lowest <= MATCHA_MAX_LONG_L, "%s: lowest=%d outside 0..%d", fn, lowest, MATCHA_MAX_LONG_L);
  MATCHA_CHECK_ARG((lowest == 0) == (order == nullptr), "%s: order must be null when lowest == 0 and only then (lowest=%d)", fn, lowest);
  MATCHA_CHECK_ARG(opts->training == 0 && opts->forward_only == 1,
                   "matcha_locus_scores: inference-only (opts->training must be 0 and opts->forward_only 1; got %d, %d)",
                   (int)opts->training, (int)opts->forward_only);
  MATCHA_CHECK_ARG(!opts->random_chrom_dev, "matcha_locus_scores: opts->random_chrom_dev needs the fused adj front end; pass opts->random_chrom");
  const matcha_shape& s = *shp;
  MATCHA_TRY(check_forward_long(s, *params, *frozen, *opts, ws, fn));
  const bool merged = long_merged(s);
  LongWs w;
  const size_t need = carve_long(s, B, L, (char*)ws, w, merged);
  if (ws_bytes < need) { set_error("matcha_locus_scores: workspace %zu < %zu bytes", ws_bytes, need); return MATCHA_ENOMEM; }
  hipStream_t st = (hipStream_t)stream;
  const ChainCall chain{s, *params, *frozen, *opts, B, L, st, {merged, true, false}, fn};

  forget_forward(ws);
  MATCHA_TRY(launch_long_plan(x, B, L, s.n_nodes, opts->status, w.rg, w.mask, st));
  MATCHA_TRY(chain_front_fwd(chain, w, losses ? losses + 1 : nullptr, true));
  MATCHA_TRY(chain_attn_fwd(chain, w));
  MATCHA_TRY(chain_tail_fwd(chain, w, nullptr, nullptr, nullptr, nullptr, MATCHA_OBJECTIVE_BCE, true));
  const matcha_tensors& p = *params;
  const HeadParams hp = {p.pff_ln_g, p.pff_ln_b, p.ln1_g, p.ln1_b, p.ln2_g, p.ln2_b, p.cls_w, p.cls_b};
  return launch_head_scores(w.rg.row_off, w.rg.tok_slot, w.H2, w.X, B, L, s.d, hp, scores, logits, lowest, order, st);
}

extern "C" size_t matcha_workspace_bytes_long_train(const matcha_shape* shp, int64_t B, int32_t L) {
  if (check_shape_long(shp, B, L, "matcha_workspace_bytes_long_train") != MATCHA_OK) return 0;
  LongWs w;
  return carve_long_train(*shp, B, L, nullptr, w, long_merged(*shp));
}

extern "C" int matcha_forward_long_train(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen, const matcha_step_opts* opts,
                                         const int64_t* x, int64_t B, int32_t L, float* logits, float* losses, void* ws, size_t ws_bytes,
                                         matcha_stream_t stream) {
  static const char fn[] = "matcha_forward_long_train";
  MATCHA_TRY(check_shape_long(shp, B, L, fn));
  MATCHA_CHECK_ARG(params && frozen && opts && x && ws && logits, "%s: null pointer", fn);
  MATCHA_CHECK_ARG(!opts->deterministic && !opts->sparse_table_grad && !opts->loss_in_forward && !opts->random_chrom_dev,
                   "matcha_forward_long_train: opts->deterministic, sparse_table_grad, loss_in_forward and random_chrom_dev belong to the L <= %d step "
                   "(got %d, %d, %d, %s)", MATCHA_MAX_L, (int)opts->deterministic, (int)opts->sparse_table_grad, (int)opts->loss_in_forward,
                   opts->random_chrom_dev ? "set" : "null");
  const matcha_shape& s = *shp;
  MATCHA_TRY(check_forward_long(s, *params, *frozen, *opts, ws, fn));
  const bool merged = long_merged(s);
  LongWs w;
  const size_t need = carve_long_train(s, B, L, (char*)ws, w, merged);
  if (ws_bytes < need) { set_error("matcha_forward_long_train: workspace %zu < %zu bytes", ws_bytes, need); return MATCHA_ENOMEM; }
  hipStream_t st = (hipStream_t)stream;
  const ChainCall chain{s, *params, *frozen, *opts, B, L, st, {merged, true, true}, fn};

  MATCHA_TRY(launch_long_plan(x, B, L, s.n_nodes, opts->status, w.rg, w.mask, st));
  MATCHA_TRY(chain_front_fwd(chain, w, losses ? losses + 1 : nullptr, true));
  StepRoute route = {};
  route.long_rows = true; route.merged_layerwise = merged;      // the backward on this workspace follows the same head formulation
  note_forward(ws, route);
  MATCHA_TRY(chain_attn_fwd(chain, w));
  return chain_tail_fwd(chain, w, nullptr, nullptr, logits, nullptr, MATCHA_OBJECTIVE_BCE, false);
}

extern "C" int matcha_backward_long(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen, const matcha_step_opts* opts,
                                    const int64_t* x, int64_t B, int32_t L, const float* dlogits, const float* drecon, matcha_tensors* grads,
                                    int32_t* touched, void* ws, size_t ws_bytes, matcha_stream_t stream) {
  static const char fn[] = "matcha_backward_long";
  MATCHA_TRY(check_shape_long(shp, B, L, fn));
  MATCHA_CHECK_ARG(params && frozen && opts && x && ws && grads && dlogits, "matcha_backward_long: null pointer (dlogits is required)");
  MATCHA_CHECK_ARG(!opts->deterministic && !opts->sparse_table_grad && !opts->loss_in_forward && !opts->random_chrom_dev,
                   "matcha_backward_long: opts->deterministic, sparse_table_grad, loss_in_forward and random_chrom_dev belong to the L <= %d step", MATCHA_MAX_L);
  MATCHA_CHECK_ARG(frozen->attr_table, "matcha_backward_long: the attribute_nn backward gathers attr_table rows (also under attr_mode 1)");
  const matcha_shape& s = *shp;
  MATCHA_CHECK_ARG(s.mode == 1 || grads->table, "matcha_backward_long: table mode without a table gradient buffer");
  LongWs w;
  // the size is checked against both formulations' layouts before the record is consumed: a refusal leaves the forward's record in place
  const size_t least = carve_long_train(s, B, L, nullptr, w, true);
  if (ws_bytes < least) { set_error("matcha_backward_long: workspace %zu < %zu bytes", ws_bytes, least); return MATCHA_ENOMEM; }
  // (a record of matcha_forward is none of this entry point's: refused like no record, and left for matcha_backward)
  StepRoute route;
  MATCHA_CHECK_ARG(recorded_route(ws, route) && route.long_rows,
                   "matcha_backward_long: no matcha_forward_long_train on record for this workspace (one backward per forward, same ws pointer)");
  const size_t need = carve_long_train(s, B, L, (char*)ws, w, route.merged_layerwise);
  if (ws_bytes < need) { set_error("matcha_backward_long: workspace %zu < %zu bytes", ws_bytes, need); return MATCHA_ENOMEM; }
  forget_forward(ws);      // one backward per forward: from here on the saved activations are being overwritten
  const ChainCall chain{s, *params, *frozen, *opts, B, L, (hipStream_t)stream, {route.merged_layerwise, true, true}, fn};
  MATCHA_TRY(chain_tail_bwd(chain, w, w.X, nullptr, nullptr, nullptr, dlogits, MATCHA_OBJECTIVE_BCE, *grads));
  MATCHA_TRY(chain_attn_bwd(chain, w, *grads));
  return chain_front_bwd(chain, w, drecon, *grads, touched);
}
