// Orchestration of one classifier step behind the C ABI: Classifier.forward (Modules.py:278-318) and its
// backward as a fixed sequence of kernel launches on the caller's stream -- no allocation, no host
// synchronisation, so the whole step is hipGraph-capturable.
//
// Token layout: ragged (ragged.hip).  The token-level layers run on Tn = Tr + 1 rows -- the Tr real tokens of the
// batch plus ONE shared padding token -- instead of B*L slots; Tr is only known on the device, so every launch is
// sized for the upper bound B*L + 1 and reads the true count from `count` (m_dev / r_dev / t_dev).
//
// This file holds the step's workspace layout (carve), its kernel route (decide_route) and the fused routes' launches.  Where a route runs
// layer by layer -- every embed_dim but 64, embed_dim 64 under a switch, matcha_get_embedding, the pieces around enc128 and around the fused
// encoder -- forward_impl / backward_impl call the chain's pieces of layerwise.hip, which the long rows' entry points (forward_long.hip) call too.
#include <stdlib.h>
#include <string.h>

#include <unordered_map>

#include "layerwise.hpp"
#include "tail_reduce.hpp"
#include "fb_unfold.hpp"
#include "ragged_roles.hpp"

namespace matcha {

thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int device_cu_count() {
  static int cache[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 256; }
  if (dev >= 0 && dev < 64 && cache[dev] > 0) return cache[dev];
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); return 256; }
  if (dev >= 0 && dev < 64) cache[dev] = n;
  return n;
}

// ---- per-kernel-class event timing -------------------------------------------------------------------
int g_prof_class = 0;
static hipEvent_t* g_prof_ev = nullptr;     // pairs (start, stop)
static int g_prof_cap = 0, g_prof_used = 0;
static double g_prof_work = 0.0;
void prof_record(bool start, double work, hipStream_t st) {
  if (start) {
    if (g_prof_used + 2 > g_prof_cap) {
      const int ncap = g_prof_cap ? 2 * g_prof_cap : 1024;
      hipEvent_t* ne = (hipEvent_t*)realloc(g_prof_ev, sizeof(hipEvent_t) * ncap);
      if (!ne) return;
      g_prof_ev = ne;
      for (int i = g_prof_cap; i < ncap; ++i)
        if (hipEventCreate(&g_prof_ev[i]) != hipSuccess) { g_prof_cap = i & ~1; return; }
      g_prof_cap = ncap;
    }
    g_prof_work += work;
    (void)hipEventRecord(g_prof_ev[g_prof_used], st);
  } else if (g_prof_used + 1 < g_prof_cap) {
    (void)hipEventRecord(g_prof_ev[g_prof_used + 1], st);
    g_prof_used += 2;
  }
}

// ---- launch log: kernel name -> number of launches since matcha_launch_log(1) -------------------------
int g_launch_log = 0;
namespace {
struct LaunchCount { const char* name; int64_t n; };
constexpr int kLaunchNames = 128;
LaunchCount g_launches[kLaunchNames];
int g_launch_names = 0;
}  // namespace
void note_launch(const char* name) {
  for (int i = 0; i < g_launch_names; ++i)
    if (g_launches[i].name == name || strcmp(g_launches[i].name, name) == 0) { ++g_launches[i].n; return; }
  if (g_launch_names < kLaunchNames) g_launches[g_launch_names++] = LaunchCount{name, 1};
}

bool adj_fused_eligible(const matcha_shape& s, const matcha_frozen& f);     // adj_fused.hip

// The L <= 8 step's workspace: the chain's buffers (layerwise.hpp) + what only the fused routes use.
struct Workspace : TokenChain {
  float* folded;                          // LayerNorm-folded projection weights of the fused d = 64 kernels
  float* enc;                             // embed_dim 128: the fused attention block's folded weights, fragments and slabs (enc128.hip)
  float* enc_rec; size_t enc_rec_floats;  // ... and its forward records, over the Q / K / V / P / O buffers the fused path does not use
  float* merged;                          // merged per-head matrices B_h = W'k^T W'q, M_h = Wfc1_h W'v (two products per head instead of four)
  float* frag;                            // the same weights + fc1 / pff_n1 blocks in MFMA-fragment order (fused_fwd32.hip streams them from L2)
  float* fb_ws;                           // fused backward: workgroup slabs + reduction partials
  float* tslab;                           // training forward: per-tile partials of the tail / pff_n1 parameter gradients
  float* tpart;                           // their two-pass reduction's split partials
  float* tslab2;                          // large batches: one slab of weight-gradient partials per workgroup of tail_bwd64_kernel
  float* qkv;                             // training forward -> fused backward: Q, K, V tiles of every (tile, head), 384 KB per tile
  float* front_ws;                        // fused front-end backward: workgroup slabs
  // node route of the table front end (null when the shape cannot take it): X and x0 per NODE [n_nodes + 1][64] (row 0: the padding id), the
  // backward's per-node sum of the tokens' gradient rows, the id list 0..n_nodes and its length {n_nodes + 1, n_nodes} (both written by the plan)
  float *XN, *x0N, *xhN, *GN; int64_t* node_ids; int32_t* node_cnt;
  float* RN;                              // ... and the heads' r rows per node [8][n_nodes + 1][64] (node_r_kernel), rebuilt by every forward on the route
  float* VN;                              // ... and their value rows y = M_h x_hat, same shape, written by the same launch of a differentiated forward (null in the compact layout)
  size_t total;
};

// A/B switches for tests and profiling (include/matcha_hip.h, matcha_set_option): ONE process-wide struct whose initial values
// come from the environment (MATCHA_DISABLE_FUSED, ...) when it is first touched; no entry point calls getenv per call.
//   disable_fused            1: layer-by-layer kernels everywhere (the d != 64 path, at embed_dim 64 too); 2: only the FRONT END (gather +
//                            attribute_nn + next_w; its backward; the fused adj kernels) as separate kernels, the encoder stays fused
//                            (the tail's backward inside the forward kernel is a per-call choice: opts->loss_in_forward)
//   disable_merged           the REFERENCE formulation of the heads (Q, K, V, fc1: four products per head forward, eight backward) instead
//                            of the merged two / four.  It lives on the layer-by-layer kernels only (attention.hip + the GEMMs), so at
//                            embed_dim 64 the switch implies disable_fused; the fused four-product kernels of rounds 1-3 (four-wave
//                            forward, eight-wave / 64-row-tile / recompute backward, their five switches) are gone since round 4
//   disable_small_batch      the kernels picked for small batches by size -- one workgroup of eight wavefronts (one per head) per half tile
//                            in the forward, the ragged plan as one launch -- replaced by the large-batch kernels
//   disable_node_front       the table front end per TOKEN at every size (node_front_shape / the rule in forward_impl decide otherwise)
//   disable_node_r           node route: r = B_h x_hat + b_h per TOKEN inside the forward kernel, the rows handed to the backward in the record (without it:
//                            once per (node, head) by node_r_kernel, both encoder kernels gather the rows by tok_key)
//   disable_node_v           node route with the r table: the backward kernel forms dZ = dDyn M_h and Z per token, as without the r table (without
//                            the switch: node_r_kernel also writes y = M_h x_hat per (node, head) in a differentiated forward and the backward's
//                            VTAB instance gathers the rows -- no dZ product, no Z; the forward's outputs are the same bits either way; only
//                            from node_v_shape's size on: below it the table does not pay and this switch changes nothing)
//   disable_node_dx          node route with the value table: the encoder's input gradients (d x_hat of the eight heads, dXs of the tail) per TOKEN, added per
//                            node by node_scatter_kernel's walk over the tokens (without the switch: both producers add into per-node rows where they
//                            are produced -- one replica per head -- and node_scatter_kernel is the per-node finisher; the forward's outputs are the
//                            same bits either way)
//   disable_launch_pairs     the fused d = 64 step with every small launch on its own, as before the pairs of DESIGN.md 4.10 (without the switch:
//                            fbm_chain_kernel's blocks un-fold their own rows -- no fb_unfold_kernel --; on the node route fb_unfold2's vectors ride in
//                            node_scatter_kernel and the plan's tile_pack / tile_compact passes in the table front end's forward / node_r_kernel;
//                            every output is the same bits either way)
//   disable_row_pack         the fused d = 64 step's plan in batch order (without the switch: rows ordered by size class so that the half tiles fill to 31
//                            tokens, ragged.hip; logits and losses are the same bits either way, token-contracted sums add in another order)
//   disable_wide_gemm        embed_dim >= 128: the 64-wide GEMM / attention kernels (gemm_lds.hip, gemm_f32.hip, attention.hip; four-product
//                            heads) instead of gemm_wide.hip / attention_wide.hip
struct OptionName { const char* name; int Options::*field; };
static const OptionName kOptionNames[] = {
    {"disable_fused", &Options::disable_fused}, {"disable_merged", &Options::disable_merged}, {"disable_small_batch", &Options::disable_small_batch},
    {"disable_wide_gemm", &Options::disable_wide_gemm}, {"disable_node_front", &Options::disable_node_front}, {"disable_node_r", &Options::disable_node_r}, {"disable_node_v", &Options::disable_node_v}, {"disable_node_dx", &Options::disable_node_dx}, {"disable_launch_pairs", &Options::disable_launch_pairs}, {"disable_row_pack", &Options::disable_row_pack}, {"debug_nan", &Options::debug_nan}, {"fused_dbg", &Options::fused_dbg}};
Options& options() {
  static Options o = [] {
    Options v;
    memset(&v, 0, sizeof(v));
    for (const OptionName& n : kOptionNames) {
      char env[64] = "MATCHA_";
      size_t k = strlen(env);
      for (const char* c = n.name; *c && k + 1 < sizeof(env); ++c) env[k++] = (char)((*c >= 'a' && *c <= 'z') ? *c - 32 : *c);
      env[k] = 0;
      const char* e = getenv(env);
      if (e) v.*(n.field) = (*e == 0) ? 1 : atoi(e);       // "MATCHA_X=" (set, empty) counts as on, like the old getenv != NULL test
      if (e && v.*(n.field) == 0 && strcmp(e, "0") != 0) v.*(n.field) = 1;
    }
    return v;
  }();
  return o;
}
// embed_dim >= 128: the layer-by-layer path with merged heads -- r = qin B_all^T (one projection instead of three), every head attends the
// SAME key / value rows kin = LN_k(x), vin = LN_v(x) ([T, d], not [T, 8d]), dyn = Z M_all^T with M_all[:, h] = Wfc1_h W_v[h]; the
// backward computes dB_all, dM_all and applies the chain rule per head (merged_chain).  Shapes the wide attention kernels take.
static bool merged_layerwise_shape(const matcha_shape& s) { return s.d >= 128 && s.d % 64 == 0; }
static bool merged_layerwise(const matcha_shape& s) { return merged_layerwise_shape(s) && attn_wide_eligible(s.d) && !options().disable_merged; }
// embed_dim 128: attention block as one fused forward / backward kernel pair (enc128.hip).  The heads' d x_hat meet through float atomics, so the
// callers that need a bitwise reproducible embedding gradient stay on the layer-by-layer kernels.
static bool enc128_enabled(const matcha_shape& s, const matcha_step_opts& o) { return enc128_shape(s.d) && merged_layerwise(s) && options().disable_fused != 1 && !o.deterministic && !o.sparse_table_grad; }
static bool fused_enabled(const matcha_shape& s) { return s.d == 64 && options().disable_fused != 1 && !options().disable_merged; }
// Node route of the table front end: everything in front of the encoder -- x0 = table[id] + attribute_nn(attr[id]), X = tanh(next_w(x0)) -- is a
// function of the node id alone (no dropout in front of the attention), so when the tokens outnumber the nodes it is computed once per NODE
// and the encoder kernels gather their rows by id; the backward adds the tokens' gradient rows per node first and runs tanh' / next_w /
// attribute_nn / the table row once per node.  The SHAPE half of the rule (it sizes the workspace, so it must not depend on a switch):
static bool node_front_shape(const matcha_shape& s, int64_t B, int L) { return s.mode == 0 && s.d == 64 && front_bwd_supported(s.d, s.n_attr) && B * L + 1 >= 4 * ((int64_t)s.n_nodes + 1); }
// ... and the value table of that route (VN: y = M_h x_hat per node for the backward, fused_bwd.hip VTAB) on top of the r table.  It costs
// node_r_kernel's V role per NODE and saves the backward kernel work per TOKEN.  Measured against the parent's library at hg38 1 Mb (3 068
// table rows), same call, three alternations: no difference that the runs' own spread lets through at 8 192, 16 384 and 32 768 rows (capacity /
// rows of the table = 13, 27, 53), -15 to -24 us of 1.2 ms at 65 536 rows (107) -- profiles/r10_node_v.md.  So the table is built from 64 on.
static bool node_v_shape(const matcha_shape& s, int64_t B, int L) { return B * L + 1 >= 64 * ((int64_t)s.n_nodes + 1); }
// ... and the per-node sums of the encoder's input gradients at their producers (StepRoute::node_dx): the per-head replicas live
// in dO (8 (n_nodes + 1) rows of the 8 (B L + 1) there) and are zeroed by tail_bwd64_kernel, 6 MB instead of 59 MB at the headline shape.  Measured
// against the parent's library like the value table (profiles/r12_node_dx.md); the rule is the value table's.
static bool node_dx_shape(const matcha_shape& s, int64_t B, int L) { return node_v_shape(s, B, L); }
// the loss can be computed: BCE needs labels and weights, the softplus MSE only its targets
static bool has_target(int objective, const float* y, const float* w) { return objective == MATCHA_OBJECTIVE_SOFTPLUS_MSE ? y != nullptr : (y && w); }
static int check_objective(int32_t objective, const char* fn) {
  if (objective == MATCHA_OBJECTIVE_BCE || objective == MATCHA_OBJECTIVE_SOFTPLUS_MSE) return MATCHA_OK;
  set_error("%s: unknown objective %d (MATCHA_OBJECTIVE_BCE or MATCHA_OBJECTIVE_SOFTPLUS_MSE)", fn, (int)objective);
  return MATCHA_EINVAL;
}
// `compact`: layout of a forward that will not be differentiated and runs the fused kernels (d = 64): only the ragged plan,
// x0, X, the adj front end's buffers, the folded weights and the per-row outputs exist; everything else has size 0.
static size_t carve(const matcha_shape& s, int64_t B, int L, char* base, Workspace& w, bool compact = false) {
  const int64_t Tn = B * L + 1, d = s.d, hd = (int64_t)MATCHA_N_HEAD * d;      // upper bound of token rows
  size_t off = 0;
  auto take_always = [&](size_t n_floats) {
    float* p = base ? (float*)(base + off) : nullptr;
    off += align_up(n_floats * sizeof(float), 256);
    return p;
  };
  auto take = [&](size_t n_floats) { return compact ? (float*)nullptr : take_always(n_floats); };
  {
    const size_t rb = ragged_bytes(B, L);
    if (base) ragged_carve(B, L, base + off, w.rg);
    off += align_up(rb, 256);
  }
  w.x0 = take_always(Tn * d); w.X = take_always(Tn * d);
  w.qin = take(Tn * d); w.kin = take(Tn * d); w.vin = take(Tn * d);
  w.stats = take(Tn * 2);
  w.Q = take(Tn * hd); w.K = take(Tn * hd); w.V = take(Tn * hd);
  w.P = take(B * MATCHA_N_HEAD * L * L);
  w.O = take(Tn * hd);
  w.Y = take(Tn * d); w.H1 = take(Tn * d); w.H2 = take(Tn * d);
  w.row_loss = take_always(B); w.logits = take_always(B);
  w.node = take_always(s.mode == 1 ? Tn * d : 0);
  w.dH2 = take(Tn * d); w.dXs = take(Tn * d); w.dZ1 = take(Tn * d); w.ddyn0 = take(Tn * d);
  // The attention block's gradients REPLACE the activations they are computed from (layer-by-layer path; the 8d-wide tensors are
  // 32 of the ~80 d floats a token cost): dO overwrites O once the fc1 weight gradient has read it; attn_bwd reads every V chunk
  // of a hyperedge before it writes its first dV chunk, and per chunk loads all K rows before it stores dQ and all Q rows before
  // it stores dK -- so dV lives in V, dQ in K's buffer and dK in Q's (attention.hip / attention_wide.hip keep that order);
  // dqin / dkin / dvin overwrite qin / kin / vin after the projection weight gradients have read them.  With embed_dim 64 the
  // fused kernels use dO as the 8 per-head d x_hat slabs and never touch Q/K/V/O, so there the alias is harmless too.
  w.dO = w.O; w.dQ = w.K; w.dK = w.Q; w.dV = w.V;
  w.dqin = w.qin; w.dkin = w.kin; w.dvin = w.vin;
  w.dZ0 = take(Tn * d); w.dX0 = take(Tn * d);
  chain_scratch_bytes(s, B, L, false, w);
  w.slab = take(w.slab_bytes / sizeof(float));
  w.gemm_ws = take(w.gemm_ws_bytes / sizeof(float));
  w.adj_ws_bytes = (s.mode == 1) ? adj_workspace_bytes(s, Tn) : 0;
  w.adj_ws = take_always(w.adj_ws_bytes / sizeof(float));
  w.folded = take_always(s.d == 64 ? fused_fold_floats() : 0);
  w.frag = take_always(s.d == 64 ? fused_frag_floats() : 0);
  w.merged = take_always(s.d == 64 ? fused_merged_floats() : 0);
  {
    const size_t nm = merged_layerwise_shape(s) ? (size_t)hd * d : 0;
    w.lwB = take_always(nm); w.lwM = take_always(nm);
    w.lwdB = take(nm); w.lwdM = take(nm);
  }
  w.enc = take_always(enc128_shape((int)d) ? enc128_ws_floats() : 0);
  w.enc_rec = w.Q;                                        // [Q, K, V, P, O] are consecutive: Tn * 32 d + B * 8 L^2 floats
  w.enc_rec_floats = (w.Q && w.O) ? (size_t)((w.O + Tn * hd) - w.Q) : 0;
  w.fb_ws = take(s.d == 64 ? fused_bwd_ws_floats(B, L) : 0);
  w.tpart = take(s.d == 64 ? fused_tail_partial_floats() : 0);
  w.tslab = take(s.d == 64 ? fused_tail_slab32_floats(B, L) : 0);   // one slab per HALF tile (>= the four-wave kernel's per-tile need)
  w.tslab2 = take(s.d == 64 ? tail_bwd_slab_floats() : 0);
  w.qkv = take(s.d == 64 ? fused_qkv_floats(B, L) : 0);        // reserved whatever the option table says: the layout must not depend on a switch read per call
  w.front_ws = take(front_bwd_supported(s.d, s.n_attr) ? front_bwd_ws_floats() : 0);
  w.tg_ws_bytes = (s.mode == 0 && !compact) ? table_grad_ws_bytes(Tn, s.n_nodes) : 0;
  w.tg_ws = take(w.tg_ws_bytes / sizeof(float));
  {
    const size_t nn = node_front_shape(s, B, L) ? (size_t)(s.n_nodes + 1) : 0;
    w.XN = take_always(nn * 64); w.x0N = take(nn * 64); w.xhN = take(nn * 64); w.GN = take(nn * 64);
    w.node_ids = reinterpret_cast<int64_t*>(take_always(nn * 2));
    w.node_cnt = reinterpret_cast<int32_t*>(take_always(nn ? 64 : 0));
    // The r table: 8 (n_nodes + 1) rows.  A workspace that can be differentiated keeps it in Q's buffer -- the fused d = 64 kernels never touch
    // Q / K / V (see above), and Tn >= 4 (n_nodes + 1) rows of 8 d floats hold it four times over -- so the route costs a training step no memory;
    // the compact layout of a forward-only call has no Q and takes the rows
    w.RN = nn ? (compact ? take_always(node_r_floats((int64_t)nn)) : w.Q) : nullptr;
    // the value table sits behind it in Q's buffer (two of the four); a forward-only layout never writes it
    w.VN = (nn && !compact && w.Q) ? w.Q + node_r_floats((int64_t)nn) : nullptr;      // (w.Q is null while the layout is only being sized)
  }
  w.total = off;
  return off;
}

// a forward with opts->forward_only set on the fused kernels needs no more than the compact layout; settled before carve(), which it sizes
static bool compact_forward(const matcha_shape& s, const matcha_step_opts& o, bool force_layerwise) { return !force_layerwise && o.forward_only && fused_enabled(s); }
// The route of one forward, from shapes, per-call options and the option table alone -- no device state, so a captured step replays it.  force_layerwise:
// the separate kernels whatever the shape (matcha_get_embedding needs H2 and X in HBM);  want_losses: the caller passed `losses`.
static StepRoute decide_route(const matcha_shape& s, const matcha_step_opts& o, int64_t B, int L, const Workspace& w, const matcha_frozen& f,
                              const float* y, const float* w_bce, int objective, bool force_layerwise, bool want_losses) {
  StepRoute r;
  r.compact = compact_forward(s, o, force_layerwise);
  r.fused = !force_layerwise && fused_enabled(s);
  r.merged_layerwise = merged_layerwise(s);
  // embed_dim 128: the attention block as one kernel (enc128.hip) -- when a training forward's records fit where the layer-wise path keeps
  // Q / K / V / P / O: the records are sized per HALF TILE (at least two, 8 x 4352 floats each), so a batch of one to three rows does not
  // fit and runs layer by layer (it used to fail with MATCHA_ENOMEM)
  r.enc128 = !force_layerwise && enc128_enabled(s, o) && (o.forward_only || enc128_rec_floats(w.rg) <= w.enc_rec_floats);
  // CSR plan: real tokens + one shared padding token; the fused kernels walk the HALF tiles (matcha_ragged_plan still builds the 64-row tiles
  // for callers that ask).  Follows the shape, not force_layerwise: the layer-by-layer kernels read neither tiling
  r.half_plan = fused_enabled(s) || r.enc128;
  r.front = r.fused && front_bwd_supported(s.d, s.n_attr) && (options().disable_fused & 2) == 0;
  r.adj_fused = r.front && s.mode == 1 && adj_fused_eligible(s, f);
  r.small = r.fused && fused_small_batch(w.rg);
  // node route (node_front_shape), large-batch kernels only.  Its backward adds the tokens' gradient rows per node with float atomics and leaves
  // no row per TOKEN, so `deterministic` and the row-sparse table gradient (whose sum is bitwise reproducible) stay on the per-token front end
  const bool atomics = !o.deterministic && !o.sparse_table_grad;
  r.node = r.front && node_front_shape(s, B, L) && !r.small && atomics && !options().disable_node_front;
  r.node_r = r.node && !options().disable_node_r;      // ... with the heads' r rows once per node
  r.node_v = r.node_r && !o.forward_only && w.VN && node_v_shape(s, B, L) && !options().disable_node_v;      // ... and, for the backward alone, their value rows
  r.fwd_values = (r.fused && !r.small) ? (r.node_v ? kValuesTable : r.node_r ? kValuesNodeProduct : kValuesToken) : 0;      // (node_operands hands VN to the forward exactly then)
  r.lif = r.fused && o.loss_in_forward && !o.forward_only && has_target(objective, y, w_bce);
  // large batches: the tail's backward inside the forward kernel stops behind its LayerNorms; pff_n1's two convolutions (dZ1, d dyn, the
  // weight gradients) are a kernel of their own right behind it (tail_bwd.hip).  Development switch fused_dbg bit 0: all of it in-kernel.
  r.split_tail = r.lif && !r.small && (options().fused_dbg & 1) == 0;
  // the backward kernel's heads ADD their d x_hat rows (float atomics) unless the sum has to be reproducible: the rows are zeroed by a launch
  // that runs anyway -- tail_bwd64_kernel, or for small batches the loss reduction's (which needs `losses`) -- and the record says so
  r.dx_zeroed = r.lif && atomics && (r.split_tail || r.small) && want_losses;
  // node route with the value table: the forward's tail adds dXs per node, tail_bwd64_kernel zeroes the heads' per-node replicas behind it
  r.node_dx = r.node_v && r.lif && r.split_tail && r.dx_zeroed && node_dx_shape(s, B, L) && !options().disable_node_dx;
  r.paired = r.fused && !options().disable_launch_pairs;
  r.long_rows = false;      // (matcha_forward_long_train notes its own record)
  return r;
}
// Does this forward's plan take the packed row order (ragged.hip)?  Only where every consumer of the plan sees tokens and half tiles, or rows through
// row_src: the fused d = 64 kernels with the loss inside the forward (the training step, every front end, `deterministic` too) and the forward that
// keeps nothing (inference logits).  NOT: the layer-by-layer path and enc128 (head_fwd / head_bwd / the attention kernels index rows by plan row;
// embeddings and attention maps go back to the caller in batch order), a fused forward differentiated by an explicit dlogits (head_bwd reads
// dlogits[b] by plan row), the row-sparse table gradient (its (id, row) list is handed to the caller), and the one-launch plan of small batches.
// The backward needs no record of it: none of its kernels indexes a hyperedge -- they walk the tokens and half tiles the plan left in the workspace.
static bool row_pack_route(const StepRoute& r, const matcha_step_opts& o, int64_t B, const Workspace& w) {
  return r.fused && (r.lif || o.forward_only) && !o.sparse_table_grad && !options().disable_row_pack && ragged_plan_packs(B, w.rg);
}
// what the encoder kernels and head_bwd read for X on this route (kernels.hpp): the per-node tables by tok_key, or X per token
static NodeOperands node_operands(const StepRoute& r, const matcha_shape& s, const Workspace& w) {
  const int64_t rows = (int64_t)s.n_nodes + 1;
  return r.node ? NodeOperands{w.XN, w.rg.tok_key, w.xhN, r.node_r ? w.RN : nullptr, r.node_v ? w.VN : nullptr, rows} : NodeOperands{w.X, nullptr, nullptr, nullptr, nullptr, rows};
}

static int check_shape(const matcha_shape* s, int64_t B, int32_t L) {
  MATCHA_TRY(check_shape_fields(s, nullptr));
  MATCHA_CHECK_ARG(L >= 1 && L <= MATCHA_MAX_L, "L=%d outside 1..%d", L, MATCHA_MAX_L);
  MATCHA_CHECK_ARG(B >= 1 && B * (int64_t)L < (1ll << 31) - 2, "B=%lld must be >= 1 and B*L < 2^31", (long long)B);
  // the layer-by-layer kernels (every embed_dim but 64) put token tiles on grid.y (<= 65 535 tiles of 128 tokens) and launch
  // T * d / 256 workgroups on grid.x: 8.38 M token rows is what they support
  MATCHA_CHECK_ARG(s->d == 64 || B * (int64_t)L + 1 <= 65535ll * 128, "B*L=%lld exceeds the %lld token rows the layer-by-layer kernels (embed_dim != 64) launch",
                   (long long)(B * (int64_t)L), 65535ll * 128);
  return MATCHA_OK;
}

}  // namespace matcha

using namespace matcha;

extern "C" int matcha_abi_version(void) { return MATCHA_ABI_VERSION; }
extern "C" const char* matcha_last_error(void) { return g_err; }
extern "C" int matcha_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

extern "C" int matcha_profile_select(int32_t kernel_class) {
  g_prof_class = kernel_class;
  g_prof_used = 0;
  g_prof_work = 0.0;
  return MATCHA_OK;
}

extern "C" int matcha_launch_log(int32_t on) {
  if (on) g_launch_names = 0;
  g_launch_log = on ? 1 : 0;
  return MATCHA_OK;
}

extern "C" int matcha_launch_log_read(char* out, size_t cap) {
  MATCHA_CHECK_ARG(out && cap > 0, "matcha_launch_log_read: null buffer");
  size_t n = 0;
  out[0] = 0;
  for (int i = 0; i < g_launch_names; ++i) {
    const int k = snprintf(out + n, cap - n, "%s %lld\n", g_launches[i].name, (long long)g_launches[i].n);
    if (k < 0 || (size_t)k >= cap - n) { set_error("matcha_launch_log_read: buffer too small"); return MATCHA_ENOMEM; }
    n += (size_t)k;
  }
  return MATCHA_OK;
}

extern "C" int matcha_route_read(const void* ws, char* out, size_t cap) {
  MATCHA_CHECK_ARG(ws && out && cap > 0, "matcha_route_read: null pointer");
  StepRoute r;
  MATCHA_CHECK_ARG(recorded_route(ws, r), "matcha_route_read: no forward on record for this workspace");
  // "name value\n" for every field of StepRoute, in the struct's order (for_each_route_field, layerwise.hpp)
  size_t n = 0;
  bool fits = true;
  out[0] = 0;
  for_each_route_field(r, [&](const char* name, const auto& v) {
    if (!fits) return;
    const int k = snprintf(out + n, cap - n, "%s %d\n", name, (int)v);
    if (k < 0 || (size_t)k >= cap - n) fits = false;
    else n += (size_t)k;
  });
  if (!fits) { set_error("matcha_route_read: buffer too small"); return MATCHA_ENOMEM; }
  return MATCHA_OK;
}

extern "C" int matcha_profile_read(double* total_ms, int64_t* launches, double* work) {
  double ms = 0.0;
  for (int i = 0; i + 1 < g_prof_used; i += 2) {
    if (hipEventSynchronize(g_prof_ev[i + 1]) != hipSuccess) { set_error("matcha_profile_read: event sync failed"); return MATCHA_EHIP; }
    float t = 0.f;
    if (hipEventElapsedTime(&t, g_prof_ev[i], g_prof_ev[i + 1]) != hipSuccess) { set_error("matcha_profile_read: elapsed failed"); return MATCHA_EHIP; }
    ms += t;
  }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = g_prof_used / 2;
  if (work) *work = g_prof_work;
  g_prof_used = 0;
  g_prof_work = 0.0;
  return MATCHA_OK;
}

extern "C" size_t matcha_workspace_bytes(const matcha_shape* shp, int64_t B, int32_t L) {
  if (check_shape(shp, B, L) != MATCHA_OK) return 0;
  Workspace w;
  return carve(*shp, B, L, nullptr, w);
}

// a forward with opts->forward_only set needs no more than this (equal to matcha_workspace_bytes when the shape has no fused path)
extern "C" size_t matcha_workspace_bytes_forward(const matcha_shape* shp, int64_t B, int32_t L) {
  if (check_shape(shp, B, L) != MATCHA_OK) return 0;
  Workspace w;
  return carve(*shp, B, L, nullptr, w, fused_enabled(*shp));
}

// force_layerwise: run the separate kernels whatever the shape (matcha_get_embedding needs H2 and X in HBM);
// stop_before_head: return after pff_n1 (no logits, no loss)
static int forward_impl(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                        const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L, const float* y,
                        const float* w_bce, float* logits, float* losses, void* ws, size_t ws_bytes,
                        matcha_stream_t stream, bool force_layerwise, bool stop_before_head, int objective) {
  MATCHA_TRY(check_shape(shp, B, L));
  MATCHA_CHECK_ARG(params && frozen && opts && x && ws, "matcha_forward: null pointer");
  MATCHA_CHECK_ARG(((uintptr_t)ws) % 256 == 0, "matcha_forward: workspace must be 256-byte aligned");
  const matcha_shape& s = *shp;
  const matcha_tensors& p = *params;
  hipStream_t st = (hipStream_t)stream;
  Workspace w;
  const size_t need = carve(s, B, L, (char*)ws, w, compact_forward(s, *opts, force_layerwise));
  if (ws_bytes < need) { set_error("matcha_forward: workspace %zu < %zu bytes", ws_bytes, need); return MATCHA_ENOMEM; }
  const int64_t Tn = B * L + 1;                 // upper bound; the true count is *w.rg.count
  const bool train = opts->training != 0;
  MATCHA_CHECK_ARG(!train || opts->seed || (opts->p_drop_adj <= 0 && opts->p_drop_fc1 <= 0 && opts->p_drop_pff <= 0),
                   "matcha_forward: training with dropout needs opts->seed");
  MATCHA_TRY(check_chain_params(p, *frozen, "matcha_forward"));
  const int32_t* cnt = w.rg.count;
  const int64_t* ids = w.rg.tok_id;

  // which kernels will run on this workspace: decided once, here (the plan, the front end and the saved records depend on it), and recorded
  const StepRoute route = decide_route(s, *opts, B, L, w, *frozen, y, w_bce, objective, force_layerwise, losses != nullptr);
  const bool keep = !opts->forward_only;       // a backward may follow: x0, the records and the saved rows are written
  const NodeOperands nx = node_operands(route, s, w);
  const bool tgt = has_target(objective, y, w_bce);
  PlanDeferred deferred;
  deferred.pending = false;
  const bool row_pack = row_pack_route(route, *opts, B, w);
  MATCHA_TRY(launch_ragged_plan(x, B, L, s.n_nodes, opts->status, w.rg, st, route.half_plan ? 1 : 0, route.node ? w.node_ids : nullptr, route.node ? w.node_cnt : nullptr,
                                (route.node && keep) ? w.GN : nullptr,        // ... which also writes the node route's id list and zeroes its accumulator
                                (route.paired && route.node) ? &deferred : nullptr, row_pack, y, w_bce));
  // (paired, node route: the plan's two tile-list passes -- batch only -- ride in the table launches below -- parameters only; the plan stops behind
  // row_fill_kernel, which those launches need for their id list anyway.  deferred.pending: the five-launch plan ran and left them)
  // front end: node rows (K1) + attribute path (K6) + add (Modules.py:263-269)
  float* recon_out = losses ? losses + 1 : nullptr;
  // table front end: the two reconstruction-loss slots are zero; loss_reduce_kernel writes them when it runs anyway
  const bool recon_zero_in_loss = s.mode == 0 && recon_out && route.fused && tgt;
  if (s.mode == 0) MATCHA_CHECK_ARG(p.table, "matcha_forward: table mode without table");
  // (merged / keep: what the layer-by-layer pieces below read of the route)
  const ChainCall chain{s, p, *frozen, *opts, B, L, st, {route.merged_layerwise, false, keep}, "matcha_forward"};
  if (!route.front) {
    MATCHA_TRY(chain_front_fwd(chain, w, recon_out, !recon_zero_in_loss));      // the separate kernels: adj rows or zero slots, x0, X = tanh(next_w(x0))
  } else if (s.mode == 0) {
    if (recon_out && !recon_zero_in_loss) MATCHA_TRY(zero_async(recon_out, 2 * sizeof(float), st));
  } else if (route.adj_fused) {
    MATCHA_TRY(adj_forward(s, p, *frozen, *opts, ids, Tn, nullptr, recon_out, w.adj_ws, w.adj_ws_bytes, st, cnt, w.rg.tok_slot, keep ? w.x0 : nullptr, w.X, keep));
  } else {
    MATCHA_TRY(adj_forward(s, p, *frozen, *opts, ids, Tn, w.node, recon_out, w.adj_ws, w.adj_ws_bytes, st, cnt, w.rg.tok_slot));
  }
  const bool prep_in_front = route.front && !route.adj_fused;      // (adj_fused: x0 and X are already there)
  if (prep_in_front) {
    // gather (or the adj front end's rows) + attribute path + add + next_w + tanh in one kernel (Modules.py:263-270)
    // (fused encoder behind it: the launch also builds the step's weight forms -- folded / merged / fragment-order -- in blocks of their own)
    const PrepSpec prep = {&p, w.folded, w.merged, w.frag};
    if (route.node) {     // the same kernel, once over the ids 0..n_nodes: the per-node tables (the weight-form blocks keep riding in the launch)
      MATCHA_TRY(launch_front_fwd(p, w.node_ids, p.table, nullptr, *frozen, s.n_attr, w.rg, nx.rows, keep ? w.x0N : nullptr, nx.X, st, &prep, w.node_cnt,
                                  deferred.pending ? &deferred.pack : nullptr));
      // ... and, for the backward kernel's staging, their normalised rows
      if (keep) MATCHA_TRY(launch_node_xhat(nx.X, w.node_cnt, nx.rows, nx.xhat, st));
      // ... and the heads' r rows, from the fragment stream the launch above just wrote (training and inference alike)
      if (nx.rn) MATCHA_TRY(launch_node_r(nx.X, w.frag, nx.rows, nx.rn, st, nx.vn, deferred.pending ? &deferred.compact : nullptr));
      else if (deferred.pending) MATCHA_TRY(launch_tile_compact(deferred.compact, st));
    } else
    MATCHA_TRY(launch_front_fwd(p, ids, s.mode == 0 ? p.table : nullptr, s.mode == 0 ? nullptr : w.node, *frozen, s.n_attr, w.rg, Tn, keep ? w.x0 : nullptr, w.X, st, &prep));     // x0 (pre-activation) is only read by the backward pass
  }
  if (keep) note_forward(ws, route); else forget_forward(ws);      // the backward pass on this workspace must follow the same route
  if (route.fused) {
    // everything from X to the logits in one kernel; a forward that will be differentiated saves Y, H1, H2 (768 B per token) -- or, with the
    // tail's backward in the kernel, has the single-wave kernel PARK the rows there between the tail's two halves instead of holding 96 registers
    // per lane (fused_fwd32_tail.hpp) -- and leaves r rows + probabilities per (half tile, head) for fused_bwdh_kernel (w.qkv)
    const bool save = keep && !route.lif;
    if (!prep_in_front) MATCHA_TRY(launch_prep_heads(p, w.folded, w.merged, w.frag, st));      // folded / merged / fragment-order weights of this step
    // the logits go straight to the caller's buffer when no later kernel reads them from the workspace (head_bwd does): one copy less per call
    float* lg_out = (logits && !save) ? logits : w.logits;
    FusedFwdLaunch a;
    a.frag = w.frag; a.small = route.small; a.y = y; a.w = w_bce; a.objective = objective; a.logits = lg_out; a.row_loss = w.row_loss;
    a.x = nx;      // (node route: the kernel reads its row from the per-node table at the plan's sanitised id -- tok_key: 0 for the padding token and foreign ids)
    a.Y = keep ? w.Y : nullptr; a.H1 = keep ? w.H1 : nullptr; a.H2 = keep ? w.H2 : nullptr; a.rimg = keep ? w.qkv : nullptr;
    a.seed = opts->seed; a.p_fc1 = train ? opts->p_drop_fc1 : 0.f; a.p_pff = train ? opts->p_drop_pff : 0.f; a.alpha = opts->alpha;
    a.ddyn0 = route.lif ? w.ddyn0 : nullptr; a.dXs = w.dXs; a.tslab = w.tslab; a.tail_dh2 = route.split_tail ? w.dH2 : nullptr;
    a.dxs_node = route.node_dx ? w.GN : nullptr;      // (zeroed by the plan's launch above)
    a.row_src = row_pack ? w.rg.row_src : nullptr;
    if (row_pack) { a.y = y ? w.rg.y_plan : nullptr; a.w = w_bce ? w.rg.w_plan : nullptr; }      // (the plan's launch copied them in its order)
    MATCHA_CHECK_ARG(!route.node_dx || nx.rows <= Tn, "matcha_forward: the heads' per-node d x_hat rows do not fit dO");
    MATCHA_TRY(launch_fused_fwd32(p, w.rg, B, L, a, st));
    if (route.split_tail)
      MATCHA_TRY(launch_tail_bwd64(p, w.dH2, w.Y, w.H1, w.rg, opts->seed, a.p_fc1, a.p_pff, w.ddyn0, w.tslab2, w.tslab, route.dx_zeroed ? w.dO : nullptr,
                                   route.node_dx ? (int64_t)MATCHA_N_HEAD * nx.rows * 64 : 0, st, w.row_loss, B, tgt ? losses : nullptr, recon_zero_in_loss));      // ... zeroes the backward's d x_hat rows, reduces the loss
    const bool zero_in_loss = route.dx_zeroed && !route.split_tail;
    if (tgt && losses && !route.split_tail)
      MATCHA_TRY(launch_loss_reduce(w.row_loss, B, losses, st, recon_zero_in_loss, zero_in_loss ? w.dO : nullptr, zero_in_loss ? (size_t)Tn * 64 * sizeof(float) : 0));
    if (logits && lg_out != logits && hipMemcpyAsync(logits, w.logits, B * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess) {
      set_error("logits copy failed"); return MATCHA_EHIP;
    }
    return MATCHA_OK;
  }
  // layer by layer (layerwise.hip): the attention block -- at embed_dim 128 as one kernel: LayerNorms, merged heads, attention, fc1 + dropout + mask,
  // X -> Y; a training forward leaves r rows + probabilities -- then pff_n1 and the head
  if (route.enc128) {
    MATCHA_TRY(merged_weights(s, p, w, st));
    MATCHA_TRY(launch_enc128_fwd(p, w.lwB, w.lwM, w.X, w.rg, B, L, w.Y, keep ? w.enc_rec : nullptr, w.enc, w.rg.tok_slot, opts->seed,
                                 (train && opts->p_drop_fc1 > 0.f) ? opts->p_drop_fc1 : 0.f, st));
  } else {
    MATCHA_TRY(chain_attn_fwd(chain, w));
  }
  return chain_tail_fwd(chain, w, y, w_bce, logits, losses, objective, stop_before_head);
}

extern "C" int matcha_forward(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                              const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L, const float* y,
                              const float* w_bce, float* logits, float* losses, void* ws, size_t ws_bytes,
                              matcha_stream_t stream) {
  return forward_impl(shp, params, frozen, opts, x, B, L, y, w_bce, logits, losses, ws, ws_bytes, stream, false, false, MATCHA_OBJECTIVE_BCE);
}

extern "C" int matcha_forward_objective(int32_t objective, const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                                        const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L, const float* y,
                                        const float* w, float* logits, float* losses, void* ws, size_t ws_bytes, matcha_stream_t stream) {
  MATCHA_TRY(check_objective(objective, "matcha_forward_objective"));
  return forward_impl(shp, params, frozen, opts, x, B, L, y, w, logits, losses, ws, ws_bytes, stream, false, false, objective);
}

extern "C" int matcha_get_embedding(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                                    const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L, float* dynamic,
                                    float* static_, float* attn, float* losses, void* ws, size_t ws_bytes, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(dynamic && static_ && opts, "matcha_get_embedding: null pointer");
  matcha_step_opts o = *opts;
  o.forward_only = 0;                  // full workspace layout: the layer-by-layer path keeps H2 and X in HBM
  o.loss_in_forward = 0;
  MATCHA_TRY(forward_impl(shp, params, frozen, &o, x, B, L, nullptr, nullptr, nullptr, losses, ws, ws_bytes, stream, true, true, MATCHA_OBJECTIVE_BCE));
  Workspace w;
  carve(*shp, B, L, (char*)ws, w);
  if (attn && hipMemcpyAsync(attn, w.P, (size_t)B * MATCHA_N_HEAD * L * L * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
    set_error("matcha_get_embedding: attention copy failed"); return MATCHA_EHIP;
  }
  return launch_expand_embedding(x, B, L, shp->d, w.rg.row_off, w.H2, w.X, params->pff_ln_g, params->pff_ln_b, dynamic, static_, (hipStream_t)stream);
}

// Development aid, not part of include/matcha_hip.h: the workspace layout as text, one "name offset bytes" line per buffer, so that
// tools/debug/ws_diff.py can say WHICH buffer a differing workspace byte belongs to (round 5: which output the failing forward variant lost).
extern "C" int matcha_debug_layout(const matcha_shape* shp, int64_t B, int32_t L, char* out, size_t cap) {
  MATCHA_TRY(check_shape(shp, B, L));
  MATCHA_CHECK_ARG(out && cap > 0, "matcha_debug_layout: null buffer");
  Workspace w;
  char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);
  const size_t total = carve(*shp, B, L, base, w);
  struct { const char* name; const void* p; } f[] = {
      {"plan", w.rg.row_off}, {"x0", w.x0}, {"X", w.X}, {"qin", w.qin}, {"kin", w.kin}, {"vin", w.vin}, {"stats", w.stats}, {"Q", w.Q}, {"K", w.K}, {"V", w.V},
      {"P", w.P}, {"O_dxh", w.O}, {"Y", w.Y}, {"H1", w.H1}, {"H2", w.H2}, {"row_loss", w.row_loss}, {"logits", w.logits}, {"node", w.node}, {"dH2", w.dH2},
      {"dXs", w.dXs}, {"dZ1", w.dZ1}, {"ddyn0", w.ddyn0}, {"dZ0", w.dZ0}, {"dX0", w.dX0}, {"slab", w.slab}, {"gemm_ws", w.gemm_ws}, {"adj_ws", w.adj_ws},
      {"folded", w.folded}, {"frag", w.frag}, {"merged", w.merged}, {"lwB", w.lwB}, {"lwM", w.lwM}, {"lwdB", w.lwdB}, {"lwdM", w.lwdM}, {"enc", w.enc}, {"fb_ws", w.fb_ws},
      {"tpart", w.tpart}, {"tslab", w.tslab}, {"tslab2", w.tslab2}, {"qkv_records", w.qkv}, {"front_ws", w.front_ws}, {"tg_ws", w.tg_ws}, {"XN", w.XN}, {"x0N", w.x0N}, {"xhN", w.xhN}, {"GN", w.GN},
      {"node_ids", w.node_ids}, {"node_cnt", w.node_cnt}, {"RN", w.RN}, {"VN", w.VN}, {"row_src", w.rg.row_src}, {"pack_sched", w.rg.sched}};
  size_t n = 0;
  for (const auto& e : f) {
    if (!e.p) continue;
    const int k = snprintf(out + n, cap - n, "%s %zu\n", e.name, (size_t)((const char*)e.p - base));
    if (k < 0 || (size_t)k >= cap - n) { set_error("matcha_debug_layout: buffer too small"); return MATCHA_ENOMEM; }
    n += (size_t)k;
  }
  const int k = snprintf(out + n, cap - n, "end %zu\n", total);
  if (k < 0 || (size_t)k >= cap - n) { set_error("matcha_debug_layout: buffer too small"); return MATCHA_ENOMEM; }
  return MATCHA_OK;
}

extern "C" int matcha_random_chrom_dev_supported(const matcha_shape* shp, const matcha_frozen* frozen) {
  if (!shp || !frozen) return 0;
  if (shp->mode == 0) return 1;
  return adj_fused_eligible(*shp, *frozen) && fused_enabled(*shp) && front_bwd_supported(shp->d, shp->n_attr) ? 1 : 0;
}

extern "C" int matcha_set_option(const char* name, int32_t value) {
  MATCHA_CHECK_ARG(name, "matcha_set_option: null name");
  for (const OptionName& n : kOptionNames)
    if (strcmp(n.name, name) == 0) { options().*(n.field) = value; return MATCHA_OK; }
  set_error("matcha_set_option: unknown option '%s'", name);
  return MATCHA_EINVAL;
}

extern "C" int32_t matcha_get_option(const char* name) {
  if (!name) return -1;
  for (const OptionName& n : kOptionNames)
    if (strcmp(n.name, name) == 0) return options().*(n.field);
  return -1;
}

extern "C" int matcha_table_grad_rows(const matcha_shape* shp, int64_t B, int32_t L, void* ws, size_t ws_bytes,
                                      const int32_t** ids, const float** rows, const int32_t** n_tokens, int64_t* cap) {
  MATCHA_TRY(check_shape(shp, B, L));
  MATCHA_CHECK_ARG(ws && ids && rows && cap, "matcha_table_grad_rows: null pointer");
  MATCHA_CHECK_ARG(shp->mode == 0, "matcha_table_grad_rows: table mode only");
  Workspace w;
  const size_t need = carve(*shp, B, L, (char*)ws, w);
  if (ws_bytes < need) { set_error("matcha_table_grad_rows: workspace %zu < %zu bytes", ws_bytes, need); return MATCHA_ENOMEM; }
  *ids = w.rg.tok_key;
  *rows = w.dX0;
  if (n_tokens) *n_tokens = w.rg.count + 1;
  *cap = B * (int64_t)L + 1;
  return MATCHA_OK;
}

static int backward_impl(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                         const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L, const float* y,
                         const float* w_bce, const float* dlogits, const float* drecon, matcha_tensors* grads,
                         int32_t* touched, void* ws, size_t ws_bytes, matcha_stream_t stream, int objective) {
  MATCHA_TRY(check_shape(shp, B, L));
  MATCHA_CHECK_ARG(params && frozen && opts && x && ws && grads, "matcha_backward: null pointer");
  MATCHA_CHECK_ARG(dlogits || has_target(objective, y, w_bce),
                   objective == MATCHA_OBJECTIVE_BCE ? "matcha_backward: need dlogits or (y, w)" : "matcha_backward: need dlogits or y");
  const matcha_shape& s = *shp;
  const matcha_tensors& p = *params;
  matcha_tensors& g_ = *grads;
  hipStream_t st = (hipStream_t)stream;
  Workspace w;
  const size_t need = carve(s, B, L, (char*)ws, w);
  if (ws_bytes < need) { set_error("matcha_backward: workspace %zu < %zu bytes", ws_bytes, need); return MATCHA_ENOMEM; }
  const int64_t Tn = B * L + 1;
  const int64_t* ids = w.rg.tok_id;            // the plan (row_off, tok_id, tok_slot, count) is still in the workspace

  // which kernels the forward ran on this workspace is what decides, not the option table now: everything below follows `route`
  StepRoute route;
  // (a record of matcha_forward_long_train is none of this entry point's: refused like no record, and left for matcha_backward_long)
  MATCHA_CHECK_ARG(recorded_route(ws, route) && !route.long_rows,
                   "matcha_backward: no matcha_forward on record for this workspace (one backward per forward, same ws pointer)");
  // fused route: this call's options and targets must ask for the loss where the forward computed it (head_bwd over rows the forward only parked, or no ddyn0)
  MATCHA_CHECK_ARG(!route.fused || route.lif == (opts->loss_in_forward && has_target(objective, y, w_bce)),
                   "matcha_backward: loss_in_forward / targets differ from the forward's on this workspace");
  MATCHA_CHECK_ARG(!(route.lif && dlogits), "matcha_backward: opts->loss_in_forward excludes an explicit dlogits");
  forget_forward(ws);                                   // one backward per forward: from here on the saved activations are being overwritten
  const bool tail_in_bwd = route.lif && (route.split_tail || route.small);     // the launch that sums the backward kernel's slabs sums the forward's tail slabs too
  const bool dx_zeroed = route.dx_zeroed && !opts->deterministic && !opts->sparse_table_grad;      // tail_bwd64_kernel / the loss reduction zeroed the heads' d x_hat buffer
  TailReduceArgs tail_args;
  const NodeOperands nx = node_operands(route, s, w);   // node route: X lives in the per-node table, rows by tok_key
  const ChainCall chain{s, p, *frozen, *opts, B, L, st, {route.merged_layerwise, false, true}, "matcha_backward"};
  if (route.lif) {
    // ddyn0 and dXs were produced by matcha_forward; only the parameter-gradient partials remain to be summed (fused_fwd32.hip).  Split tail: one
    // row-major slab per workgroup of tail_bwd64_kernel -- the convolutions' gradients and the half tiles' LayerNorm / classifier vectors (summed
    // along its walk), 512 slabs;  small batches: one slab per half tile (a few dozen);  otherwise two passes of their own
    if (route.split_tail) tail_reduce_args(w.tslab2, w.rg, L, g_, true, tail_bwd_grid(), true, tail_args);
    else if (route.small) tail_reduce_args(w.tslab, w.rg, L, g_, true, -1, false, tail_args);
    else MATCHA_TRY(launch_tail_reduce(w.tslab, w.rg, L, g_, st, true, w.tpart));
  } else {
    MATCHA_TRY(chain_tail_bwd(chain, w, nx.X, nx.xrow, y, w_bce, dlogits, objective, g_));      // head_bwd and pff_n1's products: dH2, dXs, dZ1, ddyn0
  }
  if (route.fused) {
    // attention block (fc1, attention, Q/K/V projections, the three LayerNorms) from X and ddyn0 in one head-major kernel;
    // the forward pass left the folded weights in w.folded.  w.dO doubles as the 8 per-head d x_hat slabs.
    // the eight heads add their d x_hat into ONE buffer with float atomics (executed at the memory side; per-head slabs are 8 x 256 B per token written
    // and read back) -- or, node_dx, into one per-node replica each.  `deterministic` and the row-sparse table gradient (whose sum is bitwise reproducible) keep the slabs and their fixed order: per call
    const bool dx_atomic = !opts->deterministic && !opts->sparse_table_grad;
    MATCHA_CHECK_ARG(!route.node || dx_atomic, "matcha_backward: deterministic / sparse_table_grad differ from the forward's on this workspace");
    FusedBwdLaunch a;
    a.folded = w.folded; a.merged = w.merged; a.x = nx; a.dDyn = w.ddyn0; a.dXs = w.dXs; a.rimg = w.qkv;
    a.dxh = w.dO; a.ws = w.fb_ws; a.dZ0 = route.front ? nullptr : w.dZ0;
    a.dx_atomic = dx_atomic; a.dx_zeroed = dx_zeroed; a.tail = tail_in_bwd ? &tail_args : nullptr;
    a.dx_node = route.node_dx;      // dxh = the heads' per-node replicas [8][n_nodes + 1][64] (zeroed by tail_bwd64_kernel)
    // paired launches follow the record like every other choice here.  On the node route the last launch that writes an encoder gradient is then
    // node_scatter_kernel (either body hosts fb_unfold2's vectors): encoder_done is recorded behind IT
    Unfold2Args unfold2;
    const bool unfold2_in_scatter = route.paired && route.front && route.node;
    a.paired = route.paired; a.unfold2 = unfold2_in_scatter ? &unfold2 : nullptr;
    MATCHA_CHECK_ARG(!route.node_dx || (dx_zeroed && nx.rows <= Tn), "matcha_backward: the heads' per-node d x_hat rows do not fit dO");
    MATCHA_TRY(launch_fused_bwd_merged(p, w.rg, B, L, a, g_, st));
    if (!unfold2_in_scatter) MATCHA_TRY(encoder_done(*opts, st));
    if (route.front) {
      // LayerNorm backward of the summed partials + next_w + attribute_nn backward + embedding scatter in one kernel
      if (s.mode == 0) MATCHA_CHECK_ARG(g_.table, "matcha_backward: table mode without a table gradient buffer");
      if (route.node) {
        // the tokens' rows LNbwd(d x_hat) + dXs added per node (one pass over the tokens), then tanh' / next_w / attribute_nn / the table row
        // once per node: front_bwd_kernel over the ids 0..n_nodes with the sums in dXs' place, one writer per table-gradient row
        // (node_dx: the producers added per node already -- the launch sums the heads' replicas in a fixed order and finishes each node row in place)
        MATCHA_TRY(launch_node_scatter(nx.X, w.dO, fused_bwd_dxpad(w.fb_ws), w.dXs, w.rg, Tn, w.GN, st, route.node_dx ? w.node_cnt : nullptr, nx.rows,
                                       unfold2_in_scatter ? &unfold2 : nullptr));
        if (unfold2_in_scatter) MATCHA_TRY(encoder_done(*opts, st));
        MATCHA_TRY(launch_front_bwd(p, nx.X, nullptr, 1, nx.rows, fused_bwd_dxpad(w.fb_ws), w.GN, w.x0N, w.node_ids, *frozen, s.n_attr, w.rg, nullptr, g_.table, w.front_ws, g_, st, touched, w.node_cnt));
        return MATCHA_OK;
      }
      const bool rows_out = s.mode == 1 || opts->deterministic || opts->sparse_table_grad;     // dX0 rows instead of float atomics
      MATCHA_TRY(launch_front_bwd(p, w.X, w.dO, dx_atomic ? 1 : MATCHA_N_HEAD, Tn, fused_bwd_dxpad(w.fb_ws), w.dXs, w.x0, ids, *frozen, s.n_attr, w.rg,
                                  rows_out ? w.dX0 : nullptr, rows_out ? nullptr : g_.table, w.front_ws, g_, st, s.mode == 0 ? touched : nullptr));
      if (s.mode == 0) MATCHA_TRY(table_gradient(s, *opts, w, Tn, g_, st));       // (the two `touched` flags were set by front_slab_reduce_kernel)
      else MATCHA_TRY(adj_backward(s, p, *frozen, *opts, ids, Tn, w.dX0, drecon, g_, touched, w.adj_ws, w.adj_ws_bytes, w.gemm_ws, w.gemm_ws_bytes, st, w.rg.tok_slot, route.adj_fused));
      return MATCHA_OK;
    }
  } else if (route.enc128) {
    // embed_dim 128, fused attention block: dB_all / dM_all (LayerNorm affines taken back out) + d x_hat in one kernel, then the chain rule to
    // w_qs / w_ks / w_vs / fc1 and the LayerNorm backward (enc128.hip); dxh lives in qin's buffer
    MATCHA_TRY(launch_enc128_bwd(p, w.lwB, w.lwM, w.X, w.ddyn0, w.dXs, w.rg, B, L, w.dqin, w.enc_rec, w.enc, w.lwdB, w.lwdM, g_, w.dZ0, st));
    MATCHA_TRY(merged_chain(s, p, g_, w, st));
    MATCHA_TRY(encoder_done(*opts, st));
  } else {
    MATCHA_TRY(chain_attn_bwd(chain, w, g_));      // the heads in the forward's formulation, ln3_bwd, the encoder_done event
  }
  // next_w, attribute_nn, the node embedding's gradient (layerwise.hip)
  return chain_front_bwd(chain, w, drecon, g_, touched);
}

extern "C" int matcha_backward(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                               const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L, const float* y,
                               const float* w_bce, const float* dlogits, const float* drecon, matcha_tensors* grads,
                               int32_t* touched, void* ws, size_t ws_bytes, matcha_stream_t stream) {
  return backward_impl(shp, params, frozen, opts, x, B, L, y, w_bce, dlogits, drecon, grads, touched, ws, ws_bytes, stream, MATCHA_OBJECTIVE_BCE);
}

extern "C" int matcha_backward_objective(int32_t objective, const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                                         const matcha_step_opts* opts, const int64_t* x, int64_t B, int32_t L, const float* y,
                                         const float* w, const float* dlogits, const float* drecon, matcha_tensors* grads,
                                         int32_t* touched, void* ws, size_t ws_bytes, matcha_stream_t stream) {
  MATCHA_TRY(check_objective(objective, "matcha_backward_objective"));
  return backward_impl(shp, params, frozen, opts, x, B, L, y, w, dlogits, drecon, grads, touched, ws, ws_bytes, stream, objective);
}

extern "C" int matcha_node_embeddings(const matcha_shape* shp, const matcha_tensors* params, const matcha_frozen* frozen,
                                      const int64_t* ids, int64_t T, float* rows, void* ws, size_t ws_bytes,
                                      int32_t* status, matcha_stream_t stream) {
  MATCHA_CHECK_ARG(shp && params && frozen && ids && rows, "matcha_node_embeddings: null pointer");
  MATCHA_CHECK_ARG(shp->d >= 4 && shp->d <= 256 && shp->d % 4 == 0, "matcha_node_embeddings: d=%d", shp->d);
  hipStream_t st = (hipStream_t)stream;
  if (shp->mode == 0) {
    // Wrap_Embedding: plain row gather (Modules.py:33-34)
    MATCHA_CHECK_ARG(params->table, "matcha_node_embeddings: null table");
    return launch_gather_rows(ids, T, shp->d, params->table, shp->n_nodes, rows, status, st);
  }
  MATCHA_TRY(launch_check_ids(ids, T, shp->n_nodes, status, st));      // out-of-range ids land in the padding bucket (chrom_of)
  matcha_step_opts o;
  memset(&o, 0, sizeof(o));
  o.random_chrom = -1;   // no reconstruction branch
  MATCHA_CHECK_ARG(ws && ws_bytes >= adj_workspace_bytes(*shp, T), "matcha_node_embeddings: adj mode needs a workspace of matcha_workspace_bytes()");
  return adj_forward(*shp, *params, *frozen, o, ids, T, rows, nullptr, ws, ws_bytes, st, nullptr, nullptr, nullptr, nullptr, false, true);
}
