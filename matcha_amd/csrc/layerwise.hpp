// The layer-by-layer token chain, written once (layerwise.hip): embed_fwd, next_w, the three LayerNorms, the heads' projections, the attention,
// fc1, pff_n1 and the classifier head, and their backward, as a fixed sequence of launches over the Tr real tokens + ONE shared padding token
// of a plan.  Every entry point that runs the chain calls these pieces on a TokenChain filled by its own workspace layout:
//   matcha_forward / matcha_backward off the fused embed_dim-64 route and matcha_get_embedding (model.hip: Workspace, rows of up to 8 columns),
//   matcha_forward_long, matcha_get_embedding_long, matcha_forward_long_train / matcha_backward_long (forward_long.hip: LongWs, rows of up to 32).
// What differs between them -- the plan, the attention kernels, which buffers alias which -- stays with the caller; the forward record per
// workspace pointer (StepRoute) is shared too, so a forward of either kind voids what the other left on the same pointer.
#pragma once
#include <unordered_map>
#include <utility>

#include "kernels.hpp"

namespace matcha {

// adj_frontend.hip
int adj_forward(const matcha_shape& s, const matcha_tensors& p, const matcha_frozen& f, const matcha_step_opts& o, const int64_t* x, int64_t T,
                float* node_out, float* recon_out, void* ws, size_t ws_bytes, hipStream_t st, const int32_t* t_dev, const int32_t* slot_map,
                float* fused_x0 = nullptr, float* fused_X = nullptr, bool save = false, bool fused_node = false);
int adj_backward(const matcha_shape& s, const matcha_tensors& p, const matcha_frozen& f, const matcha_step_opts& o, const int64_t* x, int64_t T,
                 float* dnode, const float* drecon, matcha_tensors& g, int32_t* touched, void* ws, size_t ws_bytes, void* gemm_ws,
                 size_t gemm_ws_bytes, hipStream_t st, const int32_t* slot_map, bool fused = false);
size_t adj_workspace_bytes(const matcha_shape& s, int64_t T);

// The chain's buffers: pointers only.  Which of them own memory and which alias another is the layout's business (model.hip: carve,
// forward_long.hip: carve_long, carve_long_train); a buffer the layout does not have is null.
struct TokenChain {
  Ragged rg;
  // saved by the forward (merged heads: Q holds r, O holds Z, every head attends the shared rows kin / vin; P: the short attention's probabilities
  // [B, 8, L, L] in the workspace -- under long_attn, where no layout keeps them, null or the CALLER's padded [8 B, L, L] tensor, which
  // attn_long_prob_kernel then fills completely (matcha_get_embedding_long))
  float *x0, *X, *qin, *kin, *vin, *stats, *Q, *K, *V, *P, *O, *Y, *H1, *H2, *row_loss, *logits, *node;
  // the backward's
  float *dH2, *dXs, *dZ1, *ddyn0, *dO, *dQ, *dK, *dV, *dqin, *dkin, *dvin, *dZ0, *dX0;
  float* slab;      size_t slab_bytes;    // column-sum slabs (LayerNorm / tail parameter gradients, the attention's padding-token gradients)
  float* gemm_ws;   size_t gemm_ws_bytes; // TN GEMM slabs
  void* adj_ws;     size_t adj_ws_bytes;
  void* tg_ws;      size_t tg_ws_bytes;   // table mode: sort scratch of the deterministic table gradient (table_grad.hip)
  float *lwB, *lwM, *lwdB, *lwdM;         // merged heads: B_all [8d, d], M_all [d, 8d] and their gradients
  uint32_t* mask;                         // long rows: the plan's scratch, a row's real columns as a bit set [B] (ragged_long.hip); read under long_attn only
};

// What the call sites differ in.
struct ChainOpts {
  bool merged;      // merged heads (r = qin B_all^T, dyn = Z M_all^T: two products per head) instead of the reference's four
  bool long_attn;   // attention_long.hip / attention_long_bwd.hip (k <= 32, no P kept) instead of attention.hip / attention_wide.hip (k <= 8, P kept).
                    // A flag of its own, not L > 8: the long entry points take L from 2
  bool keep;        // a backward follows: activations are kept.  With long_attn the padding token's O row -- which that attention does not write, and
                    // which then feeds dM / dWfc1 as a factor of a zero gradient row -- is zeroed; a layout whose O lies over Q must not ask for it
};

// One call's constants, as the entry point received them.  fn: its name in error texts
struct ChainCall {
  const matcha_shape& s; const matcha_tensors& p; const matcha_frozen& f; const matcha_step_opts& o;
  int64_t B; int L; hipStream_t st; ChainOpts c; const char* fn;
  int64_t Tn() const { return B * L + 1; }      // upper bound of token rows; the true count is *rg.count
};

// one product of the chain: M rows bounded by the plan's device-side token count, dropout counters keyed by the token's original slot b L + l
GemmArgs gemm1(const TokenChain& w, const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K, bool b_kn = false);
// B_all / M_all of this step (two launches' worth of small GEMMs in one), and the chain rule from their gradients to w_q / w_k / w_v / fc1
int merged_weights(const matcha_shape& s, const matcha_tensors& p, const TokenChain& w, hipStream_t st);
int merged_chain(const matcha_shape& s, const matcha_tensors& p, matcha_tensors& g, const TokenChain& w, hipStream_t st);
// slab_bytes / gemm_ws_bytes of a layout: the colsum slabs, the attention backward's slab of the given kind, the TN GEMM shapes of the chain
void chain_scratch_bytes(const matcha_shape& s, int64_t B, int L, bool long_attn, TokenChain& w);
// the part of the shape check every entry point shares (fn != null: the texts carry "fn: " in front)
int check_shape_fields(const matcha_shape* s, const char* fn);
// every parameter the chain reads is there (the table and the adj front end's tensors are the front end's own checks)
int check_chain_params(const matcha_tensors& p, const matcha_frozen& f, const char* fn);

// ---- the pieces: straight-line, each where the fused routes cut the chain ------------------------------------------------------------
// adj front end (recon_out: losses + 1 or null) or, zero_recon, the table front end's two zero reconstruction slots;  x0;  X = tanh(next_w x0)
int chain_front_fwd(const ChainCall& c, const TokenChain& w, float* recon_out, bool zero_recon);
// ln3, the heads' projections, attention, Y = mask(dropout(fc1(O)))          (replaced by enc128; with the next piece, by the fused encoder)
int chain_attn_fwd(const ChainCall& c, const TokenChain& w);
// pff_n1, then -- unless stop_before_head -- the classifier head.  y, w_bce, losses: optional.  A layout without a logits buffer has the head write the
// caller's `logits` directly; otherwise they are copied there when the caller passed one
int chain_tail_fwd(const ChainCall& c, const TokenChain& w, const float* y, const float* w_bce, float* logits, float* losses, int objective,
                   bool stop_before_head);
// head_bwd (X / xrow: the per-token X and null, or the node route's table and its row map) and pff_n1's two TN / NN pairs: dH2, dXs, dZ1, ddyn0
int chain_tail_bwd(const ChainCall& c, const TokenChain& w, const float* X, const int32_t* xrow, const float* y, const float* w_bce, const float* dlogits,
                   int objective, matcha_tensors& g);
// fc1, attention, projections in the forward's formulation, ln3_bwd (-> dZ0), the encoder_done event
int chain_attn_bwd(const ChainCall& c, const TokenChain& w, matcha_tensors& g);
// next_w, attribute_nn, then the table gradient (scatter, or sorted / row-sparse as c.o asks) or the adj front end's backward; the `touched` flags
int chain_front_bwd(const ChainCall& c, const TokenChain& w, const float* drecon, matcha_tensors& g, int32_t* touched);

// Table mode, after the backward left one gradient row per compact token in w.dX0 (ids in w.rg.tok_key): add them into the dense table gradient
// deterministically (table_grad.hip; opts.deterministic) -- unless the caller asked for the row-sparse form (opts.sparse_table_grad: the list stays
// in the workspace for matcha_table_grad_rows / the data-parallel exchange)
int table_gradient(const matcha_shape& s, const matcha_step_opts& o, const TokenChain& w, int64_t Tn, matcha_tensors& g, hipStream_t st);
// opts->encoder_done_event: every gradient from ln_q_g to cls_b is final at this point of the stream (include/matcha_hip.h)
int encoder_done(const matcha_step_opts& o, hipStream_t st, const char* fn = "matcha_backward");
// MATCHA_DEBUG_NAN=1: count the non-finite values in the valid rows of a buffer and print them (synchronises; development only)
void nan_check(const char* name, const float* p, const int32_t* rows_dev, int64_t rows, int64_t width, hipStream_t st);

// ---- the forward record ----------------------------------------------------------------------------------------------------------------
// The kernel route of one step: every decision of the forward that a later line of it, or the backward on the same workspace, depends on.
// decide_route (model.hip, behind the workspace layout it reads) fills it ONCE per short forward; matcha_forward_long_train notes one with
// long_rows set and its head formulation in merged_layerwise.
// StepRoute::fwd_values: per token inside the kernel (a second product per head) | per token from the node's x_hat with the r rows gathered (the route
// without the value table: inference, disable_node_v) | gathered from the value table VN next to the r rows (no product in the head loop)
constexpr int kValuesToken = 1, kValuesNodeProduct = 2, kValuesTable = 3;
struct StepRoute {
  bool compact;                  // workspace layout of a forward that will not be differentiated (carve)
  bool half_plan;                // the ragged plan stops at the half tiles (level 1: no 64-row tile list, no token -> tile map)
  bool fused;                    // embed_dim 64: X -> logits in one forward kernel, the attention block's backward in one (fused_fwd32.hip, fused_bwd.hip)
  bool merged_layerwise, enc128; // layer by layer: merged heads;  at embed_dim 128 the attention block as ONE kernel pair (enc128.hip)
  bool front, adj_fused;         // fused front end and its backward (front_fused.hip);  the adj front end as ONE kernel over the chromosome-sorted rows (adj_fused.hip)
  bool small;                    // the small-batch kernels (fused_small_batch)
  bool lif;                      // the tail's backward ran inside the forward kernel: Y / H1 / H2 hold parked rows, ddyn0 and dXs are final
  bool split_tail, dx_zeroed;    // ... up to its LayerNorms, the convolutions' as tail_bwd64_kernel;  the forward zeroed the d x_hat rows the backward's heads add into
  bool node;                     // table front end per NODE: X lives in the per-node table, rows by tok_key
  bool node_r, node_v;           // ... the heads' r rows gathered from the per-node table (none in the record);  ... and the value table VN, gathered by the forward and left for the backward
  int fwd_values;                // where fused_fwd32_kernel took the heads' value rows y_h = M_h x_hat from (kValues*; 0: another kernel ran the forward)
  bool node_dx;                  // ... d x_hat and dXs added per NODE by their producers (AH in dO, AS in GN): node_scatter_kernel is the per-node finisher
  bool paired;                   // fused route: independent small launches share a launch -- the chain rule's blocks un-fold their own rows; with node_dx
                                 // the node route the final vectors ride in node_scatter_kernel and the plan's tile lists in the table launches.  Off: the launches of the step one by one
  bool long_rows;                // the forward was matcha_forward_long_train: the long rows' training layout, consumed by matcha_backward_long alone
};
// Every member of a route (const or not) handed to f(name, member), in the struct's order: the ONE list of the fields besides the struct itself --
// matcha_route_read prints from it and the host checks compare, count and set fields through it.  A structured binding names ALL members of an
// aggregate, so a field added to (or taken out of) the struct stops this function from compiling until the list follows.
template <class Route, class F>
inline void for_each_route_field(Route& r, F&& f) {
  auto& [compact, half_plan, fused, merged_layerwise, enc128, front, adj_fused, small, lif, split_tail, dx_zeroed, node, node_r, node_v, fwd_values, node_dx,
         paired, long_rows] = r;
#define MATCHA_ROUTE_FIELD(x) f(#x, x)
  MATCHA_ROUTE_FIELD(compact); MATCHA_ROUTE_FIELD(half_plan); MATCHA_ROUTE_FIELD(fused); MATCHA_ROUTE_FIELD(merged_layerwise); MATCHA_ROUTE_FIELD(enc128);
  MATCHA_ROUTE_FIELD(front); MATCHA_ROUTE_FIELD(adj_fused); MATCHA_ROUTE_FIELD(small); MATCHA_ROUTE_FIELD(lif); MATCHA_ROUTE_FIELD(split_tail);
  MATCHA_ROUTE_FIELD(dx_zeroed); MATCHA_ROUTE_FIELD(node); MATCHA_ROUTE_FIELD(node_r); MATCHA_ROUTE_FIELD(node_v); MATCHA_ROUTE_FIELD(fwd_values);
  MATCHA_ROUTE_FIELD(node_dx); MATCHA_ROUTE_FIELD(paired); MATCHA_ROUTE_FIELD(long_rows);
#undef MATCHA_ROUTE_FIELD
}
// Which route the forward that last ran on a workspace took.  The backward keys off THIS record and reads no option: the two calls are
// separate on the autograd path and the switches are process-wide, so a flip between them would otherwise make the backward consume records
// nobody wrote.  Host-side record per workspace pointer (the decision picks a kernel, so it cannot live in device memory without a
// synchronisation); bounded, evicted oldest-first, guarded by a mutex.  ONE map for every entry point: any forward on a pointer replaces the
// record (a training forward) or drops it (a forward that keeps nothing), the backward that consumed it drops it, and a backward of the
// other kind -- matcha_backward on a long_rows record, matcha_backward_long on any other -- finds no record of its own and is refused
// before any launch.
extern std::unordered_map<const void*, std::pair<StepRoute, uint64_t>> g_fwd_state;     // ws -> (route, age)
void note_forward(const void* ws, const StepRoute& route);
bool recorded_route(const void* ws, StepRoute& route);       // false: no forward on record for this workspace
void forget_forward(const void* ws);

}  // namespace matcha
