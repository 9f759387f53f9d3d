// What the long rows' host chains share: forward_long.hip (matcha_forward_long, matcha_forward_long_train) and backward_long.hip (matcha_backward_long).
#pragma once
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

int check_shape_long(const matcha_shape* s, int64_t B, int32_t L, const char* fn);
// merged heads (r = qin B_all^T, shared key / value rows, dyn = Z M_all^T) where embed_dim is a multiple of 64, unless the option table says otherwise
bool long_merged(const matcha_shape& s);
// one product of the token-level chain: M rows bounded by the plan's device-side token count, dropout counters keyed by token slot b L + l
GemmArgs gemm_long(const Ragged& rg, const float* A, const float* Bm, float* Cm, int64_t M, int64_t N, int64_t K, bool b_kn = false);

// The training layout for long rows: every activation the backward reads is kept in a buffer of its own (O is NOT written over Q), the
// gradients of the 8 d-wide tensors too, except dO, which takes O's place once the fc1 weight gradient has read it.  Per token, in floats:
// x0, X, qin, kin, vin, Y, H1, H2, dH2, dXs, dZ1, ddyn0, dZ0, dX0, dqin, dkin, dvin (17 d), the LayerNorm statistics (2), r / Z / dR with merged
// heads (24 d: 41 d in all), Q, K, V, O, dQ, dK, dV without (56 d: 73 d in all), + d on the adj front end; + the plan's 20 B (8 B per row).
struct LongTrainWs {
  Ragged rg; uint32_t* mask;
  float *x0, *X, *qin, *kin, *vin, *stats, *Q, *K, *V, *O, *Y, *H1, *H2, *logits, *node;      // saved by the forward (merged: Q = r, O = Z, no K / V)
  float *dH2, *dXs, *dZ1, *ddyn0, *dO, *dQ, *dK, *dV, *dqin, *dkin, *dvin, *dZ0, *dX0;       // the backward's (merged: dQ = dR, no dK / dV)
  float* slab; size_t slab_bytes;        // column-sum slabs (LayerNorm / tail parameter gradients), the attention's padding-row slabs
  float* gemm_ws; size_t gemm_ws_bytes;  // TN GEMM slabs
  void* adj_ws; size_t adj_ws_bytes;
  float *lwB, *lwM, *lwdB, *lwdM;        // merged heads: B_all [8 d, d], M_all [d, 8 d] and their gradients
};
size_t carve_long_train(const matcha_shape& s, int64_t B, int L, char* base, LongTrainWs& w, bool merged);

// One backward per forward: the host-side record of matcha_forward_long_train per workspace pointer (the head formulation it ran), consumed
// by matcha_backward_long.  Bounded, evicted oldest-first, guarded by a mutex -- as matcha_forward / matcha_backward keep theirs (model.hip).
void long_note_forward(const void* ws, bool merged);
bool long_take_forward(const void* ws, bool* merged);      // false: no forward on record; true: the record is removed

}  // namespace matcha
