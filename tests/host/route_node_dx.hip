// decide_route's node_dx field (model.hip: the encoder's input gradients summed per node at their producers) under AddressSanitizer +
// UndefinedBehaviorSanitizer on the host, next to tests/host/host_checks.hip: the same host-only objects, model.hip included as source so
// that its static functions are reachable, a driver of its own.  No kernel runs.  Checked over shapes x front ends x per-call options x
// every switch: what the field implies; that its switch takes out this field and no other; that the heads' per-node replicas
// [8][n_nodes + 1][64] fit the dO buffer they are carved in wherever the field is set; the sizes the size rule fixes; the record.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../matcha_amd/csrc/model.hip"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    ++g_checks;                                                                  \
    if (!(cond)) { ++g_fail; fprintf(stderr, "CHECK FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

static matcha_shape shape(int d, int n_attr, int n_nodes, int n_chrom, int mode, int max_bins) {
  matcha_shape s;
  s.d = d; s.n_attr = n_attr; s.n_nodes = n_nodes; s.n_chrom = n_chrom; s.mode = mode; s.max_bins = max_bins;
  return s;
}
static StepRoute route_of(const matcha_shape& s, const matcha_step_opts& o, int64_t B, int L, bool targets, bool force_layerwise, bool want_losses, Workspace* wout = nullptr) {
  Workspace w;
  char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);      // the layout only: nothing is dereferenced
  carve(s, B, L, base, w, compact_forward(s, o, force_layerwise));
  matcha_frozen f;
  memset(&f, 0, sizeof(f));
  f.feat_row_pad = 64;
  static const float t[1] = {0.f};
  if (wout) *wout = w;
  return decide_route(s, o, B, L, w, f, targets ? t : nullptr, targets ? t : nullptr, MATCHA_OBJECTIVE_BCE, force_layerwise, want_losses);
}
static bool same_but_dx(const StepRoute& a, const StepRoute& b) {
  return a.compact == b.compact && a.half_plan == b.half_plan && a.fused == b.fused && a.merged_layerwise == b.merged_layerwise && a.enc128 == b.enc128 &&
         a.front == b.front && a.adj_fused == b.adj_fused && a.small == b.small && a.lif == b.lif && a.split_tail == b.split_tail &&
         a.dx_zeroed == b.dx_zeroed && a.node == b.node && a.node_r == b.node_r && a.node_v == b.node_v;
}

int main() {
  matcha_set_option("fused_dbg", 0);
  const char* switches[] = {"", "disable_fused", "disable_fused", "disable_merged", "disable_small_batch", "disable_wide_gemm", "disable_node_front", "disable_node_r", "disable_node_v", "disable_node_dx"};
  const int values[] = {0, 1, 2, 1, 1, 1, 1, 1, 1, 1};
  int seen = 0;
  for (int sw = 0; sw < 10; ++sw) {
    if (sw) CHECK(matcha_set_option(switches[sw], values[sw]) == MATCHA_OK);
    for (int d : {16, 64, 128})
      for (int mode = 0; mode < 2; ++mode)
        for (int n_nodes : {150, 3067})
          for (int64_t B : {2ll, 1024ll, 3072ll, 8192ll, 65536ll})
            for (int L : {5, 8})
              for (int bits = 0; bits < 128; ++bits) {
                const matcha_shape s = mode ? shape(d, 24, n_nodes, 23, 1, 250) : shape(d, 24, n_nodes, 0, 0, 0);
                matcha_step_opts o;
                memset(&o, 0, sizeof(o));
                o.training = 1;
                o.forward_only = bits & 1; o.deterministic = (bits >> 1) & 1; o.loss_in_forward = (bits >> 2) & 1; o.sparse_table_grad = (bits >> 5) & 1;
                const bool targets = (bits >> 3) & 1, force = (bits >> 4) & 1, want_losses = (bits >> 6) & 1;
                Workspace w;
                const StepRoute r = route_of(s, o, B, L, targets, force, want_losses, &w);
                if (r.node_dx) {
                  CHECK(r.node_v && r.node_r && r.node && r.lif && r.split_tail && r.dx_zeroed && !r.small && !r.compact);
                  CHECK(mode == 0 && d == 64 && targets && want_losses && o.loss_in_forward && !o.forward_only && !o.deterministic && !o.sparse_table_grad && !force);
                  CHECK(sw != 9 && sw != 8 && sw != 7 && sw != 6);
                  const int64_t Tn = B * L + 1, rows = (int64_t)n_nodes + 1;
                  CHECK(Tn >= 64 * rows);
                  // the replicas inside dO, the dXs sums inside GN: [8][rows][64] floats of the 8 d Tn there, [rows][64] of GN's
                  CHECK(w.dO && w.GN && w.VN && (size_t)MATCHA_N_HEAD * rows * 64 <= (size_t)Tn * MATCHA_N_HEAD * s.d);
                  CHECK((const char*)(w.dO + (size_t)MATCHA_N_HEAD * rows * 64) <= (const char*)w.Y);      // O is followed by Y in the layout
                  seen += sw == 0;
                }
                if (sw == 9) {      // the switch takes out this field and no other
                  matcha_set_option("disable_node_dx", 0);
                  const StepRoute on = route_of(s, o, B, L, targets, force, want_losses);
                  matcha_set_option("disable_node_dx", 1);
                  CHECK(!r.node_dx && same_but_dx(r, on));
                  CHECK(on.node_dx == (on.node_v && on.lif && on.split_tail && on.dx_zeroed));
                }
              }
    if (sw) matcha_set_option(switches[sw], 0);
  }
  CHECK(seen > 0);
  // hg38 1 Mb (3 068 table rows), a training step with targets: the field from 65 536 rows on, as the value table; c23 from 3 072 rows
  matcha_step_opts o;
  memset(&o, 0, sizeof(o));
  o.training = 1; o.loss_in_forward = 1;
  for (int64_t B : {8192ll, 16384ll, 32768ll, 65536ll}) CHECK(route_of(shape(64, 24, 3067, 0, 0, 0), o, B, 5, true, false, true).node_dx == (B == 65536));
  CHECK(route_of(shape(64, 24, 150, 0, 0, 0), o, 3072, 5, true, false, true).node_dx);
  CHECK(!route_of(shape(64, 24, 150, 0, 0, 0), o, 3072, 5, true, false, false).node_dx);       // nobody asked for the losses: no launch zeroes the replicas
  CHECK(!route_of(shape(64, 24, 150, 0, 0, 0), o, 2048, 5, true, false, true).node_dx);        // the small-batch kernels
  // the record hands the field to the backward as it is
  const void* ws = reinterpret_cast<const void*>((uintptr_t)1 << 12);
  StepRoute r = route_of(shape(64, 24, 150, 0, 0, 0), o, 3072, 5, true, false, true), got;
  for (int v = 0; v < 2; ++v) {
    r.node_dx = v;
    note_forward(ws, r);
    CHECK(recorded_route(ws, got) && got.node_dx == (bool)v && same_but_dx(got, r));
  }
  forget_forward(ws);
  CHECK(!recorded_route(ws, got));
  // the option table knows the switch by name and from the environment's spelling
  CHECK(matcha_get_option("disable_node_dx") == 0 && matcha_set_option("disable_node_dx", 1) == MATCHA_OK && matcha_get_option("disable_node_dx") == 1);
  matcha_set_option("disable_node_dx", 0);
  printf("%d checks, %d failed\n", g_checks, g_fail);
  if (g_fail == 0) printf("ALL NODE_DX ROUTE CHECKS PASSED\n");
  return g_fail ? 1 : 0;
}
