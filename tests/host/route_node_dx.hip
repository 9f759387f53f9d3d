// decide_route's node_dx field (model.hip: the encoder's input gradients summed per node at their producers) under AddressSanitizer +
// UndefinedBehaviorSanitizer on the host, next to tests/host/host_checks.hip: the same host-only objects, model.hip included as source so
// that its static functions are reachable, a driver of its own.  No kernel runs.  Checked over shapes x front ends x per-call options x
// every switch: what the field implies; that its switch takes out this field and no other; that the heads' per-node replicas
// [8][n_nodes + 1][64] fit the dO buffer they are carved in wherever the field is set; the sizes the size rule fixes; the record.
#include "host_driver.hpp"

int main() {
  matcha_set_option("fused_dbg", 0);
  const int kFront = route_switch("disable_node_front"), kR = route_switch("disable_node_r"), kV = route_switch("disable_node_v"), kDx = route_switch("disable_node_dx");
  int seen = 0;
  for (int sw = 0; sw < kNumRouteSwitches; ++sw) {
    set_route_switch(sw, true);
    for (int d : {16, 64, 128})
      for (int mode = 0; mode < 2; ++mode)
        for (int n_nodes : {150, 3067})
          for (int64_t B : {2ll, 1024ll, 3072ll, 8192ll, 65536ll})
            for (int L : {5, 8})
              for (int bits = 0; bits < 128; ++bits) {
                const matcha_shape s = mode ? shape(d, 24, n_nodes, 23, 1, 250) : shape(d, 24, n_nodes, 0, 0, 0);
                matcha_step_opts o = train_opts();
                o.forward_only = bits & 1; o.deterministic = (bits >> 1) & 1; o.loss_in_forward = (bits >> 2) & 1; o.sparse_table_grad = (bits >> 5) & 1;
                const bool targets = (bits >> 3) & 1, force = (bits >> 4) & 1, want_losses = (bits >> 6) & 1;
                Workspace w;
                const StepRoute r = route_of(s, o, B, L, targets, force, want_losses, &w);
                if (r.node_dx) {
                  CHECK(r.node_v && r.node_r && r.node && r.lif && r.split_tail && r.dx_zeroed && !r.small && !r.compact);
                  CHECK(mode == 0 && d == 64 && targets && want_losses && o.loss_in_forward && !o.forward_only && !o.deterministic && !o.sparse_table_grad && !force);
                  CHECK(sw != kDx && sw != kV && sw != kR && sw != kFront);
                  const int64_t Tn = B * L + 1, rows = (int64_t)n_nodes + 1;
                  CHECK(Tn >= 64 * rows);
                  // the replicas inside dO, the dXs sums inside GN: [8][rows][64] floats of the 8 d Tn there, [rows][64] of GN's
                  CHECK(w.dO && w.GN && w.VN && (size_t)MATCHA_N_HEAD * rows * 64 <= (size_t)Tn * MATCHA_N_HEAD * s.d);
                  CHECK((const char*)(w.dO + (size_t)MATCHA_N_HEAD * rows * 64) <= (const char*)w.Y);      // O is followed by Y in the layout
                  seen += sw == 0;
                }
                if (sw == kDx) {      // the switch takes out this field and no other: decide_route reads it for node_dx alone, and no field reads node_dx
                  matcha_set_option("disable_node_dx", 0);
                  const StepRoute on = route_of(s, o, B, L, targets, force, want_losses);
                  matcha_set_option("disable_node_dx", 1);
                  CHECK(!r.node_dx && route_diff(r, on) == (on.node_dx ? Fields{"node_dx"} : Fields{}));
                  CHECK(on.node_dx == (on.node_v && on.lif && on.split_tail && on.dx_zeroed));
                }
              }
    set_route_switch(sw, false);
  }
  CHECK(seen > 0);
  // hg38 1 Mb (3 068 table rows), a training step with targets: the field from 65 536 rows on, as the value table; c23 from 3 072 rows
  const matcha_step_opts o = train_opts();
  for (int64_t B : {8192ll, 16384ll, 32768ll, 65536ll}) CHECK(route_of(shape(64, 24, 3067, 0, 0, 0), o, B, 5, true).node_dx == (B == 65536));
  CHECK(route_of(shape(64, 24, 150, 0, 0, 0), o, 3072, 5, true).node_dx);
  CHECK(!route_of(shape(64, 24, 150, 0, 0, 0), o, 3072, 5, true, false, false).node_dx);       // nobody asked for the losses: no launch zeroes the replicas
  CHECK(!route_of(shape(64, 24, 150, 0, 0, 0), o, 2048, 5, true).node_dx);        // the small-batch kernels
  // the record hands the field to the backward as it is
  const void* ws = reinterpret_cast<const void*>((uintptr_t)1 << 12);
  StepRoute r = route_of(shape(64, 24, 150, 0, 0, 0), o, 3072, 5, true), got;
  for (int v = 0; v < 2; ++v) {
    r.node_dx = v;
    note_forward(ws, r);
    CHECK(recorded_route(ws, got) && got.node_dx == (bool)v && route_diff(got, r).empty());
  }
  forget_forward(ws);
  CHECK(!recorded_route(ws, got));
  // the option table knows the switch by name and from the environment's spelling
  CHECK(matcha_get_option("disable_node_dx") == 0 && matcha_set_option("disable_node_dx", 1) == MATCHA_OK && matcha_get_option("disable_node_dx") == 1);
  matcha_set_option("disable_node_dx", 0);
  return finish("NODE_DX ROUTE CHECKS");
}
