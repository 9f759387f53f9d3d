// decide_route's `paired` field (model.hip: independent small launches of the fused step share a launch) under AddressSanitizer +
// UndefinedBehaviorSanitizer on the host, next to tests/host/route_node_dx.hip: the same host-only objects, model.hip included as source so
// that its static functions are reachable, a driver of its own.  No kernel runs.  Checked over shapes x front ends x per-call options x
// every switch: the field is the fused route's and nothing else's; its switch takes out this field and no other; no other switch touches it
// beyond what it does to `fused`; the record hands it to the backward; the plan's deferral (what the forward leaves to the table launches)
// exists exactly where the five-launch plan runs at level 1.
#include "host_driver.hpp"

int main() {
  matcha_set_option("fused_dbg", 0);
  const int kPairs = route_switch("disable_launch_pairs"), kLayerwise = route_switch("disable_fused", 1), kUnmerged = route_switch("disable_merged");
  int seen = 0, seen_node_dx = 0;
  for (int sw = 0; sw < kNumRouteSwitches; ++sw) {
    set_route_switch(sw, true);
    for (int d : {16, 64, 128})
      for (int mode = 0; mode < 2; ++mode)
        for (int n_nodes : {150, 3067})
          for (int64_t B : {2ll, 384ll, 1024ll, 3072ll, 8192ll, 65536ll})
            for (int L : {5, 8})
              for (int bits = 0; bits < 128; ++bits) {
                const matcha_shape s = mode ? shape(d, 24, n_nodes, 23, 1, 250) : shape(d, 24, n_nodes, 0, 0, 0);
                matcha_step_opts o = train_opts();
                o.forward_only = bits & 1; o.deterministic = (bits >> 1) & 1; o.loss_in_forward = (bits >> 2) & 1; o.sparse_table_grad = (bits >> 5) & 1;
                const bool targets = (bits >> 3) & 1, force = (bits >> 4) & 1, want_losses = (bits >> 6) & 1;
                const StepRoute r = route_of(s, o, B, L, targets, force, want_losses);
                // the fused route's field: set wherever the fused d = 64 kernels run (the merged backward's chain rule runs on every one of them) and
                // the switch is off -- whatever the front end, the batch size and the per-call options are
                CHECK(r.paired == (r.fused && sw != kPairs));
                if (r.paired) {
                  CHECK(d == 64 && !force && sw != kLayerwise && sw != kUnmerged);
                  ++seen;
                  seen_node_dx += r.node_dx;
                }
                if (sw == kPairs) {      // the switch takes out this field and no other: decide_route reads it for `paired` alone, and no field reads `paired`
                  matcha_set_option("disable_launch_pairs", 0);
                  const StepRoute on = route_of(s, o, B, L, targets, force, want_losses);
                  matcha_set_option("disable_launch_pairs", 1);
                  CHECK(!r.paired && on.paired == on.fused && route_diff(r, on) == (on.paired ? Fields{"paired"} : Fields{}));
                }
              }
    set_route_switch(sw, false);
  }
  CHECK(seen > 0 && seen_node_dx > 0);
  // the headline and the tests' shapes: a training step with targets
  const matcha_step_opts o = train_opts();
  {
    const StepRoute h = route_of(shape(64, 24, 3067, 0, 0, 0), o, 65536, 5, true);
    CHECK(h.paired && h.node && h.node_r && h.node_v && h.node_dx && h.half_plan);
    const StepRoute c = route_of(shape(64, 24, 150, 0, 0, 0), o, 3072, 5, true);
    CHECK(c.paired && c.node_dx);
    const StepRoute c8 = route_of(shape(64, 24, 150, 0, 0, 0), o, 1536, 8, true);
    CHECK(c8.paired && c8.node_dx);
    const StepRoute sm = route_of(shape(64, 24, 150, 0, 0, 0), o, 384, 5, true);
    CHECK(sm.paired && sm.small && !sm.node);
    const StepRoute adj = route_of(shape(64, 24, 3067, 23, 1, 250), o, 65536, 5, true);
    CHECK(adj.paired && !adj.node);
    matcha_step_opts fo = o;
    fo.training = 0; fo.forward_only = 1; fo.loss_in_forward = 0;
    const StepRoute inf = route_of(shape(64, 24, 150, 0, 0, 0), fo, 3072, 5, false, false, false);
    CHECK(inf.paired && inf.node && inf.node_r && !inf.node_v && inf.compact);
    CHECK(!route_of(shape(128, 24, 3067, 0, 0, 0), o, 8192, 5, true).paired);
  }
  // the record hands the field to the backward as it is
  const void* ws = reinterpret_cast<const void*>((uintptr_t)1 << 12);
  StepRoute r = route_of(shape(64, 24, 150, 0, 0, 0), o, 3072, 5, true), got;
  for (int v = 0; v < 2; ++v) {
    r.paired = v;
    note_forward(ws, r);
    matcha_set_option("disable_launch_pairs", 1 - v);      // the option table at the time of the backward is not what decides
    CHECK(recorded_route(ws, got) && got.paired == (bool)v && route_diff(got, r).empty());
    matcha_set_option("disable_launch_pairs", 0);
  }
  forget_forward(ws);
  CHECK(!recorded_route(ws, got));
  // the plan's deferral: the two tile-list passes are left to the caller exactly at level 1 of the five-launch plan (host side only: the launches
  // fail without a device and are not issued here -- the rule is the launcher's first lines, restated)
  {
    Ragged rg;
    char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);
    ragged_carve(65536, 5, base, rg);
    CHECK(rg.nsb == 163 && rg.nsb <= kCompactRoleSb);
    ragged_carve(384, 5, base, rg);
    CHECK(rg.nsb == 1);
    ragged_carve(1 << 20, 8, base, rg);
    CHECK(rg.nsb > kCompactRoleSb);                        // beyond the role form: launch_node_r falls back to the stand-alone kernel
  }
  // the option table knows the switch by name
  CHECK(matcha_get_option("disable_launch_pairs") == 0 && matcha_set_option("disable_launch_pairs", 1) == MATCHA_OK && matcha_get_option("disable_launch_pairs") == 1);
  matcha_set_option("disable_launch_pairs", 0);
  return finish("LAUNCH PAIR ROUTE CHECKS");
}
