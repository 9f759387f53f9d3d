// What every host check driver of tests/host/ shares.  The drivers are stand-alone programs on the library's host-only objects, compiled with
// AddressSanitizer + UndefinedBehaviorSanitizer (csrc/Makefile: host-asan) and run by tests/test_cpu_host_checks.py; no kernel runs in any of them.
// model.hip is included as SOURCE so that its static functions (carve, check_shape, decide_route) are reachable.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../matcha_amd/csrc/model.hip"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    ++g_checks;                                                                  \
    if (!(cond)) { ++g_fail; fprintf(stderr, "CHECK FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #cond, matcha_last_error()); } \
  } while (0)

// the counts and, with no failure, the line the runner looks for ("ALL <what> PASSED"); main's exit status
static int finish(const char* what) {
  printf("%d checks, %d failed\n", g_checks, g_fail);
  if (g_fail == 0) printf("ALL %s PASSED\n", what);
  return g_fail ? 1 : 0;
}

// an entry point's refusal: MATCHA_EINVAL with `word` in the message
static bool refused(int rc, const char* word) {
  const bool hit = rc == MATCHA_EINVAL && strstr(matcha_last_error(), word) != nullptr;
  if (!hit) fprintf(stderr, "  rc=%d error=\"%s\" (wanted \"%s\")\n", rc, matcha_last_error(), word);
  return hit;
}

static matcha_shape shape(int d, int n_attr, int n_nodes, int n_chrom, int mode, int max_bins) {
  matcha_shape s;
  s.d = d; s.n_attr = n_attr; s.n_nodes = n_nodes; s.n_chrom = n_chrom; s.mode = mode; s.max_bins = max_bins;
  return s;
}
static matcha_step_opts train_opts() {
  matcha_step_opts o;
  memset(&o, 0, sizeof(o));
  o.training = 1; o.loss_in_forward = 1;
  return o;
}

// ---- the step's kernel route (model.hip: decide_route; layerwise.hpp: StepRoute, for_each_route_field) ----
static StepRoute route_of(const matcha_shape& s, const matcha_step_opts& o, int64_t B, int L, bool targets, bool force_layerwise = false, bool want_losses = true,
                          Workspace* wout = nullptr) {
  Workspace w;
  char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);      // the layout only: nothing is dereferenced
  carve(s, B, L, base, w, compact_forward(s, o, force_layerwise));
  matcha_frozen f;
  memset(&f, 0, sizeof(f));
  f.feat_row_pad = 64;                                                 // what the fused adj kernels take
  static const float t[1] = {0.f};
  if (wout) *wout = w;
  return decide_route(s, o, B, L, w, f, targets ? t : nullptr, targets ? t : nullptr, MATCHA_OBJECTIVE_BCE, force_layerwise, want_losses);
}

// every switch of the option table that decide_route reads, with the values it tells apart; entry 0 is "no switch set".  A sweep `over the switches` in
// any driver is a loop over this table, so a new switch is swept by all of them.
struct RouteSwitch { const char* name; int value; };
static const RouteSwitch kRouteSwitches[] = {{"", 0}, {"disable_fused", 1}, {"disable_fused", 2}, {"disable_merged", 1}, {"disable_small_batch", 1},
                                             {"disable_wide_gemm", 1}, {"disable_node_front", 1}, {"disable_node_r", 1}, {"disable_node_v", 1},
                                             {"disable_node_dx", 1}, {"disable_launch_pairs", 1}};
static const int kNumRouteSwitches = (int)(sizeof(kRouteSwitches) / sizeof(kRouteSwitches[0]));
static int route_switch(const char* name, int value = 1) {      // its index in the table
  for (int i = 0; i < kNumRouteSwitches; ++i)
    if (!strcmp(kRouteSwitches[i].name, name) && kRouteSwitches[i].value == value) return i;
  fprintf(stderr, "no route switch %s=%d\n", name, value);
  abort();
}
static void set_route_switch(int sw, bool on) {
  if (sw) CHECK(matcha_set_option(kRouteSwitches[sw].name, on ? kRouteSwitches[sw].value : 0) == MATCHA_OK);
}

typedef std::vector<std::string> Fields;
// the names of the fields in which two routes differ, in the struct's order: an assertion on it speaks for ALL fields, also those added later
static Fields route_diff(const StepRoute& a, const StepRoute& b) {
  std::vector<int> va;
  for_each_route_field(a, [&](const char*, const auto& v) { va.push_back((int)v); });
  Fields out;
  size_t i = 0;
  for_each_route_field(b, [&](const char* name, const auto& v) { if (va[i++] != (int)v) out.push_back(name); });
  return out;
}
static Fields route_field_names() {
  Fields out;
  const StepRoute r = {};
  for_each_route_field(r, [&](const char* name, const auto&) { out.push_back(name); });
  return out;
}
static void set_route_field(StepRoute& r, int index, int value) {
  int i = 0;
  for_each_route_field(r, [&](const char*, auto& v) { if (i++ == index) v = value; });
}
