// Host-side checks of libmatcha_hip's NON-KERNEL logic under AddressSanitizer + UndefinedBehaviorSanitizer (SURVEY.md §5
// "sanitizers"; GPU ASan is not available on the MI355X pool, so this is where sanitizers run): every source file of the
// library is compiled for the host only (hipcc --offload-host-only -fsanitize=address,undefined), this driver is linked
// against those objects and executed by tests/test_cpu_host_checks.py in the CPU container.  No kernel runs here -- launches
// fail with "no device" and the entry points must turn that into MATCHA_EHIP; what IS exercised, instrumented:
//   * argument validation and error reporting of every extern "C" entry point (null pointers, bad shapes, misaligned or
//     too-small workspaces);
//   * every workspace-sizing function over a sweep of shapes (monotone in B, 256-byte granules, no overflow);
//   * the workspace carving of model.hip / ragged.hip: every region inside the buffer, ordered, aligned -- checked by writing
//     the first and last byte of every region into an exactly-sized heap buffer (ASan traps an overrun);
//   * the option table (matcha_set_option / environment parsing);
//   * the step's kernel route (decide_route: implications over a sweep of shapes, options and switches, the sizes the history fixed) and the
//     per-workspace record of it, as the library keeps it and as matcha_route_read prints it;
//   * the C restatement of the ragged plan (oracle/c/ragged_plan.c), fuzzed with its invariants.
// host_driver.hpp holds what the drivers of this directory share.
#include <random>

#include "host_driver.hpp"

extern "C" int64_t matcha_oracle_ragged_halves(const int32_t* row_off, int64_t B, const int32_t* tile_meta, int64_t n_tiles, int32_t* half_meta,
                                               int64_t halves_cap, int32_t* tok_tile);
extern "C" int64_t matcha_oracle_ragged_plan(const int64_t* x, int64_t B, int32_t L, int64_t n_nodes, int32_t* row_off, int32_t* tok_slot,
                                             int64_t* tok_id, int32_t* tok_key, int32_t* tok_pos, int32_t* count, int32_t* tile_meta,
                                             int64_t tiles_cap, int32_t* status);

static void touch(char* base, size_t total, const void* p, const void* next) {
  // first and last byte of the region [p, next): ASan traps if either lies outside the heap block
  if (!p) return;
  char* a = (char*)p;
  char* b = next ? (char*)next : base + total;
  CHECK(a >= base && a <= base + total && b >= a && b <= base + total);
  CHECK(((uintptr_t)(a - base)) % 256 == 0);
  if (b > a) { a[0] = 1; b[-1] = 1; }
}

static void check_carve(const matcha_shape& s, int64_t B, int L, bool compact) {
  Workspace w0;
  const size_t total = carve(s, B, L, nullptr, w0, compact);
  CHECK(total > 0 && total % 256 == 0);
  char* raw = (char*)malloc(total + 256);
  char* base = (char*)(((uintptr_t)raw + 255) / 256 * 256);          // the library requires 256-byte alignment
  const size_t slack = (size_t)(raw + total + 256 - (base + total));
  (void)slack;
  Workspace w;
  const size_t t2 = carve(s, B, L, base, w, compact);
  CHECK(t2 == total);
  // regions in carve order (null = size 0 in this layout)
  const void* order[] = {w.rg.row_off, w.rg.tok_slot, w.rg.tok_id, w.rg.count, w.rg.blk_sum, w.rg.tok_pos, w.rg.tok_key, w.rg.tile_meta,
                         w.rg.sb_tiles, w.rg.sb_cnt, w.rg.sb_first, w.x0, w.X, w.qin, w.kin, w.vin, w.stats, w.Q, w.K, w.V, w.P, w.O, w.Y, w.H1,
                         w.H2, w.row_loss, w.logits, w.node, w.dH2, w.dXs, w.dZ1, w.ddyn0, w.dZ0,
                         w.dX0, w.slab, w.gemm_ws, w.adj_ws, w.folded, w.fb_ws, w.tslab, w.qkv, w.front_ws, w.tg_ws};
  // the attention block's gradients live in the buffers of the activations they replace (model.hip::carve)
  CHECK(w.dO == w.O && w.dQ == w.K && w.dK == w.Q && w.dV == w.V && w.dqin == w.qin && w.dkin == w.kin && w.dvin == w.vin);
  const int n = (int)(sizeof(order) / sizeof(order[0]));
  const char* prev = base;
  for (int i = 0; i < n; ++i) {
    if (!order[i]) continue;
    CHECK((const char*)order[i] >= prev);                             // carve order is address order
    prev = (const char*)order[i];
    const void* next = nullptr;
    for (int j = i + 1; j < n; ++j)
      if (order[j] && order[j] != order[i]) { next = order[j]; break; }
    touch(base, total, order[i], next);
  }
  free(raw);
}

static void check_sizes_and_validation() {
  const int dims[] = {8, 16, 32, 64, 128, 192, 256};
  for (int d : dims)
    for (int mode = 0; mode < 2; ++mode)
      for (int L = 1; L <= 8; L += (L < 5 ? 1 : 3)) {
        matcha_shape s = mode ? shape(d, 24, 3067, 23, 1, 250) : shape(d, 24, 3067, 0, 0, 0);
        size_t prev = 0;
        for (int64_t B : {1ll, 2ll, 96ll, 384ll, 4097ll, 65536ll}) {
          const size_t full = matcha_workspace_bytes(&s, B, L), fwd = matcha_workspace_bytes_forward(&s, B, L);
          CHECK(full > 0 && full % 256 == 0 && fwd > 0 && fwd <= full && full >= prev);
          prev = full;
          if (B <= 4097) { check_carve(s, B, L, false); if (d == 64) check_carve(s, B, L, true); }
        }
      }
  // shapes the library must reject, with a message
  matcha_shape bad = shape(20, 24, 10, 0, 0, 0);
  CHECK(matcha_workspace_bytes(&bad, 4, 3) == 0 && strstr(matcha_last_error(), "embed_dim") != nullptr);
  matcha_shape ok = shape(64, 24, 3067, 0, 0, 0);
  CHECK(matcha_workspace_bytes(&ok, 4, 9) == 0);                       // L > 8
  CHECK(matcha_workspace_bytes(&ok, 0, 3) == 0);                       // B < 1
  CHECK(matcha_workspace_bytes(&ok, (1ll << 31), 2) == 0);             // B * L overflows int32 token indices
  CHECK(matcha_workspace_bytes(nullptr, 4, 3) == 0);
  matcha_shape wide = shape(128, 24, 3067, 0, 0, 0);
  CHECK(matcha_workspace_bytes(&wide, 65535ll * 128, 1) == 0);         // beyond what the layer-by-layer launches support
  matcha_shape nomode = shape(64, 24, 3067, 0, 2, 0);
  CHECK(matcha_workspace_bytes(&nomode, 4, 3) == 0);
  matcha_shape noattr = shape(64, 0, 3067, 0, 0, 0);
  CHECK(matcha_workspace_bytes(&noattr, 4, 3) == 0);
  // sizing helpers of the other entry points
  CHECK(matcha_hashset_bytes(0) >= 1024 * 4 && matcha_hashset_bytes(1000) >= 2 * 1000 * 4 && matcha_hashset_bytes(100000000) >= 2ull * 100000000 * 4);
  CHECK(matcha_hashset_bytes(-5) == matcha_hashset_bytes(0));
  CHECK(matcha_gemm_tn_workspace_bytes(512, 64, 100000) > 0);
  CHECK(matcha_attn_bwd_workspace_bytes(65536, 64) > 0);
  CHECK(matcha_scatter_rows_workspace_bytes(1 << 20, 256, 1000000) > 3ull * (1 << 20) * 4);
  CHECK(matcha_ragged_plan_bytes(65536, 5) > 0 && matcha_ragged_plan_bytes(65536, 9) == 0 && matcha_ragged_plan_bytes(0, 5) == 0);
  CHECK(matcha_corrcoef_workspace_bytes(2491) > 0);
  if (matcha_device_count() > 0) {        // these two size rocPRIM scratch by asking rocPRIM, which needs a device to pick its configuration
    CHECK(matcha_quantile_workspace_bytes(1000000) > 0);
    CHECK(matcha_kmer_workspace_bytes(1000000, 3, 3067) > 0);
  }
}

static void check_entry_point_errors() {
  matcha_shape s = shape(64, 24, 3067, 0, 0, 0);
  matcha_tensors p;
  memset(&p, 0, sizeof(p));
  matcha_frozen f;
  memset(&f, 0, sizeof(f));
  matcha_step_opts o;
  memset(&o, 0, sizeof(o));
  const size_t need = matcha_workspace_bytes(&s, 8, 3);
  char* raw = (char*)malloc(need + 512);
  char* ws = (char*)(((uintptr_t)raw + 255) / 256 * 256);
  int64_t x[24] = {1, 2, 3};
  float logits[8], losses[3];
  // null pointers / bad alignment / too small a workspace: rejected before anything is launched
  CHECK(matcha_forward(&s, nullptr, &f, &o, x, 8, 3, nullptr, nullptr, logits, losses, ws, need, nullptr) == MATCHA_EINVAL);
  CHECK(matcha_forward(&s, &p, &f, &o, x, 8, 3, nullptr, nullptr, logits, losses, ws + 4, need, nullptr) == MATCHA_EINVAL);
  CHECK(matcha_forward(&s, &p, &f, &o, x, 8, 3, nullptr, nullptr, logits, losses, ws, need / 2, nullptr) == MATCHA_ENOMEM);
  CHECK(strstr(matcha_last_error(), "workspace") != nullptr);
  CHECK(matcha_forward(&s, &p, &f, &o, x, 8, 3, nullptr, nullptr, logits, losses, ws, need, nullptr) == MATCHA_EINVAL);   // parameter pointers are null
  o.training = 1; o.p_drop_fc1 = 0.3f;
  CHECK(matcha_forward(&s, &p, &f, &o, x, 8, 3, nullptr, nullptr, logits, losses, ws, need, nullptr) == MATCHA_EINVAL);   // dropout without a seed
  matcha_tensors g;
  memset(&g, 0, sizeof(g));
  CHECK(matcha_backward(&s, &p, &f, &o, x, 8, 3, nullptr, nullptr, nullptr, nullptr, &g, nullptr, ws, need, nullptr) == MATCHA_EINVAL);   // neither dlogits nor (y, w)
  CHECK(matcha_backward(&s, &p, &f, &o, x, 8, 3, nullptr, nullptr, logits, nullptr, &g, nullptr, ws, need / 2, nullptr) == MATCHA_ENOMEM);
  CHECK(matcha_node_embeddings(&s, &p, &f, x, 3, logits, nullptr, 0, nullptr, nullptr) == MATCHA_EINVAL);                 // null table
  CHECK(matcha_get_embedding(&s, &p, &f, &o, x, 8, 3, nullptr, nullptr, nullptr, nullptr, ws, need, nullptr) == MATCHA_EINVAL);
  const int32_t *ids = nullptr, *nt = nullptr;
  const float* rows = nullptr;
  int64_t cap = 0;
  CHECK(matcha_table_grad_rows(&s, 8, 3, ws, need, &ids, &rows, &nt, &cap) == MATCHA_OK && cap == 25);
  CHECK((const char*)ids >= ws && (const char*)ids + 25 * 4 <= ws + need && (const char*)rows >= ws && (const char*)(rows + 25 * 64) <= ws + need);
  matcha_shape adj = shape(64, 24, 3067, 23, 1, 250);
  CHECK(matcha_table_grad_rows(&adj, 8, 3, ws, need, &ids, &rows, &nt, &cap) == MATCHA_EINVAL);
  CHECK(matcha_adamw_step(nullptr, nullptr, nullptr, nullptr, 10, nullptr, 1, nullptr, nullptr, nullptr, nullptr, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, nullptr) != MATCHA_OK);
  CHECK(matcha_hashset_build(ws, 16, x, 100, 3, nullptr) == MATCHA_EINVAL);                                               // set buffer too small
  CHECK(matcha_hashset_build(ws, need, x, 3, 9, nullptr) == MATCHA_EINVAL);
  CHECK(matcha_neg_sample(nullptr, nullptr, 0, 3, x, 8, 3, 3, 0, nullptr, 10, nullptr, 1, nullptr, x, nullptr, nullptr) == MATCHA_EINVAL);
  CHECK(matcha_scatter_rows(nullptr, nullptr, 10, 64, 100, nullptr, nullptr, 0, nullptr) == MATCHA_EINVAL);
  CHECK(matcha_scatter_rows((const int32_t*)x, logits, 10, 63, 100, logits, ws, need, nullptr) == MATCHA_EINVAL);        // d % 4
  matcha_ragged_view view;
  CHECK(matcha_ragged_plan(x, 8, 3, 100, nullptr, ws, 64, &view, nullptr) == MATCHA_ENOMEM);
  CHECK(matcha_ragged_plan(x, 8, 9, 100, nullptr, ws, need, &view, nullptr) == MATCHA_EINVAL);
  CHECK(matcha_gemm(7, logits, logits, logits, 8, 8, 8, nullptr, nullptr, nullptr, nullptr, 0, nullptr) != MATCHA_OK);
  // an empty or negative contraction and negative extents are refused before any launch, for every op; M == 0 or N == 0 is a no-op
  for (int op = MATCHA_GEMM_NT; op <= MATCHA_GEMM_TN; ++op) {
    CHECK(matcha_gemm(op, logits, logits, logits, 8, 8, 0, nullptr, nullptr, nullptr, ws, need, nullptr) == MATCHA_EINVAL);
    CHECK(strstr(matcha_last_error(), "contraction") != nullptr);
    CHECK(matcha_gemm(op, logits, logits, logits, 8, 8, -3, nullptr, nullptr, nullptr, ws, need, nullptr) == MATCHA_EINVAL);
    CHECK(matcha_gemm(op, logits, logits, logits, -1, 8, 8, nullptr, nullptr, nullptr, ws, need, nullptr) == MATCHA_EINVAL);
    CHECK(matcha_gemm(op, logits, logits, logits, 8, -1, 8, nullptr, nullptr, nullptr, ws, need, nullptr) == MATCHA_EINVAL);
    CHECK(matcha_gemm(op, logits, logits, logits, 0, 8, 8, nullptr, nullptr, nullptr, ws, need, nullptr) == MATCHA_OK);
    CHECK(matcha_gemm(op, logits, logits, logits, 8, 0, 8, nullptr, nullptr, nullptr, ws, need, nullptr) == MATCHA_OK);
    CHECK(matcha_gemm(op, logits, logits, logits, 0, 0, 0, nullptr, nullptr, nullptr, ws, need, nullptr) == MATCHA_EINVAL);
  }
  CHECK(matcha_gemm(MATCHA_GEMM_NT, nullptr, logits, logits, 8, 8, 8, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == MATCHA_EINVAL);
  CHECK(matcha_embed_fwd(nullptr, 8, 64, nullptr, nullptr, nullptr, 24, nullptr, nullptr, nullptr, nullptr) == MATCHA_EINVAL);
  CHECK(matcha_quantile_uniform(nullptr, 10, 1000, nullptr, nullptr, nullptr, 0, nullptr) != MATCHA_OK);
  CHECK(matcha_zscore_rows(nullptr, 4, 4, nullptr) != MATCHA_OK);
  // a valid call up to the first launch: without a device the launch fails and is REPORTED, not ignored
  if (matcha_device_count() == 0) {
    int32_t status[4] = {0, 0, 0, 0};
    const int rc = matcha_ragged_plan(x, 8, 3, 100, status, ws, need, &view, nullptr);
    CHECK(rc == MATCHA_EHIP);
    CHECK((const char*)view.row_off >= ws && (const char*)view.tile_meta < ws + need);
  }
  free(raw);
}

static void check_options() {
  CHECK(matcha_get_option("disable_fused") == 0 && matcha_get_option("no_such_option") == -1 && matcha_get_option(nullptr) == -1);
  CHECK(matcha_set_option("no_such_option", 1) == MATCHA_EINVAL && matcha_set_option(nullptr, 1) == MATCHA_EINVAL);
  CHECK(matcha_set_option("disable_merged", 1) == MATCHA_OK && matcha_get_option("disable_merged") == 1);
  CHECK(matcha_set_option("disable_merged", 0) == MATCHA_OK && matcha_get_option("disable_merged") == 0);
  // MATCHA_FUSED_DBG=3 was exported by the test before this process started: the environment is read once, at first use
  CHECK(matcha_get_option("fused_dbg") == 3);
  matcha_shape s = shape(64, 24, 3067, 0, 0, 0);
  const size_t a = matcha_workspace_bytes_forward(&s, 1024, 5);
  matcha_set_option("disable_fused", 1);
  const size_t b = matcha_workspace_bytes_forward(&s, 1024, 5);
  matcha_set_option("disable_fused", 0);
  CHECK(a < b && b == matcha_workspace_bytes(&s, 1024, 5));          // the compact layout exists only with the fused kernels
}

// ---- the step's kernel route (model.hip: StepRoute, decide_route, the per-workspace record): decided without a device, so checked here ----
static void check_routes() {
  const int dbg = matcha_get_option("fused_dbg");
  matcha_set_option("fused_dbg", 0);                  // (bit 0 keeps the whole tail in the forward kernel: no split tail to check)
  CHECK(device_cu_count() == 256 || matcha_device_count() > 0);      // without a device the small-batch bound is 512 half tiles
  // implications, over shapes x front ends x per-call options x every switch
  const Fields names = route_field_names();
  const int n_fields = (int)names.size();
  std::vector<int> seen(n_fields, 0);
  for (int sw = 0; sw < kNumRouteSwitches; ++sw) {
    set_route_switch(sw, true);
    for (int d : {16, 64, 128, 256})
      for (int mode = 0; mode < 2; ++mode)
        for (int64_t B : {2ll, 1024ll, 8192ll, 65536ll})
          for (int bits = 0; bits < 32; ++bits) {
            const matcha_shape s = mode ? shape(d, 24, 3068, 23, 1, 250) : shape(d, 24, 3068, 0, 0, 0);
            matcha_step_opts o = train_opts();
            o.forward_only = bits & 1; o.deterministic = (bits >> 1) & 1; o.loss_in_forward = (bits >> 2) & 1;
            const bool targets = (bits >> 3) & 1, force = (bits >> 4) & 1;
            const StepRoute r = route_of(s, o, B, 5, targets, force);
            CHECK(!r.node_v || r.node_r);
            CHECK(!r.node_r || r.node);
            CHECK(!r.node || (r.fused && r.front && !r.small && !o.deterministic && !o.sparse_table_grad && mode == 0));
            CHECK(!r.split_tail || r.lif);
            CHECK(!r.lif || (r.fused && targets && o.loss_in_forward));
            CHECK(!r.dx_zeroed || (r.lif && !o.deterministic));
            CHECK(!r.enc128 || (!r.fused && d == 128 && r.merged_layerwise));
            CHECK(!r.fused || d == 64);
            CHECK(!r.front || r.fused);
            CHECK(!r.adj_fused || (r.front && mode == 1));
            CHECK(!r.small || r.fused);
            CHECK(!r.compact || (r.fused && o.forward_only));
            CHECK(!o.forward_only || (!r.node_v && !r.lif));
            CHECK(!force || (!r.fused && !r.enc128 && !r.node && !r.compact));
            CHECK(!r.long_rows);                        // decide_route never sets it: the long training forward notes its own record
            int i = 0;
            if (!sw) for_each_route_field(r, [&](const char*, const auto& v) { seen[i++] += v != 0; });
          }
    set_route_switch(sw, false);
  }
  // the default sweep reaches every field decide_route can set -- all but long_rows: none of the implications is vacuous
  for (int i = 0; i < n_fields; ++i) CHECK((seen[i] > 0) == (names[i] != "long_rows"));

  // the table front end at hg38 1 Mb (3 068 nodes), k <= 5, a training step with targets: the node route from 8 192 rows, its value table at 65 536
  const matcha_shape t64 = shape(64, 24, 3068, 0, 0, 0);
  const matcha_step_opts o = train_opts();
  for (int64_t B : {8192ll, 16384ll, 32768ll, 65536ll}) {
    const StepRoute r = route_of(t64, o, B, 5, true);
    CHECK(r.fused && r.front && !r.small && r.node && r.node_r && r.node_v == (B == 65536));
    CHECK(r.lif && r.split_tail && r.dx_zeroed && !r.compact && r.half_plan && !r.adj_fused && !r.enc128 && !r.merged_layerwise);
  }
  const StepRoute small = route_of(t64, o, 1024, 5, true);
  CHECK(small.fused && small.front && small.small && !small.node && !small.node_r && !small.node_v && small.lif && !small.split_tail && small.dx_zeroed);
  // each switch of the node route takes out its own field and the fields that depend on it, nothing else.  From decide_route: node_r needs node and
  // node_v needs node_r; fwd_values names the table only with node_v and the per-node product only with node_r; node_dx needs node_v.  Every other
  // field reads none of these
  const StepRoute base = route_of(t64, o, 65536, 5, true);
  CHECK(base.fwd_values == kValuesTable && base.node_dx && base.paired);
  const char* node_sw[] = {"disable_node_v", "disable_node_r", "disable_node_front"};
  const Fields node_diff[] = {{"node_v", "fwd_values", "node_dx"}, {"node_r", "node_v", "fwd_values", "node_dx"}, {"node", "node_r", "node_v", "fwd_values", "node_dx"}};
  for (int i = 0; i < 3; ++i) {
    matcha_set_option(node_sw[i], 1);
    const StepRoute r = route_of(t64, o, 65536, 5, true);
    matcha_set_option(node_sw[i], 0);
    CHECK(route_diff(base, r) == node_diff[i]);
    CHECK(r.fwd_values == (i == 0 ? kValuesNodeProduct : kValuesToken));
  }
  for (const char* sw : {"disable_node_dx", "disable_launch_pairs"}) {      // the two switches without dependants: their own field alone
    matcha_set_option(sw, 1);
    const StepRoute r = route_of(t64, o, 65536, 5, true);
    matcha_set_option(sw, 0);
    CHECK(route_diff(base, r) == Fields{!strcmp(sw, "disable_node_dx") ? "node_dx" : "paired"});
  }
  {
    matcha_set_option("disable_small_batch", 1);
    const StepRoute r = route_of(t64, o, 1024, 5, true);
    matcha_set_option("disable_small_batch", 0);
    CHECK(!r.small && r.split_tail && r.dx_zeroed && !r.node);            // 5 121 token rows: below the node route's size rule
  }
  CHECK(route_diff(base, route_of(t64, o, 65536, 5, true)).empty());     // every switch restored

  // the record: field for field, dropped by forget_forward, the 4 096 most recent workspaces kept
  g_fwd_state.clear();
  const StepRoute zero = {};
  auto pattern = [&](int i) {      // every field from the bits of a hash of i: a flag from bit j, a number (fwd_values) as 1..3 where its bit is set
    StepRoute r = zero;
    const uint32_t h = (uint32_t)i * 2654435761u;
    for (int j = 0; j < n_fields; ++j) set_route_field(r, j, ((h >> j) & 1) ? 1 + (int)((h >> 28) % 3) : 0);
    return r;
  };
  auto ws_ptr = [](int i) { return reinterpret_cast<const void*>((uintptr_t)(i + 1) << 12); };
  StepRoute got;
  CHECK(!recorded_route(ws_ptr(0), got));
  for (int j = 0; j < n_fields; ++j)                  // one field set at a time, a number at each of its values (1..3: kValuesToken .. kValuesTable)
    for (int v = 1; v <= 3; ++v) {
      StepRoute one = zero;
      set_route_field(one, j, v);
      CHECK(route_diff(one, zero) == Fields{names[j]});
      note_forward(ws_ptr(0), one);
      CHECK(recorded_route(ws_ptr(0), got) && route_diff(got, one).empty() && g_fwd_state.size() == 1);
    }
  forget_forward(ws_ptr(0));
  CHECK(!recorded_route(ws_ptr(0), got) && g_fwd_state.empty());
  std::vector<int> ones(n_fields, 0);
  for (int i = 0; i < 4097; ++i) {
    const StepRoute r = pattern(i);
    note_forward(ws_ptr(i), r);
    int j = 0;
    for_each_route_field(r, [&](const char*, const auto& v) { ones[j++] += v != 0; });
  }
  for (int j = 0; j < n_fields; ++j) CHECK(ones[j] > 1024 && ones[j] < 3072);      // the pattern sets and clears every field, about half the time each
  CHECK(g_fwd_state.size() == 4096 && !recorded_route(ws_ptr(0), got));
  int kept = 0;
  for (int i = 1; i < 4097; ++i) kept += recorded_route(ws_ptr(i), got) && route_diff(got, pattern(i)).empty();
  CHECK(kept == 4096);
  CHECK(!route_diff(pattern(1), pattern(7)).empty());
  note_forward(ws_ptr(1), pattern(7));               // a pointer already on record is refreshed, nothing evicted
  CHECK(g_fwd_state.size() == 4096 && recorded_route(ws_ptr(2), got) && recorded_route(ws_ptr(1), got) && route_diff(got, pattern(7)).empty());
  g_fwd_state.clear();
  matcha_set_option("fused_dbg", dbg);
}

// matcha_route_read: the record as text, the only reader of it outside the library (matcha_amd/_lib.py: route_record).  The text below is the
// entry's output format, written out: "name value\n" per field in the struct's order, here with every value 0.
static void check_route_read() {
  static const char kZeroText[] =
      "compact 0\nhalf_plan 0\nfused 0\nmerged_layerwise 0\nenc128 0\nfront 0\nadj_fused 0\nsmall 0\nlif 0\nsplit_tail 0\ndx_zeroed 0\n"
      "node 0\nnode_r 0\nnode_v 0\nfwd_values 0\nnode_dx 0\npaired 0\nlong_rows 0\n";
  const size_t len = strlen(kZeroText);
  const void* const ws = reinterpret_cast<const void*>((uintptr_t)1 << 12);
  const StepRoute zero = {};
  std::vector<char> buf(len + 1);                     // exactly what the text takes: ASan traps a write past it
  g_fwd_state.clear();
  note_forward(ws, zero);
  CHECK(matcha_route_read(ws, buf.data(), buf.size()) == MATCHA_OK && !strcmp(buf.data(), kZeroText));
  // each field set alone -- fwd_values at each of its three constants -- changes the digit of its own line and nothing else
  int j = 0;
  for (const char* line = kZeroText; *line; line = strchr(line, '\n') + 1, ++j) {
    const bool number = !strncmp(line, "fwd_values ", 11);
    for (int v : {kValuesToken, kValuesNodeProduct, kValuesTable}) {
      if (!number && v != 1) continue;
      std::string want(kZeroText);
      want[(size_t)(strchr(line, '\n') - kZeroText) - 1] = (char)('0' + v);
      StepRoute one = zero;
      set_route_field(one, j, v);
      note_forward(ws, one);
      CHECK(matcha_route_read(ws, buf.data(), buf.size()) == MATCHA_OK && want == buf.data());
    }
  }
  CHECK(j == (int)route_field_names().size());
  // one byte short: MATCHA_ENOMEM with a message, nothing written past the buffer
  std::vector<char> tight(len);
  CHECK(matcha_route_read(ws, tight.data(), tight.size()) == MATCHA_ENOMEM && strstr(matcha_last_error(), "buffer too small") != nullptr);
  // refused: null pointers, an empty buffer, a workspace with no forward on record
  CHECK(refused(matcha_route_read(nullptr, buf.data(), buf.size()), "matcha_route_read: null pointer"));
  CHECK(refused(matcha_route_read(ws, nullptr, buf.size()), "matcha_route_read: null pointer"));
  CHECK(refused(matcha_route_read(ws, buf.data(), 0), "matcha_route_read: null pointer"));
  forget_forward(ws);
  CHECK(refused(matcha_route_read(ws, buf.data(), buf.size()), "matcha_route_read: no forward on record for this workspace"));
  CHECK(g_fwd_state.empty());
}

static void fuzz_plan_oracle() {
  std::mt19937_64 rng(7);
  for (int it = 0; it < 300; ++it) {
    const int L = 1 + (int)(rng() % 8);
    const int64_t B = 1 + (int64_t)(rng() % (it < 250 ? 300 : 20000));
    const int64_t T = B * L, N = 50;
    std::vector<int64_t> x(T);
    const int style = (int)(rng() % 4);
    for (int64_t i = 0; i < T; ++i) {
      const uint64_t r = rng();
      x[i] = (style == 0) ? (int64_t)(r % (N + 1)) : (style == 1 ? (int64_t)(1 + r % N) : (style == 2 ? ((r & 7) ? 0 : (int64_t)(1 + r % N)) : (int64_t)(r % (N + 3)) - 1));
    }
    const int64_t cap = (T + 1 + (64 - L) - 1) / (64 - L) + (T + 1 + 63 * 32 - 1) / (63 * 32) + 2;        // ragged.hip: tiles_cap
    std::vector<int32_t> row_off(B + 1), slot(T + 1), key(T + 1), pos(T + 1), meta(cap * 4);
    std::vector<int64_t> id(T + 1);
    int32_t count[3], status = 0;
    const int64_t nt = matcha_oracle_ragged_plan(x.data(), B, L, N, row_off.data(), slot.data(), id.data(), key.data(), pos.data(), count, meta.data(), cap, &status);
    CHECK(nt >= 1 && nt <= cap && count[2] == nt);
    const int64_t Tr = count[1];
    CHECK(count[0] == Tr + 1 && row_off[B] == Tr && slot[Tr] == T && id[Tr] == 0);
    int64_t real = 0;
    bool bad = false;
    for (int64_t i = 0; i < T; ++i) { real += x[i] != 0; bad |= (x[i] < 0 || x[i] > N); }
    CHECK(real == Tr && (status != 0) == bad);
    int64_t tok = 0, hy = 0;
    for (int64_t t = 0; t < nt; ++t) {
      CHECK(meta[4 * t] == tok && meta[4 * t + 2] == hy && meta[4 * t + 1] <= 63 && meta[4 * t + 3] >= 1);
      CHECK(row_off[meta[4 * t + 2]] == meta[4 * t] && row_off[meta[4 * t + 2] + meta[4 * t + 3]] == meta[4 * t] + meta[4 * t + 1]);
      tok += meta[4 * t + 1]; hy += meta[4 * t + 3];
    }
    CHECK(tok == Tr && hy == B);
    for (int64_t t = 0; t < Tr; ++t) {
      const int64_t b = slot[t] / L;
      CHECK(t >= row_off[b] && t < row_off[b + 1] && (pos[t] & 255) == t - row_off[b] && (pos[t] >> 8) == row_off[b + 1] - row_off[b]);
      CHECK(key[t] == (int32_t)id[t] && (id[t] == x[slot[t]] || (id[t] == 0 && (x[slot[t]] < 0 || x[slot[t]] > N))));
    }
    for (int64_t t = Tr; t <= T; ++t) CHECK(key[t] == 0);
    // half tiles (<= 31 tokens: one wavefront of the fused forward) + the token -> (tile, row) map
    const int64_t hcap = (T + 1 + (32 - L) - 1) / (32 - L) + (T + 1 + 63 * 32 - 1) / (63 * 32) + 2;       // ragged.hip: halves_cap
    std::vector<int32_t> half(hcap * 4), tt(T + 1, -1);
    const int64_t nh = matcha_oracle_ragged_halves(row_off.data(), B, meta.data(), nt, half.data(), hcap, tt.data());
    CHECK(nh >= nt && nh <= hcap);
    tok = 0; hy = 0;
    for (int64_t t = 0; t < nh; ++t) {
      CHECK(half[4 * t] == tok && half[4 * t + 2] == hy && half[4 * t + 1] <= 31 && half[4 * t + 3] >= 1);
      CHECK(row_off[half[4 * t + 2] + half[4 * t + 3]] == half[4 * t] + half[4 * t + 1]);
      tok += half[4 * t + 1]; hy += half[4 * t + 3];
    }
    CHECK(tok == Tr && hy == B);
    for (int64_t t = 0; t < Tr; ++t) {
      const int64_t w = tt[t] >> 6, row = tt[t] & 63;
      CHECK(tt[t] >= 0 && w < nt && meta[4 * w] + row == t && row < meta[4 * w + 1]);
    }
  }
}

int main() {
  check_options();                      // first: the option table must see the environment of the process start
  check_sizes_and_validation();
  check_entry_point_errors();
  check_routes();
  check_route_read();
  fuzz_plan_oracle();
  printf("device_count=%d\n", matcha_device_count());
  return finish("HOST CHECKS");
}
