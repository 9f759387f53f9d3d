"""Every kernel route of the training step held to fp32 grade against the fp64 oracle (tests/fp64_grade.py): one dropout-free
Trainer.forward_backward step and the eval-mode model(x) of each case, every output within K = 8 times the fp32 oracle's own noise.
The ``_drop`` / ``_highp`` / ``saturated_pff`` cases run the same step with dropout ON -- what the benchmark and every published number run --
against the oracle with the kernels' own masks injected (oracle/rng.py, G.step_masks): the masks' regeneration in the backward's epilogues,
the tanh recovered from the stored post-dropout H1, gemm_wide's and the layer-by-layer kernels' dropout epilogues are dead code at p = 0.
The parity tests elsewhere allow 1e-4 (the north star); a kernel that silently loses a factor of 20 -- a dropped bf16 plane product,
a tanh that is only accurate in absolute terms -- passes them and fails here.  Each case also asserts its kernel set (a size rule that
moves a case onto other kernels fails it) and that its bound is tight enough to reject the three-product witness.

The d = 64 table front end has three routes (model.hip: node_front_shape, the options disable_node_r / disable_node_front), and every case
NAMES the one it runs (``Case.table``): the option it runs under and the node kernels it must / must not launch are derived from that name, for
every case of the table.  Every graded condition of the large-batch table step -- default weights, the four stresses, the regression
objective, L = 8, the separate tail, the first size past the small-batch kernels -- runs on all three routes from one batch and one set of
references, and the size rule is crossed by size alone at wide_adj (3 300 / 3 400 rows).  GPU only (-m gpu).
"""
import contextlib
from dataclasses import dataclass, field, replace
from typing import Dict, FrozenSet, Optional, Tuple

import numpy as np
import pytest
import torch

from matcha_amd import synth, _lib
from tests import fp64_grade as G
from tests.helpers import oracle_state
from tests.test_cpu_long_grid import DIM_CASES
from tests.test_hip_model import hip_model, _trainer_grads

pytestmark = pytest.mark.gpu

# kernel sets (matcha_launch_log): what each case must run and must not run, so that a size rule or a switch that moves a case onto other
# kernels fails it instead of quietly testing something else.  The sets of t16 / a32 and the sorted-gradient kernels were read off the
# first MI355X run and frozen.
_BIG64 = frozenset({"fused_fwd32_kernel", "tail_bwd64_kernel", "fused_bwdh_kernel", "fbm_reduce_kernel", "fbm_chain_kernel"})
_FRONT64 = frozenset({"front_fwd3_kernel", "front_bwd_kernel"})
_ADJ64 = frozenset({"adj_fused_fwd_kernel", "adj_recon_kernel", "adj_fused_bwd_kernel"})
_ENC128 = frozenset({"enc128_fwd_kernel", "enc128_bwd_kernel", "enc128_unfold_kernel", "head_fwd_kernel", "head_bwd_kernel"})
_WIDE = frozenset({"gemm_wide_kernel", "gemm_tn_wide_kernel", "attn_fwd_wide_kernel", "attn_bwd_wide_kernel"})
_LAYERWISE = frozenset({"attn_fwd_kernel", "attn_bwd_kernel", "ln3_fwd_kernel", "ln3_bwd_kernel", "head_fwd_kernel", "head_bwd_kernel",
                        "gemm_lds_kernel", "gemm_tn_kernel", "embed_fwd_kernel", "embed_scatter_kernel"})
_SORTED_TABLE = frozenset({"tg_hist_kernel", "tg_idscan_kernel", "tg_place_kernel", "tg_runsum_kernel", "tg_colscan_kernel"})
_SMALL = frozenset({"fused_fwd32h_kernel", "plan_small_kernel"})
_NOT_FUSED = frozenset({"fused_fwd32_kernel", "fused_fwd32h_kernel", "fused_bwdh_kernel", "enc128_fwd_kernel", "attn_fwd_wide_kernel"})
# the table front end's route (Case.table): the node kernels that must / must not run, and the option that switches a node-shaped case there
_NODE = frozenset({"node_scatter_kernel", "node_xhat_kernel", "node_r_kernel"})
_TABLE_SETS = {"node_r": (_NODE, frozenset()), "node_rec": (_NODE - {"node_r_kernel"}, frozenset({"node_r_kernel"})),
               "token": (frozenset(), _NODE), "": (frozenset(), _NODE)}
_TABLE_OPTION = {"node_rec": "disable_node_r", "token": "disable_node_front"}


@dataclass(frozen=True)
class Case:
    layout: str
    d: int
    mode: str
    seed: int                              # weights (and the adj features)
    ks: Tuple[int, ...] = (2, 3, 4, 5)
    rows_per_k: int = 1024
    L: int = 0
    rows: object = None                    # None = the whole batch; an int, or "edge-" / "edge+" (size rule, resolved on the device)
    batch_seed: int = 0                    # 0: seed + 500
    route: str = ""                        # "det" | "nolif" | "fourprod" | "layerwise"
    objective: str = "class"
    stress: str = ""                       # "small" | "sharp" | "saturated" | "hot" | "saturated_pff"
    drop: Optional[Tuple[float, float, float]] = None      # (p_adj, p_fc1, p_pff): the step runs with dropout ON; None: every Dropout.p = 0
    drop_seed: int = 0                     # the step's dropout seed (Trainer base_seed = drop_seed - 1); 0: seed + 700
    # route of the d = 64 table front end: "node_r" (per node, r table) | "node_rec" (per node, r rows in the record: disable_node_r) | "token"
    # (per token: disable_node_front, or with by_size a batch below the size rule and NO option); "": a case the rule cannot reach
    table: str = ""
    by_size: bool = False
    must: FrozenSet[str] = frozenset()
    must_not: FrozenSet[str] = frozenset()
    k_of: Dict[str, float] = field(default_factory=dict, hash=False, compare=False)


T64 = Case("hg38_1mb", 64, "table", 81, table="node_r", must=_BIG64 | _FRONT64,
           must_not=_SMALL | _SORTED_TABLE | {"embed_fwd_kernel", "front_fwd_kernel", "head_bwd_kernel", "attn_fwd_kernel"})
A64 = Case("hg38_1mb", 64, "adj", 82, must=_BIG64 | _ADJ64, must_not=_SMALL | {"adj_encode_fwd_kernel", "front_fwd3_kernel", "attn_fwd_kernel"})
T128 = Case("c1", 128, "table", 83, ks=(2, 3, 4, 5, 6, 7, 8), rows_per_k=585, must=_ENC128,
            must_not={"attn_fwd_wide_kernel", "attn_bwd_wide_kernel", "attn_fwd_kernel", "attn_bwd_kernel"})
_TINY = dict(batch_seed=1009, table="", must=_SMALL | _FRONT64 | {"fused_bwdh_kernel"}, must_not={"fused_fwd32_kernel", "tail_bwd64_kernel"})

CASES = {
    "t64_big": T64,
    "t64_det": replace(T64, route="det", table="", must=T64.must | _SORTED_TABLE, must_not=T64.must_not - _SORTED_TABLE),
    "t64_nolif": replace(T64, route="nolif", must=(T64.must - {"tail_bwd64_kernel"}) | {"head_bwd_kernel"},
                         must_not=(T64.must_not - {"head_bwd_kernel"}) | {"tail_bwd64_kernel"}),
    # at embed_dim 64 both switches land on the layer-by-layer kernels with the reference's four products per head
    "t64_fourprod": replace(T64, route="fourprod", table="", must=_LAYERWISE, must_not=_BIG64 | _FRONT64 | _SMALL),
    "t64_layerwise": replace(T64, route="layerwise", table="", must=_LAYERWISE, must_not=_BIG64 | _FRONT64 | _SMALL),
    # the last batch size whose half tiles fit two per CU (the one-workgroup-per-half forward; the plan there is already the multi-launch
    # one) and the first that does not
    "t64_edge-": replace(T64, rows="edge-", table="", must={"fused_fwd32h_kernel", "fused_bwdh_kernel"} | _FRONT64, must_not={"fused_fwd32_kernel", "tail_bwd64_kernel"}),
    "t64_edge+": replace(T64, rows="edge+"),
    # (a batch whose first rows let the witness show: at one to three rows its logit error is a matter of the rows drawn)
    "t64_tiny1": replace(T64, rows=1, **_TINY),
    "t64_tiny2": replace(T64, rows=2, **_TINY),
    "t64_tiny3": replace(T64, rows=3, **_TINY),
    "t64_k8": Case("c23", 64, "table", 84, ks=(2, 3, 4, 5, 6, 7, 8), rows_per_k=585, L=8, table="node_r", must=T64.must, must_not=T64.must_not),
    "t64_nattr5": Case("c1", 64, "table", 85, rows_per_k=512, must={"embed_fwd_kernel", "embed_scatter_kernel", "fused_fwd32h_kernel",
                                                                     "fused_bwdh_kernel", "lnhat_bwd_kernel"}, must_not=_FRONT64),
    "a64_hg38": A64,
    "a64_wide": replace(A64, layout="wide_adj", seed=86),
    "t128": T128,
    "a128_wide": Case("wide_adj", 128, "adj", 87, ks=(2, 3, 4, 5, 6, 7, 8), rows_per_k=585,
                      must=_ENC128 | {"adj_encode_fwd_kernel", "adj_tn_kernel<1>"}, must_not=T128.must_not | _ADJ64),
    "t256": Case("c1", 256, "table", 88, ks=(2, 3, 4, 5, 6, 7, 8), rows_per_k=286, must=_WIDE, must_not={"enc128_fwd_kernel", "enc128_bwd_kernel", "fused_fwd32_kernel"}),
    "t16": Case("tiny", 16, "table", 89, rows_per_k=64, must=_LAYERWISE | {"plan_small_kernel"}, must_not=_NOT_FUSED),
    "a32": Case("tiny", 32, "adj", 90, rows_per_k=64, must=(_LAYERWISE - {"embed_scatter_kernel"}) | {"plan_small_kernel", "adj_encode_fwd_kernel",
                "adj_sort_small_kernel", "adj_tn_kernel<0>", "adj_tn_kernel<1>"}, must_not=_NOT_FUSED | _ADJ64),
    # pff_classifier's bias gradient is ONE number, the sum of 4 096 dlogits 2 (softplus(z) - y) softplus'(z) / B that cancel 40 : 1, so its
    # e is a single draw of the logits' propagated rounding noise and so is the fp32 noise it is divided by (measured ratio 7.6): K 16
    "r64": replace(T64, objective="regress", k_of={"pff_classifier.PWF_Conv0.bias": 16.0}),
}
for _base in ("t64_big", "a64_hg38", "t128"):
    for _s in ("small", "sharp", "saturated", "hot"):
        _c = CASES[_base]
        CASES[f"{_base}_{_s}"] = replace(_c, stress=_s, rows_per_k=3 * _c.rows_per_k if _s == "hot" else _c.rows_per_k)
CASES["t128_hot"] = replace(CASES["t128_hot"], batch_seed=1101)          # (the default batch leaves the witness only 2.0x out)
CASES["t64_big_hot_det"] = replace(CASES["t64_big_hot"], route="det", table="", must=CASES["t64_det"].must, must_not=CASES["t64_det"].must_not)
# Every graded condition of the large-batch table step on the two other routes as well: same weights, batch and references (_data drops
# ``table``), only the option differs.  At these sizes the rule picks the node route (20 481 >= 12 272 at hg38_1mb's 4 096 rows), so without
# the counterparts the per-token kernels -- what every table with 4 (N + 1) > B L + 1 runs: front_bwd_kernel's float atomics into the table, > 10^4
# addends into one row in `hot` -- and the node route's r-in-the-record backward would be graded at c23 with default weights only.
TABLE_BASES = ("t64_big", "t64_big_small", "t64_big_sharp", "t64_big_saturated", "t64_big_hot", "r64", "t64_k8", "t64_nolif", "t64_edge+")
for _base in TABLE_BASES:
    assert CASES[_base].table == "node_r", _base
    for _t in ("token", "node_rec"):
        CASES[f"{_base}_{_t}"] = replace(CASES[_base], table=_t)
# Both sides of the size rule reached by SIZE, no option set: wide_adj as a table layout has N + 1 = 4 157 rows, 4 (N + 1) = 16 628; 3 300 rows
# (capacity 16 501) stay per token -- the one graded per-token workspace carved WITHOUT the node tables --, 3 400 rows (17 001) take the node route
# (tests/test_hip_node_front.py::test_size_rule_and_exclusions).  n_attr is 8 there.
CASES["t64_wide_below"] = replace(T64, layout="wide_adj", seed=91, rows_per_k=825, table="token", by_size=True)
CASES["t64_wide_above"] = replace(T64, layout="wide_adj", seed=91, rows_per_k=850, table="node_r")

# The embed dims check_shape_fields accepts beside 16, 32, 64, 128 and 256 (tests/test_cpu_long_grid.py::DIM_CASES), on the L <= 8 step: below 64 the
# layer-by-layer kernels (attention's `fon` clamp at a partial last 32-feature tile, GEMMs at K = d no multiple of 16), at 192 the wide kernels (three
# 64-feature chunks, a 3 x 3 bmm_heads grid, gemm_wide at N = 1 536, K = 192).  rows_per_k as t16 / a32 (64) and t256 (286): the smallest that reach
# those routes.  Below 64: _LAYERWISE and nothing of _NOT_FUSED.  At 192: _WIDE without gemm_tn_wide_kernel -- its tiles are 128 x 128 and
# gemm_tn_wide_eligible wants M and N multiples of 128, which neither 192 nor 1 536 x 192 is, so every weight gradient takes gemm_tn_kernel, and the
# products with N = 192 take gemm_lds_kernel -- and neither enc128_* nor fused_fwd32_kernel.  What goes beyond that was read off the first MI355X run
# and frozen: the adj front end's kernels (the small sort at 256 / 448 rows, the histogram sort at 2 002), bmm_heads_kernel and the row plan at 192.
_C1_KS = (2, 3, 4, 5, 6, 7, 8)
_ADJ_FRONT = frozenset({"adj_encode_fwd_kernel", "adj_tn_kernel<0>", "adj_tn_kernel<1>", "adj_tanh_gather_kernel", "adj_recon_loss_kernel"})
for _layout, _d, _mode, _seed in DIM_CASES:
    _ks = dict(ks=_C1_KS) if _layout == "c1" else {}
    if _d < 64:
        _must = _LAYERWISE | {"plan_small_kernel"}
        _must = _must if _mode == "table" else (_must - {"embed_scatter_kernel"}) | _ADJ_FRONT | {"adj_sort_small_kernel"}
        _sets = dict(must=_must, must_not=_NOT_FUSED | _ADJ64 | {"gemm_wide_kernel", "gemm_tn_wide_kernel"})
    else:
        _must = (_WIDE - {"gemm_tn_wide_kernel"}) | {"gemm_tn_kernel", "gemm_lds_kernel", "bmm_heads_kernel", "head_sum_row_kernel", "row_fill_kernel"}
        _must = _must | {"embed_scatter_kernel"} if _mode == "table" else _must | _ADJ_FRONT | {"adj_hist_kernel", "adj_scan_kernel", "adj_scatter_kernel"}
        _sets = dict(must=_must, must_not=frozenset({"enc128_fwd_kernel", "enc128_bwd_kernel", "fused_fwd32_kernel", "fused_fwd32h_kernel",
                                                     "attn_fwd_kernel", "plan_small_kernel"}) | _ADJ64)
    CASES[f"{_mode[0]}{_d}"] = Case(_layout, _d, _mode, _seed, rows_per_k=64 if _d < 64 else 286, **_ks, **_sets)

# ---- dropout ON -----------------------------------------------------------------------------------------------------------------------------
# Twins of the cases above at the model's default p (same shapes: already the smallest that reach each kernel set), the kernel sets, the table
# route and the witness assertion unchanged.  The high-p twins take p that no float represents, the widest gap between floor(p 2^32) of the double
# and of the float (oracle/rng.py) and (1 / (1 - p)) (1 - p) furthest from 1.
P_DEFAULT, P_HIGH = (0.2, 0.3, 0.4), (0.6, 0.7, 0.9)
DROP_BASES = ("t64_big", "t64_big_token", "t64_big_node_rec", "t64_det", "t64_nolif", "t64_fourprod", "t64_layerwise", "t64_edge-", "t64_edge+",
              "t64_tiny2", "t64_k8", "t64_nattr5", "t64_wide_below", "a64_hg38", "a64_wide", "t128", "a128_wide", "t256", "t16", "a32", "r64",
              "a40", "t192")
for _base in DROP_BASES:
    CASES[f"{_base}_drop"] = replace(CASES[_base], drop=P_DEFAULT)
for _base in ("t64_big", "a64_hg38", "t128"):
    CASES[f"{_base}_highp"] = replace(CASES[_base], drop=P_HIGH)
# pff_n1's first layer saturated (G.saturated_pff): tail_bwd64_kernel (t64_big) and the in-kernel tail's own copy of that code
# (fused_fwd32_tail.hpp: t64_nolif, t64_edge-) compute 1 - t^2 from t = H1 (1 - p_pff), H1 stored AFTER the dropout, where 1 - t^2 is ~1e-3
for _base in ("t64_big", "t64_nolif", "t64_edge-"):
    CASES[f"{_base}_saturated_pff_drop"] = replace(CASES[_base], stress="saturated_pff", drop=P_DEFAULT)
CASES["t64_big_saturated_pff"] = replace(CASES["t64_big"], stress="saturated_pff")              # the control: the same stress, dropout-free


def _drop_ps(c: Case):
    """(p_adj, p_fc1, p_pff) as Classifier._dropout_p() must report them for the case (the table front end has no adj dropout)."""
    return (c.drop[0] if c.mode == "adj" else 0.0, c.drop[1], c.drop[2])


RESULTS = {}


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    yield
    if RESULTS:
        print("\nfp32 grade: worst e(HIP) / noise per case (step: logits, losses, every gradient; eval: model(x) logits)")
        for name, (step, ev, wit) in RESULTS.items():
            print(f"  {name:26s} step {step:5.2f}   eval {ev:5.2f}   witness {wit:6.1f} x bound")


_DATA = {}


def _data(c: Case):
    """(sd, fe, x, y, w, chrom, references, three-product witness, the eval logits' references) of a case; cached, several routes share
    one batch.  With ``drop`` the step's references and the witness get the step's masks, the eval references stay mask-free."""
    key = replace(c, route="", table="", by_size=False, must=frozenset(), must_not=frozenset())
    if key in _DATA:
        return _DATA[key]
    num = synth.LAYOUTS[c.layout]
    _, fe, sd = oracle_state(num, c.d, c.mode, c.seed)
    x, y, w = G.make_case_batch(c.layout, list(c.ks), c.rows_per_k, c.batch_seed or c.seed + 500, c.L)
    if c.rows is not None:
        n = G.edge_rows(c.rows, x.shape[1]) if isinstance(c.rows, str) else c.rows
        assert n <= len(x)
        x, y, w = x[:n], y[:n], w[:n]
    chrom = int(np.random.default_rng(c.seed).integers(fe.n_chrom))
    if c.stress == "small":
        sd = G.small_amplitude(sd)
    elif c.stress == "sharp":
        sd = G.sharp_attention(sd)
    elif c.stress == "saturated":
        sd = G.saturated_logits(sd, fe, x, chrom)
        w = w.copy()
        w[::5] = 0.0
    elif c.stress == "saturated_pff":
        sd = G.saturated_pff(sd, fe, x, chrom)
    elif c.stress == "hot":
        x = G.hot_node(x, 0.85)                             # 85 % of 12 285 - 12 288 rows: > 10^4 addends into one table row
    if c.objective == "regress":
        y = np.where(y > 0, w, 0.0).astype(np.float32)       # positive rows carry a target in [0.5, 4), negatives 0
        w = None
    masks, ref_eval = None, None
    if c.drop is not None:
        masks = G.step_masks(c.drop_seed or c.seed + 700, _drop_ps(c), x.size, c.d, num if c.mode == "adj" else None)
        ref_eval = G.references(sd, fe, x, y, w, chrom=chrom, objective=c.objective, backward=False)      # eval mode draws no mask
    ref = G.references(sd, fe, x, y, w, chrom=chrom, objective=c.objective, masks=masks)
    wit = G.oracle_step(sd, fe, x, y, w, chrom=chrom, objective=c.objective, ops=G.THREE_PRODUCT, backward=False, masks=masks)
    _DATA[key] = (sd, fe, x, y, w, chrom, ref, wit, ref_eval or ref)
    return _DATA[key]


@pytest.mark.parametrize("name", list(CASES))
def test_step_and_eval_at_fp32_grade(name):
    from matcha_amd.engine import Trainer
    c = CASES[name]
    sd, fe, x, y, w, chrom, ref, wit, ref_eval = _data(c)
    clf, _ = hip_model(synth.LAYOUTS[c.layout], c.d, c.mode, c.seed, sd=sd)
    for m in clf.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    base_seed = 0
    if c.drop is not None:
        for m, p in zip((getattr(clf.node_embedding, "dropout", None), clf.encode1.mul_head_attn.dropout, clf.encode1.pff_n1.dropout), c.drop):
            if m is not None:
                m.p = p
        assert clf._dropout_p() == _drop_ps(c), (name, clf._dropout_p())       # the masks of _data are the model's own p
        base_seed = (c.drop_seed or c.seed + 700) - 1                          # the first step draws with base_seed + 1
    clf.train()
    switch = {"fourprod": "disable_merged", "layerwise": "disable_fused"}.get(c.route)
    # the table route: named by every case, reachable only by the fused d = 64 table step, switched by its option unless the size decides
    assert c.table in _TABLE_SETS and (not c.by_size or c.table == "token"), (name, c.table)
    assert not c.table or (c.d == 64 and c.mode == "table" and c.route in ("", "nolif")), (name, c.table)
    must_node, must_not_node = _TABLE_SETS[c.table]
    table_switch = None if c.by_size else _TABLE_OPTION.get(c.table)
    assert not (switch and table_switch)
    switch = switch or table_switch
    if c.layout == "wide_adj" and c.mode == "table":
        assert (len(x) * x.shape[1] + 1 >= 4 * (int(np.sum(synth.LAYOUTS[c.layout])) + 1)) == (c.table == "node_r"), (name, x.shape)
    with (_lib.option(switch) if switch else contextlib.nullcontext()):
        tr = Trainer(clf, lr=1e-3, deterministic=(c.route == "det"), objective=c.objective, base_seed=base_seed)
        if c.route == "nolif":
            tr.loss_in_forward = False
        xd = torch.from_numpy(x).cuda().contiguous()
        yd = torch.from_numpy(y).cuda().contiguous()
        wd = None if w is None else torch.from_numpy(w).cuda().contiguous()
        with _lib.launch_log() as log:
            logits = tr.forward_backward(xd, yd, wd, 1.0, 0.001, chrom)
            torch.cuda.synchronize()
        grads = {n: (None if v is None else v.cpu().double().numpy()) for n, v in _trainer_grads(tr, clf).items()}
        got = G.StepOut(logits.cpu().double().numpy(),
                        {G.main_loss_name(c.objective): float(tr.losses[0]), "recon": float(tr.losses[1])}, grads)
        clf.eval()
        with torch.no_grad():
            lg_eval = clf(xd).cpu().double().numpy()
    ran = {k for k, n in log.counts.items() if n > 0}
    print(f"{name}: B = {len(x)}, L = {x.shape[1]}, table route {c.table or '-'}, kernels {sorted(ran)}")
    ratio = G.assert_grade(f"{name} step", G.grade(got, ref, c.k_of))
    ratio_eval = G.assert_grade(f"{name} eval", G.logit_rows(lg_eval, ref_eval, c.k_of.get("logits", G.K)))
    # the bound must be tight enough to reject the three-product witness (its forward is enough)
    wit_over = max(r.err / (r.k * r.noise) for r in G.logit_rows(wit.logits, ref, c.k_of.get("logits", G.K)))
    RESULTS[name] = (ratio, ratio_eval, wit_over)
    assert wit_over >= 2.0, (name, wit_over)
    must, must_not = set(c.must) | must_node, set(c.must_not) | must_not_node
    assert must <= ran, (name, sorted(must - ran), sorted(ran))
    assert not (must_not & ran), (name, sorted(must_not & ran))
