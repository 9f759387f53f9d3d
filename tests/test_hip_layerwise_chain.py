"""The layer-by-layer token chain (matcha_amd/csrc/layerwise.hip) behind every entry point that runs it: rows of up to 8 columns
(matcha_forward / matcha_backward off the fused embed_dim-64 route, matcha_get_embedding) and rows of up to 32 (matcha_forward_long,
matcha_forward_long_train / matcha_backward_long).

1. Launches.  The chain was written out once per entry point before it became one set of functions; each case below records the
   {kernel: launches} of its calls and compares the whole dict with what the commit before that change (PARENT) launched on the same
   input -- no launch added, dropped or moved to another kernel.
2. The record.  One forward record per workspace pointer, shared by the short and the long pair: a forward of either kind replaces the
   other's record, and the backward of the replaced kind is refused before any launch.

The entry points are called directly (C ABI), as tests/test_hip_long_train.py::c_step does.  GPU only (-m gpu)."""
import ctypes as C

import numpy as np
import pytest
import torch

from matcha_amd import _lib, synth
from tests.test_cpu_long_train import rows_of
from tests.test_hip_model import hip_model

pytestmark = pytest.mark.gpu

PARENT = "a9658a9"      # the tables below were recorded from a build of this commit, on an MI355X
BETA = 0.001

# name -> (kind, layout, embed_dim, front end, L, (option, value) or None, dropout, deterministic)
CASES = {
    "short_d16_table": ("step", "tiny", 16, "table", 5, None, True, True),
    "short_d128_adj_layerwise": ("step", "c1", 128, "adj", 5, ("disable_fused", 1), False, False),
    "short_d128_default": ("step", "c1", 128, "table", 5, None, False, False),
    "short_d64_fused_encoder": ("step", "c23", 64, "table", 5, ("disable_fused", 2), False, True),
    "long_d16_four_products": ("long_step", "tiny", 16, "table", 9, None, False, False),
    "long_d64_table": ("long_step", "c23", 64, "table", 9, None, True, False),
    "long_d64_adj": ("long_step", "c23", 64, "adj", 9, None, False, False),
    "long_forward_d64": ("long_forward", "c23", 64, "table", 9, None, False, False),
    "embedding_d16": ("embedding", "tiny", 16, "table", 5, None, False, False),
}

# {kernel: launches} per case, recorded from PARENT
_ADJ = {"adj_encode_fwd_kernel": 1, "adj_flags_kernel": 1, "adj_recon_dnode_kernel": 1, "adj_recon_final_kernel": 1, "adj_recon_loss_kernel": 1,
        "adj_sort_small_kernel": 1, "adj_tanh_gather_kernel": 1, "adj_tn_kernel<0>": 1, "adj_tn_kernel<1>": 1}
_TABLE_GRAD = {"tg_colscan_kernel": 1, "tg_hist_kernel": 1, "tg_idscan_kernel": 1, "tg_place_kernel": 1, "tg_runsum_kernel": 1}
_LONG_PLAN = {"long_plan_count_kernel": 1, "long_plan_fill_kernel": 1, "long_plan_scan_kernel": 1}
LAUNCHES = {
    "short_d16_table": {
        "attn_bwd_kernel": 1, "attn_fwd_kernel": 1, "attn_pad_reduce_kernel": 1, "colsum_reduce_kernel": 2, "embed_fwd_kernel": 1, "fill_i32_kernel": 1,
        "gemm_lds_kernel": 10, "gemm_tn_kernel": 8, "head_bwd_kernel": 1, "head_fwd_kernel": 1, "ln3_bwd_kernel": 1, "ln3_fwd_kernel": 1,
        "plan_small_kernel": 1, "slab_reduce_kernel": 8, "zero_f32_kernel": 1, **_TABLE_GRAD},
    "short_d128_adj_layerwise": {
        "attn_bwd_kernel": 1, "attn_bwd_wide_kernel": 1, "attn_fwd_wide_kernel": 1, "attn_pad_reduce_kernel": 1, "bmm_heads_kernel": 2,
        "colsum_reduce_kernel": 2, "embed_fwd_kernel": 1, "gemm_lds_kernel": 2, "gemm_tn_kernel": 1, "gemm_tn_wide_kernel": 6, "gemm_wide_kernel": 12,
        "head_bwd_kernel": 1, "head_fwd_kernel": 1, "head_sum_row_kernel": 1, "ln3_bwd_kernel": 1, "ln3_fwd_kernel": 1, "plan_small_kernel": 1,
        "slab_reduce_kernel": 7, "zero_f32_kernel": 3, **_ADJ},
    "short_d128_default": {
        "bmm_heads_kernel": 2, "colsum_reduce_kernel": 1, "embed_fwd_kernel": 1, "embed_scatter_kernel": 1, "enc128_bwd_kernel": 1, "enc128_colsum_kernel": 1,
        "enc128_fwd_kernel": 1, "enc128_lnhat_bwd_kernel": 1, "enc128_prep_kernel": 1, "enc128_reduce_kernel": 1, "enc128_unfold_kernel": 1,
        "fill_i32_kernel": 1, "gemm_tn_kernel": 1, "gemm_tn_wide_kernel": 3, "gemm_wide_kernel": 6, "head_bwd_kernel": 1, "head_fwd_kernel": 1,
        "plan_small_kernel": 1, "slab_reduce_kernel": 4, "zero_f32_kernel": 2},
    "short_d64_fused_encoder": {
        "colsum_reduce_kernel": 1, "embed_fwd_kernel": 1, "fb_unfold2_kernel": 1, "fbm_chain_kernel": 1, "fbm_reduce_kernel": 1, "fill_i32_kernel": 1,
        "fused_bwdh_kernel": 1, "fused_fwd32h_kernel": 1, "gemm_lds_kernel": 4, "gemm_tn_kernel": 4, "head_bwd_kernel": 1, "lnhat_bwd_kernel": 1,
        "plan_small_kernel": 1, "prep_heads_kernel": 1, "slab_reduce_kernel": 4, "zero_f32_kernel": 1, **_TABLE_GRAD},
    "long_d16_four_products": {
        "attn_long_bwd_kernel": 1, "attn_long_kernel": 1, "attn_long_pad_reduce_kernel": 1, "colsum_reduce_kernel": 2, "embed_fwd_kernel": 1,
        "embed_scatter_kernel": 1, "fill_i32_kernel": 1, "gemm_lds_kernel": 10, "gemm_tn_kernel": 8, "head_bwd_kernel": 1, "head_fwd_kernel": 1,
        "ln3_bwd_kernel": 1, "ln3_fwd_kernel": 1, "long_zero_row_kernel": 1, "slab_reduce_kernel": 8, "zero_f32_kernel": 1, **_LONG_PLAN},
    "long_d64_table": {
        "attn_long_bwd_kernel": 1, "attn_long_kernel": 1, "attn_long_pad_reduce_kernel": 1, "bmm_heads_kernel": 2, "colsum_reduce_kernel": 2,
        "embed_fwd_kernel": 1, "embed_scatter_kernel": 1, "fill_i32_kernel": 1, "gemm_lds_kernel": 8, "gemm_tn_kernel": 6, "gemm_wide_kernel": 2,
        "head_bwd_kernel": 1, "head_fwd_kernel": 1, "ln3_bwd_kernel": 1, "ln3_fwd_kernel": 1, "long_zero_row_kernel": 1, "slab_reduce_kernel": 6,
        "zero_f32_kernel": 3, **_LONG_PLAN},
    "long_d64_adj": {
        "attn_long_bwd_kernel": 1, "attn_long_kernel": 1, "attn_long_pad_reduce_kernel": 1, "bmm_heads_kernel": 2, "colsum_reduce_kernel": 2,
        "embed_fwd_kernel": 1, "gemm_lds_kernel": 12, "gemm_tn_kernel": 7, "gemm_wide_kernel": 2, "head_bwd_kernel": 1, "head_fwd_kernel": 1,
        "ln3_bwd_kernel": 1, "ln3_fwd_kernel": 1, "long_zero_row_kernel": 1, "slab_reduce_kernel": 7, "zero_f32_kernel": 3, **_LONG_PLAN, **_ADJ},
    "long_forward_d64": {
        "attn_long_kernel": 1, "bmm_heads_kernel": 1, "embed_fwd_kernel": 1, "gemm_lds_kernel": 4, "gemm_wide_kernel": 1, "head_fwd_kernel": 1,
        "ln3_fwd_kernel": 1, "zero_f32_kernel": 1, **_LONG_PLAN},
    "embedding_d16": {
        "attn_fwd_kernel": 1, "embed_fwd_kernel": 1, "expand_embedding_kernel": 1, "gemm_lds_kernel": 5, "ln3_fwd_kernel": 1, "plan_small_kernel": 1,
        "zero_f32_kernel": 1},
}

_MODELS = {}


def model(layout, d, mode, dropout):
    key = (layout, d, mode, dropout)
    if key not in _MODELS:
        clf, _ = hip_model(synth.LAYOUTS[layout], d, mode, 700 + d)
        if not dropout:
            for m in clf.modules():
                if isinstance(m, torch.nn.Dropout):
                    m.p = 0.0
        _MODELS[key] = clf.train()
    return _MODELS[key]


def batch(layout, L, B=7):
    """x [B, L] with rows of k = L, 2, 1, 0 and B - 4 random k; labels and weights."""
    rng = np.random.default_rng(900 + L)
    N = int(np.sum(synth.LAYOUTS[layout]))
    ks = ([L, 2, 1, 0] + [int(k) for k in rng.integers(1, L + 1, size=max(B - 4, 0))])[:B]
    return rows_of(rng, N, ks, L), (rng.random(B) < 0.5).astype(np.float32), (0.5 + 1.5 * rng.random(B)).astype(np.float32)


class Call:
    """The arguments of one case's entry points: a model's runtime, a batch on the device, the output and gradient buffers."""

    def __init__(self, clf, x, y, w, dropout=False, deterministic=False):
        self.clf, self.rt = clf, clf._runtime()
        rt = self.rt
        self.lib = rt.lib
        np.random.seed(0)
        self.opts, _ = clf._opts(rt, True)
        o = self.opts
        o.training, o.forward_only, o.random_chrom, o.deterministic = 1, 0, 1, int(deterministic)
        o.status = rt.status.data_ptr()
        self.seed = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
        o.seed = self.seed.data_ptr() if dropout else None
        if not dropout:
            o.p_drop_adj = o.p_drop_fc1 = o.p_drop_pff = 0.0
        self.x = torch.from_numpy(x).cuda().contiguous()
        self.y, self.w = torch.from_numpy(y).cuda(), torch.from_numpy(w).cuda()
        self.B, self.L = self.x.shape
        self.logits = torch.full((self.B,), float("nan"), dtype=torch.float32, device="cuda")
        self.losses = torch.zeros(3, dtype=torch.float32, device="cuda")
        self.gflat = torch.zeros(rt.n_flat, dtype=torch.float32, device="cuda")
        self.grads = rt.tensors_for(self.gflat)
        self.touched = torch.zeros(rt.n_touched, dtype=torch.int32, device="cuda")
        self.dr = torch.full((1,), BETA, dtype=torch.float32, device="cuda")

    def head(self, opts=None):
        rt = self.rt
        return (C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts or self.opts), _lib.ptr(self.x), self.B, self.L)

    def forward(self, ws, long_rows):
        out = (_lib.ptr(self.logits), _lib.ptr(self.losses), _lib.ptr(ws), ws.numel(), self.rt.stream())
        if long_rows:
            return self.lib.matcha_forward_long_train(*self.head(), *out)
        return self.lib.matcha_forward(*self.head(), None, None, *out)

    def backward(self, ws, long_rows):
        dl = (self.w * (torch.sigmoid(self.logits) - self.y) / self.B).contiguous()
        self.gflat.zero_()
        tail = (C.byref(self.grads), _lib.ptr(self.touched), _lib.ptr(ws), ws.numel(), self.rt.stream())
        if long_rows:
            rc = self.lib.matcha_backward_long(*self.head(), _lib.ptr(dl), _lib.ptr(self.dr), *tail)
        else:
            rc = self.lib.matcha_backward(*self.head(), None, None, _lib.ptr(dl), _lib.ptr(self.dr), *tail)
        torch.cuda.synchronize()
        return rc

    def error(self):
        return self.lib.matcha_last_error().decode()

    def outputs(self):
        out = {"logits": self.logits.cpu().numpy(), "losses": self.losses.cpu().numpy(), "touched": self.touched.cpu().numpy()}
        names = {id(p): n for n, p in self.clf.named_parameters()}
        for p, o in zip(self.rt.live, self.rt.seg_off_list[:-1]):
            out["grad/" + names[id(p)]] = self.gflat[o:o + p.numel()].cpu().numpy()
        return out


def run_case(name):
    """({kernel: launches}, {output name: array}) of one case."""
    kind, layout, d, mode, L, option, dropout, deterministic = CASES[name]
    clf = model(layout, d, mode, dropout)
    c = Call(clf, *batch(layout, L), dropout=dropout, deterministic=deterministic)
    rt, lib = c.rt, c.lib
    if option:
        _lib.set_option(*option)
    try:
        with _lib.launch_log() as log:
            if kind in ("step", "long_step"):
                long_rows = kind == "long_step"
                ws = rt.workspace(c.B, L, long_train=True) if long_rows else rt.workspace(c.B, L)
                ws.fill_(0xFF)
                rc = c.forward(ws, long_rows)
                assert rc == 0, c.error()
                rc = c.backward(ws, long_rows)
                assert rc == 0, c.error()
                out = c.outputs()
            elif kind == "long_forward":
                o = c.opts
                o.training, o.forward_only = 0, 1
                ws = rt.workspace(c.B, L, long_rows=True)
                ws.fill_(0xFF)
                rc = lib.matcha_forward_long(*c.head(), _lib.ptr(c.logits), _lib.ptr(c.losses), _lib.ptr(ws), ws.numel(), rt.stream())
                assert rc == 0, c.error()
                out = {"logits": c.logits.cpu().numpy(), "losses": c.losses.cpu().numpy()}
            else:
                o = c.opts
                o.training = 0
                ws = rt.workspace(c.B, L)
                ws.fill_(0xFF)
                dyn = torch.empty(c.B, L, d, dtype=torch.float32, device="cuda")
                sta, attn = torch.empty_like(dyn), torch.empty(c.B, _lib.N_HEAD, L, L, dtype=torch.float32, device="cuda")
                rc = lib.matcha_get_embedding(*c.head(), _lib.ptr(dyn), _lib.ptr(sta), _lib.ptr(attn), _lib.ptr(c.losses), _lib.ptr(ws), ws.numel(),
                                              rt.stream())
                assert rc == 0, c.error()
                out = {"dynamic": dyn.cpu().numpy(), "static": sta.cpu().numpy(), "attn": attn.cpu().numpy(), "losses": c.losses.cpu().numpy()}
            torch.cuda.synchronize()
    finally:
        if option:
            _lib.set_option(option[0], 0)
    return {k: n for k, n in log.counts.items() if n > 0}, out


@pytest.mark.parametrize("name", list(CASES))
def test_launches_are_the_parents(name):
    counts, out = run_case(name)
    print(name, counts)
    for k, v in out.items():
        if k != "attn":      # (the raw copy of P: rows of padding queries are never written -- Classifier.get_embedding zeroes them)
            assert np.isfinite(v).all(), (name, k)
    kind = CASES[name][0]
    # the case runs what its name says
    if name == "short_d128_default":
        assert "enc128_fwd_kernel" in counts and "enc128_bwd_kernel" in counts, sorted(counts)
    if name == "short_d128_adj_layerwise":
        assert not any(k.startswith("enc128") for k in counts) and "bmm_heads_kernel" in counts, sorted(counts)
    if name == "short_d64_fused_encoder":
        assert "fused_bwdh_kernel" in counts and "embed_fwd_kernel" in counts, sorted(counts)
    if kind.startswith("long"):
        assert "attn_long_kernel" in counts and ("bmm_heads_kernel" in counts) == (CASES[name][2] % 64 == 0), sorted(counts)
    assert counts == LAUNCHES[name], (name, {k: (counts.get(k), LAUNCHES[name].get(k)) for k in set(counts) | set(LAUNCHES[name])
                                             if counts.get(k) != LAUNCHES[name].get(k)})


def _refused(c, ws, long_rows):
    with _lib.launch_log() as log:
        rc = c.backward(ws, long_rows)
    assert rc == -22 and "on record" in c.error(), (rc, c.error())
    assert ("matcha_forward_long_train" in c.error()) == long_rows, c.error()
    assert not {k for k, n in log.counts.items() if n > 0}, log.counts      # refused before any launch


def test_one_forward_record_per_workspace_for_both_pairs():
    clf = model("tiny", 16, "table", False)
    c = Call(clf, *batch("tiny", 8, B=4))
    rt = c.rt
    n = max(c.lib.matcha_workspace_bytes(C.byref(rt.shape), 4, 8), c.lib.matcha_workspace_bytes_long_train(C.byref(rt.shape), 4, 8))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    for first_long in (True, False):
        assert c.forward(ws, first_long) == 0, c.error()
        assert c.forward(ws, not first_long) == 0, c.error()      # the second forward overwrote what the first left: its record is the one that stands
        _refused(c, ws, first_long)
        assert c.backward(ws, not first_long) == 0, c.error()     # (the refusal left the record in place)
        assert np.isfinite(c.gflat.cpu().numpy()).all()
        _refused(c, ws, not first_long)                            # one backward per forward
