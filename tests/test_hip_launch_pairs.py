"""Paired launches of the fused d = 64 step (model.hip: StepRoute::paired): independent small launches share a launch -- on the
node route the plan's tile_pack pass rides in the table front end's forward and tile_compact in node_r_kernel; everywhere on the merged backward
fbm_chain_kernel's blocks un-fold their own rows (no fb_unfold_kernel); on the node route fb_unfold2's vectors ride in node_scatter_kernel
(either body).  Every role runs the text of the stand-alone kernel, so against the same step with every launch on its own (option
disable_launch_pairs) the plan, the forward's outputs and every encoder gradient are compared BITWISE.  The front end's gradients pass through
float atomics on the node route (the order of the adds differs from run to run): they are held to the repository's route-against-route
bound, 2e-5 of each tensor's largest element, and to the fp64 oracle's grade (tests/fp64_grade.py, K = 8) on the dropout-free batch.

Shapes: c23 (150 nodes).  3 072 mixed-k rows of L = 5 -- capacity 15 361 >= 64 x 151, the smallest that takes the value table and node_dx, 8
planning superblocks -- and 1 536 rows of L = 8 (capacity 12 289).  The workspace starts as NaN bytes (MATCHA_POISON_WS).  GPU only (-m gpu).
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from matcha_amd import synth, _lib
from tests import fp64_grade as G
from tests.test_hip_model import hip_model, _trainer_grads
from tests.test_hip_node_dx import _compare, _got
from tests.test_hip_node_front import _bitwise, _c23, _id_batch, _no_dropout

pytestmark = pytest.mark.gpu

AWAY = {"tile_pack_kernel", "tile_compact_kernel", "fb_unfold_kernel", "fb_unfold2_kernel"}       # launches the pairs take out of a node-route step
PINNED = ["front_fwd3_kernel", "node_xhat_kernel", "node_r_kernel", "fused_fwd32_kernel", "tail_bwd64_kernel", "fused_bwdh_kernel", "fbm_reduce_kernel",
          "fbm_chain_kernel", "node_scatter_kernel", "front_bwd_kernel"]


@pytest.fixture(autouse=True)
def _poisoned_workspace(monkeypatch):
    monkeypatch.setenv("MATCHA_POISON_WS", "nan")


def _setting(pairs):
    return contextlib.nullcontext() if pairs else _lib.option("disable_launch_pairs")


def _cdiv(a, b):
    return -(-a // b)


def _plan(ws, B, L):
    """The plan's arrays as the forward left them at the head of the workspace (ragged.hip: ragged_carve's order and 256-byte alignment, checked
    against matcha_ragged_plan_bytes).  What later kernels or matcha_ragged_view read; the packing scratch (sb_*) is not part of the plan."""
    T = B * L
    nsb = _cdiv(T + 1, 63 * 32)
    tiles, halves = _cdiv(T + 1, 64 - L) + nsb, _cdiv(T + 1, 32 - L) + nsb
    sb_cap, sb_hcap = _cdiv(63 * 32 + L, 64 - L) + 2, _cdiv(63 * 32 + L, 32 - L) + 2
    fields = [("row_off", (B + 1) * 4), ("tok_slot", (T + 1) * 4), ("tok_id", (T + 1) * 8), ("count", 256), ("blk_sum", _cdiv(B, 256) * 4),
              ("tok_pos", (T + 1) * 4), ("tok_key", (T + 1) * 4), ("tile_meta", (tiles + 2) * 16), ("sb_tiles", nsb * sb_cap * 16), ("sb_cnt", nsb * 4),
              ("sb_first", (nsb + 1) * 4), ("half_meta", (halves + 2) * 16), ("sb_htiles", nsb * sb_hcap * 16), ("sb_hcnt", nsb * 4), ("tok_tile", (T + 1) * 4)]
    off, out = 0, {}
    raw = ws.view(torch.uint8)
    for name, nbytes in fields:
        if not name.startswith("sb_") and name != "blk_sum":
            out[name] = raw[off:off + (16 if name == "count" else nbytes)].cpu().numpy().copy()
        off += _cdiv(nbytes, 256) * 256
    assert off == _lib.load().matcha_ragged_plan_bytes(B, L), (off, B, L)
    return out


def _same_plan(label, a, b):
    assert a.keys() == b.keys()
    for n in a:
        assert np.array_equal(a[n], b[n]), (label, n, int((a[n] != b[n]).sum()))
    cnt = a["count"].view(np.int32)
    assert cnt[0] == cnt[1] + 1 and cnt[2] == 0 and cnt[3] > 0, (label, cnt)      # the forward plans half tiles only
    return cnt


def _grads(tr, clf):
    return {n: (None if v is None else v.cpu().double().numpy()) for n, v in _trainer_grads(tr, clf).items()}


def _run(pairs, x, y, w, *, dropout, node=True, prepare=None, **trainer_kw):
    """One Trainer.forward_backward on a fresh model and Trainer under one setting of the switch: logits, losses, gradients, launch counts, the
    plan, the status word."""
    from matcha_amd.engine import Trainer
    c = _c23()
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
    if not dropout:
        _no_dropout(clf)
    clf.train()
    with _setting(pairs), (contextlib.nullcontext() if node else _lib.option("disable_node_front")):
        tr = Trainer(clf, lr=1e-3, base_seed=11, **trainer_kw)
        if prepare:
            prepare(tr)
        xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (x, y, w))
        with _lib.launch_log() as log:
            logits = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
            torch.cuda.synchronize()
    ws, _ = tr._buffers(*x.shape)
    return dict(lg=logits.cpu().numpy().copy(), ls=tr.losses.cpu().numpy().copy(), g=_grads(tr, clf), counts={k: n for k, n in log.counts.items() if n > 0},
                plan=_plan(ws, *x.shape), status=tr.rt.status.cpu().numpy().copy())


def _batch(kind):
    """(x, y, w).  L = 5: 3 072 rows but for `odd_rows`; `l8`: 1 536 rows of L = 8."""
    c = _c23()
    x, y, w = c["x"].copy(), c["y"], c["w"]
    rng = np.random.default_rng(581)
    if kind == "mixed":
        pass
    elif kind in ("five", "foreign"):
        x = _id_batch(kind)
    elif kind == "pads_inside":                                # every row's slots in a random order: pads may sit anywhere in the row
        x = np.take_along_axis(x, np.argsort(rng.random(x.shape), axis=1), axis=1)
    elif kind == "empty_rows":                                 # a run of all-padding rows across a 256-row block boundary, and scattered ones
        x[200:330] = 0
        x[rng.choice(len(x), size=150, replace=False)] = 0
    elif kind == "odd_rows":                                   # 3 100 rows: not a multiple of the 256 rows of a counting block
        x, y, w = G.make_case_batch("c23", [2, 3, 4, 5], 775, 582, 5)
        assert x.shape == (3100, 5)
    elif kind == "l8":
        x, y, w = G.make_case_batch("c23", [2, 3, 4, 5], 384, 583, 8)
        assert x.shape == (1536, 8) and 1536 * 8 + 1 >= 64 * 151
    elif kind == "l8_pads_inside":
        x, y, w = G.make_case_batch("c23", [2, 3, 5, 8], 384, 584, 8)
        x = np.take_along_axis(x, np.argsort(rng.random(x.shape), axis=1), axis=1)
        x[700:800] = 0
    else:
        raise KeyError(kind)
    return x, y, w


def _check_log(on, off):
    """Default: none of the four launches, each pinned name once.  With the switch: the same step with the four launches back, once each."""
    assert not (AWAY & on.keys()), sorted(AWAY & on.keys())
    for n in PINNED:
        assert on.get(n, 0) == 1 and off.get(n, 0) == 1, (n, on, off)
    assert set(off) == set(on) | AWAY, sorted(set(off) ^ set(on))
    assert all(off[n] == 1 for n in AWAY), off
    assert all(off[n] == on[n] for n in on), (on, off)
    assert sum(off.values()) == sum(on.values()) + 4


@pytest.mark.parametrize("kind", ["mixed", "pads_inside", "empty_rows", "odd_rows", "five", "foreign", "l8", "l8_pads_inside"])
def test_paired_step_is_bitwise(kind):
    """Dropout on: the plan, logits, both losses and every encoder gradient bitwise between the settings; the front end's gradients within the
    bound; the launch log; the status word."""
    x, y, w = _batch(kind)
    on, off = (_run(p, x, y, w, dropout=True) for p in (True, False))
    _check_log(on["counts"], off["counts"])
    cnt = _same_plan(kind, on["plan"], off["plan"])
    assert cnt[1] == int(((x != 0)).sum()) and int(cnt[3]) >= _cdiv(int(cnt[1]), 31)
    assert np.array_equal(on["status"], off["status"]) and bool(on["status"][0] != 0) == (kind == "foreign"), (on["status"], off["status"])
    assert _bitwise(on["lg"], off["lg"]) and _bitwise(on["ls"], off["ls"]), (on["ls"], off["ls"])
    assert np.isfinite(on["lg"]).all() and np.isfinite(on["ls"]).all()
    _compare(f"{kind}: pairs against single launches", on["g"], off["g"])


def test_gradients_at_fp64_grade():
    """Dropout-free on the shared batch: both settings at the oracle's grade (K = 8), encoder gradients bitwise between them."""
    c = _c23()
    on, off = (_run(p, c["x"], c["y"], c["w"], dropout=False) for p in (True, False))
    _check_log(on["counts"], off["counts"])
    for label, r in (("pairs", on), ("single launches", off)):
        G.assert_grade(label, G.grade(_got(r["lg"], r["ls"], r["g"]), c["ref"]))
    assert _bitwise(on["lg"], off["lg"]) and _bitwise(on["ls"], off["ls"])
    _compare("dropout-free", on["g"], off["g"])


def test_token_walk_hosts_the_vectors_too():
    """disable_node_dx: node_scatter_kernel walks the tokens; its launch hosts fb_unfold2's vectors like the per-node finisher's (the launches of
    a node-route step do not depend on where d x_hat is summed)."""
    c = _c23()
    with _lib.option("disable_node_dx"):
        on, off = (_run(p, c["x"], c["y"], c["w"], dropout=True) for p in (True, False))
    _check_log(on["counts"], off["counts"])
    _same_plan("token walk", on["plan"], off["plan"])
    assert _bitwise(on["lg"], off["lg"]) and _bitwise(on["ls"], off["ls"])
    _compare("token walk: pairs against single launches", on["g"], off["g"])


def test_inference_forward():
    """A forward that keeps nothing (compact workspace; no node_xhat_kernel): the plan's arrays and the logits bitwise, the two plan launches gone."""
    from matcha_amd.engine import Trainer
    c = _c23()
    out = {}
    for pairs in (True, False):
        clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
        clf.eval()
        tr = Trainer(clf, lr=1e-3, base_seed=11)
        xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))
        key = (*c["x"].shape, "eval")                         # eval_forward's workspace, handed over as NaN bytes
        ws = tr._ws[key] = tr.rt.workspace(*c["x"].shape, forward_only=True)
        ws.fill_(0xFF)
        tr._logits[key] = torch.empty(len(c["x"]), dtype=torch.float32, device=ws.device)
        with _setting(pairs), _lib.launch_log() as log:
            lg = tr.eval_forward(xd, yd, wd).cpu().numpy().copy()
            torch.cuda.synchronize()
        out[pairs] = (lg, {k: n for k, n in log.counts.items() if n > 0}, _plan(ws, *c["x"].shape))
    on, off = out[True][1], out[False][1]
    assert "node_xhat_kernel" not in on and on.get("node_r_kernel", 0) == 1 and on.get("front_fwd3_kernel", 0) == 1 and on.get("fused_fwd32_kernel", 0) == 1, on
    assert set(off) == set(on) | {"tile_pack_kernel", "tile_compact_kernel"} and not ({"tile_pack_kernel", "tile_compact_kernel"} & on.keys()), (on, off)
    _same_plan("inference", out[True][2], out[False][2])
    assert _bitwise(out[True][0], out[False][0]) and np.isfinite(out[True][0]).all()


class _Abi:
    """matcha_forward and matcha_backward as two calls on one Trainer's buffers (tests/test_hip_route_record.py), dropout-free."""

    def __init__(self):
        from matcha_amd.engine import Trainer
        c = _c23()
        self.clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
        _no_dropout(self.clf)
        self.clf.train()
        self.tr = tr = Trainer(self.clf, lr=1e-3, base_seed=11)
        self.batch = tuple(torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))
        self.B, self.L = c["x"].shape
        self.ws, self.logits = tr._buffers(self.B, self.L)
        self.opts = tr._opts(1.0, 0.001, 0)

    def step(self, fwd_pairs, bwd_pairs):
        tr, rt, (xd, yd, wd) = self.tr, self.tr.rt, self.batch
        self.ws.fill_(0xFF)
        with _setting(fwd_pairs):
            _lib.check(tr.lib.matcha_forward(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(self.opts), _lib.ptr(xd), self.B, self.L,
                                             _lib.ptr(yd), _lib.ptr(wd), _lib.ptr(self.logits), _lib.ptr(tr.losses), _lib.ptr(self.ws), self.ws.numel(),
                                             rt.stream()), "matcha_forward")
        tr.gflat.zero_()
        with _setting(bwd_pairs), _lib.launch_log() as log:
            _lib.check(tr.lib.matcha_backward(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(self.opts), _lib.ptr(xd), self.B, self.L,
                                              _lib.ptr(yd), _lib.ptr(wd), None, None, C.byref(tr.grads), _lib.ptr(tr.touched), _lib.ptr(self.ws), self.ws.numel(),
                                              rt.stream()), "matcha_backward")
        torch.cuda.synchronize()
        return _grads(tr, self.clf), {k: n for k, n in log.counts.items() if n > 0}


@pytest.mark.parametrize("fwd_pairs", [True, False], ids=["forward_default", "forward_disable_launch_pairs"])
def test_backward_follows_the_recorded_route(fwd_pairs):
    """The switch flipped between the two calls: the backward launches what the forward's record says, with the bits of the un-flipped run."""
    a = _Abi()
    want, want_log = a.step(fwd_pairs, fwd_pairs)
    got, log = a.step(fwd_pairs, not fwd_pairs)
    assert log == want_log, (log, want_log)
    assert ("fb_unfold_kernel" in log) == ("fb_unfold2_kernel" in log) == (not fwd_pairs), log
    _compare(f"forward {fwd_pairs}, backward {not fwd_pairs}", got, want)


def test_three_optimiser_steps_on_a_poisoned_workspace():
    """Three steps on ONE workspace that starts as NaN, under both settings: the first step's logits and losses bitwise between them (later steps
    start from parameters that differ by the front end's atomics), finite losses and parameters throughout, logits that move."""
    from matcha_amd.engine import Trainer
    c = _c23()
    first = {}
    for pairs in (True, False):
        clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
        clf.train()
        with _setting(pairs):
            tr = Trainer(clf, lr=1e-3, base_seed=11)
            xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))
            seen = []
            for i in range(3):
                _, _, lg = tr.step(xd, yd, wd, 1.0, 0.001, 0)
                torch.cuda.synchronize()
                seen.append(lg.cpu().numpy().copy())
                ls = tr.losses.cpu().numpy().copy()
                assert np.isfinite(ls).all() and np.isfinite(seen[-1]).all(), (pairs, i, ls)
                assert all(bool(torch.isfinite(p).all()) for p in clf.parameters()), (pairs, i)
                if i == 0:
                    first[pairs] = (seen[0], ls)
        assert not _bitwise(seen[0], seen[1]) and not _bitwise(seen[1], seen[2])
    assert _bitwise(first[True][0], first[False][0]) and _bitwise(first[True][1], first[False][1])


def test_graph_replay_equals_eager():
    from matcha_amd.engine import Trainer
    c = _c23()
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
    _no_dropout(clf)
    clf.train()
    tr = Trainer(clf, lr=1e-3, base_seed=11)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))
    with _lib.launch_log() as log:
        eager = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0).clone()
    torch.cuda.synchronize()
    assert not (AWAY & {k for k, n in log.counts.items() if n > 0}) and log.counts.get("node_scatter_kernel", 0) == 1, log.counts
    g_eager = _grads(tr, clf)
    plan_eager = _plan(tr._buffers(*c["x"].shape)[0], *c["x"].shape)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
    out.zero_()
    tr.gflat.zero_()
    tr._buffers(*c["x"].shape)[0].fill_(0xFF)                                    # the replay rebuilds the plan from NaN bytes
    graph.replay()
    torch.cuda.synchronize()
    assert _bitwise(out.cpu().numpy(), eager.cpu().numpy())
    _same_plan("replay", _plan(tr._buffers(*c["x"].shape)[0], *c["x"].shape), plan_eager)
    _compare("one replay against eager", _grads(tr, clf), g_eager)


def _all_bitwise(label, a, b):
    for n, v in b.items():
        assert (a[n] is None) == (v is None), (label, n)
        if v is not None:
            assert np.array_equal(a[n], v), (label, n, float(np.abs(a[n] - v).max()))


def test_small_batch_and_per_token_routes():
    """Off the node route only the backward's un-folding is paired (one launch less).  384 rows (the small-batch kernels) and the per-token front end
    at 3 072 rows.  With the fixed-order sums (`deterministic`: no float atomics anywhere in the step) EVERY gradient is bitwise between the
    settings; with the default options (the heads' d x_hat and the table rows through float atomics, whose order differs from run to run) the
    encoder gradients are bitwise and the front end's within the bound."""
    c = _c23()
    xs, ys, ws_ = G.make_case_batch("c23", [2, 3, 4, 5], 96, 585, 5)
    assert xs.shape == (384, 5)
    for label, (x, y, w), node, must in (("384 rows", (xs, ys, ws_), True, "plan_small_kernel"), ("per token", (c["x"], c["y"], c["w"]), False, "tile_pack_kernel")):
        on, off = (_run(p, x, y, w, dropout=True, node=node, deterministic=True) for p in (True, False))
        assert "node_scatter_kernel" not in on["counts"] and must in on["counts"], (label, on["counts"])
        assert set(off["counts"]) == set(on["counts"]) | {"fb_unfold_kernel"} and "fb_unfold_kernel" not in on["counts"], (label, on["counts"], off["counts"])
        assert on["counts"].get("fb_unfold2_kernel", 0) == 1 and on["counts"].get("fbm_chain_kernel", 0) == 1, (label, on["counts"])
        assert sum(off["counts"].values()) == sum(on["counts"].values()) + 1, label
        for n in on["plan"]:
            assert np.array_equal(on["plan"][n], off["plan"][n]), (label, n)
        assert _bitwise(on["lg"], off["lg"]) and _bitwise(on["ls"], off["ls"]), label
        _all_bitwise(label, on["g"], off["g"])
        on, off = (_run(p, x, y, w, dropout=True, node=node) for p in (True, False))
        assert sum(off["counts"].values()) == sum(on["counts"].values()) + 1 and "fb_unfold_kernel" not in on["counts"], (label, on["counts"])
        assert _bitwise(on["lg"], off["lg"]) and _bitwise(on["ls"], off["ls"]), label
        _compare(f"{label}, default options", on["g"], off["g"])
