"""Per-node sums of the encoder's input gradients at their producers (model.hip: StepRoute::node_dx).  On the node route with the
value table the eight heads of fused_bwdh_kernel add their d x_hat rows into one per-node replica each, the forward's tail adds its dXs rows per
node, tail_bwd64_kernel zeroes the replicas, and node_scatter_kernel -- the same launch name -- is the per-node finisher
G[node] = LNbwd(sum_h AH[h][node] ; x_hat_node) + AS[node]: no [T, 64] d x_hat buffer, no dXs row per token, no walk over the tokens.  Against the
same route with the sums formed by the token walk (option disable_node_dx): the forward's outputs and every encoder gradient do not depend on
where d x_hat is summed, so they are compared BITWISE; the front end's gradients are the same sums in another order and are held to the
fp64 oracle's grade (tests/fp64_grade.py, K = 8) and to the repository's route-against-route bound, 2e-5 of each tensor's largest element.

Which body ran is read off the workspace: it starts as NaN bytes (MATCHA_POISON_WS), and the dXs rows are written by the forward exactly when the
sums are NOT formed at the producers.  Shape: test_hip_node_front.py's (c23, 150 nodes, 3 072 mixed-k rows, L = 5: capacity 15 361 >= 64 x 151),
its helpers re-used.  GPU only (-m gpu).
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from matcha_amd import synth, _lib
from tests import fp64_grade as G
from tests import state_twin as S
from tests.helpers import oracle_state
from tests.test_hip_model import hip_model, _trainer_grads
from tests.test_hip_node_front import _bitwise, _c23, _id_batch, _no_dropout, _step
from tests.test_hip_node_r import _close

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _poisoned_workspace(monkeypatch):
    monkeypatch.setenv("MATCHA_POISON_WS", "nan")


def _setting(dx):
    return contextlib.nullcontext() if dx else _lib.option("disable_node_dx")


def _run(dx, sd, x, y, w, *, dropout, layout="c23", prepare=None, seed=0):
    with _setting(dx):
        return _step(layout, sd, x, y, w, node=True, dropout=dropout, prepare=prepare, seed=seed)


def _dxs_written(tr, B, L):
    """Did the forward store dXs rows per token?  (The first 16 token rows of the poisoned workspace's dXs buffer.)"""
    ws, _ = tr._buffers(B, L)
    buf = C.create_string_buffer(8192)
    fn = tr.lib.matcha_debug_layout
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_char_p, C.c_size_t]
    assert fn(C.byref(tr.rt.shape), B, L, buf, 8192) == 0
    lay = dict((ln.split()[0], int(ln.split()[1])) for ln in buf.value.decode().strip().split("\n"))
    off = lay["dXs"]
    words = ws.view(torch.uint8)[off:off + 16 * 64 * 4].cpu().numpy().view(np.uint32)
    untouched = bool((words == 0xFFFFFFFF).all())
    assert untouched or bool(np.isfinite(words.view(np.float32)).all())
    return not untouched


def _got(lg, ls, g):
    return G.StepOut(lg.astype(np.float64), {"bce": float(ls[0]), "recon": float(ls[1])}, g)


def _front(name):
    return name.startswith(S.FRONT)


def _compare(label, g, g_off):
    """Encoder gradients (ln_q_g .. cls_b) bitwise, the front end's within the bound."""
    for n, b in g_off.items():
        a = g[n]
        assert (a is None) == (b is None), (label, n)
        if b is not None and not _front(n):
            assert np.array_equal(a, b), (label, n, float(np.abs(a - b).max()))
    _close(label, {n: v for n, v in g.items() if _front(n)}, {n: v for n, v in g_off.items() if _front(n)})


def test_forward_is_bitwise_and_the_launches_are_the_same():
    c = _c23()
    out = {}
    for dx in (True, False):
        lg, ls, _, ran, (tr, _, xd) = _run(dx, c["sd"], c["x"], c["y"], c["w"], dropout=True)
        tr.check_status()
        assert {"node_scatter_kernel", "node_r_kernel", "tail_bwd64_kernel", "fused_fwd32_kernel", "fused_bwdh_kernel", "front_bwd_kernel"} <= ran, sorted(ran)
        assert _dxs_written(tr, *xd.shape) == (not dx), dx
        out[dx] = (lg, ls, ran)
    assert _bitwise(out[True][0], out[False][0])
    assert _bitwise(out[True][1], out[False][1]), (out[True][1], out[False][1])
    assert out[True][2] == out[False][2], sorted(out[True][2] ^ out[False][2])


def _batch(kind):
    c = _c23()
    if kind == "mixed":
        return c["x"], c["y"], c["w"]
    if kind in ("five", "few", "foreign"):
        return _id_batch(kind), c["y"], c["w"]
    k = {"all_k5": 5, "all_k2": 2}[kind]                   # no padding key anywhere / three padding slots per row: dxpad dominates row 0
    x, y, w = G.make_case_batch("c23", [k], 3072, 574 if k == 5 else 576, 5)
    assert x.shape == (3072, 5) and ((x != 0).sum(1) == k).all()
    return x, y, w


@pytest.mark.parametrize("kind", ["mixed", "five", "few", "all_k5", "all_k2", "foreign"])
def test_gradients(kind):
    """Dropout-free: the default at fp64 grade (where the oracle takes the batch: not the foreign ids), its encoder gradients bitwise and its
    front-end gradients within 2e-5 of each tensor's largest element of disable_node_dx's."""
    c = _c23()
    x, y, w = _batch(kind)
    lg, ls, g, ran, (tr, _, xd) = _run(True, c["sd"], x, y, w, dropout=False)
    assert not _dxs_written(tr, *xd.shape)
    if kind == "foreign":
        with pytest.raises(IndexError):
            tr.check_status()
    else:
        tr.check_status()
        ref = c["ref"] if kind == "mixed" else G.references(c["sd"], c["fe"], x, y, w, chrom=0)
        G.assert_grade(f"{kind}: per-node sums at the producers", G.grade(_got(lg, ls, g), ref))
    lg1, ls1, g1, ran1, (tr1, _, _) = _run(False, c["sd"], x, y, w, dropout=False)
    assert _dxs_written(tr1, *xd.shape)
    assert ran == ran1 and "node_scatter_kernel" in ran
    assert _bitwise(lg, lg1) and _bitwise(ls, ls1)
    _compare(f"{kind}: producers against the token walk", g, g1)


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

    def step(self, fwd_dx, bwd_dx):
        tr, rt, (xd, yd, wd) = self.tr, self.tr.rt, self.batch
        self.ws.fill_(0xFF)
        with _setting(fwd_dx):
            _lib.check(tr.lib.matcha_forward(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(self.opts), _lib.ptr(xd), self.B, self.L,
                                             _lib.ptr(yd), _lib.ptr(wd), _lib.ptr(self.logits), _lib.ptr(tr.losses), _lib.ptr(self.ws), self.ws.numel(),
                                             rt.stream()), "matcha_forward")
        tr.gflat.zero_()
        with _setting(bwd_dx), _lib.launch_log() as log:
            _lib.check(tr.lib.matcha_backward(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(self.opts), _lib.ptr(xd), self.B, self.L,
                                              _lib.ptr(yd), _lib.ptr(wd), None, None, C.byref(tr.grads), _lib.ptr(tr.touched), _lib.ptr(self.ws), self.ws.numel(),
                                              rt.stream()), "matcha_backward")
        torch.cuda.synchronize()
        g = {n: (None if v is None else v.cpu().double().numpy()) for n, v in _trainer_grads(tr, self.clf).items()}
        return g, {k for k, n in log.counts.items() if n > 0}, _dxs_written(tr, self.B, self.L)


@pytest.mark.parametrize("fwd_dx", [True, False], ids=["forward_default", "forward_disable_node_dx"])
def test_backward_follows_the_recorded_route(fwd_dx):
    """The switch flipped between the two calls: the backward consumes what the forward left -- the kernels and, within the bound, the
    gradients of the un-flipped run of the forward's setting -- and holds the oracle's grade."""
    a = _Abi()
    want, want_ran, want_dxs = a.step(fwd_dx, fwd_dx)
    got, ran, dxs = a.step(fwd_dx, not fwd_dx)
    assert dxs == want_dxs == (not fwd_dx)
    assert ran == want_ran and "node_scatter_kernel" in ran, sorted(ran ^ want_ran)
    _compare(f"forward {fwd_dx}, backward {not fwd_dx}", got, want)
    ref = _c23()["ref"]
    grads = {n: None for n in ref.r64.grads}
    grads.update(got)
    G.assert_grade("flipped", G.grade(G.StepOut(a.logits.cpu().double().numpy(), {"bce": float(a.tr.losses[0]), "recon": float(a.tr.losses[1])}, grads), ref))


def test_accumulators_are_zeroed_inside_the_step():
    """Three steps on ONE workspace that starts as NaN: each at the oracle's grade (a replica or a dXs sum left over from the step before would
    double it), then three optimiser steps: finite losses and parameters, logits that move."""
    from matcha_amd.engine import Trainer
    c = _c23()
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
    _no_dropout(clf)
    clf.train()
    tr = Trainer(clf, lr=1e-3, base_seed=11)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))
    for i in range(3):
        tr.gflat.zero_()
        lg = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
        torch.cuda.synchronize()
        assert not _dxs_written(tr, *xd.shape)
        g = {n: (None if v is None else v.cpu().double().numpy()) for n, v in _trainer_grads(tr, clf).items()}
        G.assert_grade(f"step {i} on one workspace", G.grade(_got(lg.cpu().numpy(), tr.losses.cpu().numpy(), g), c["ref"]))
    seen = []
    for _ in range(3):
        tr.step(xd, yd, wd, 1.0, 0.001, 0)
        torch.cuda.synchronize()
        assert np.isfinite(tr.losses.cpu().numpy()).all()
        assert all(bool(torch.isfinite(p).all()) for p in clf.parameters())
        clf.eval()
        with torch.no_grad():
            seen.append(clf(xd).cpu().numpy().copy())
        clf.train()
        assert np.isfinite(seen[-1]).all()
    assert not _bitwise(seen[0], seen[1]) and not _bitwise(seen[1], seen[2])


def test_sequences_on_one_workspace():
    """default, disable_node_dx, default on ONE Trainer (one workspace, gradients re-zeroed in between) equal fresh runs."""
    from matcha_amd.engine import Trainer
    c = _c23()
    fresh = {dx: _run(dx, c["sd"], c["x"], c["y"], c["w"], dropout=False) for dx in (True, False)}
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
    _no_dropout(clf)
    clf.train()
    tr = Trainer(clf, lr=1e-3, base_seed=11)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))
    for dx in (True, False, True):
        tr.gflat.zero_()
        with _setting(dx), _lib.launch_log() as log:
            lg = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
            torch.cuda.synchronize()
        assert log.counts.get("node_scatter_kernel", 0) == 1, (dx, log.counts)
        f_lg, f_ls, f_g = fresh[dx][:3]
        assert _bitwise(lg.cpu().numpy(), f_lg) and _bitwise(tr.losses.cpu().numpy(), f_ls), dx
        _compare(f"{'default' if dx else 'disable_node_dx'} in sequence", {n: (None if v is None else v.cpu().double().numpy()) for n, v in _trainer_grads(tr, clf).items()}, f_g)


def test_separate_tail_takes_the_token_walk():
    """loss_in_forward off: no dXs in the forward, so the token-walking body runs, at grade."""
    c = _c23()

    def nolif(tr):
        tr.loss_in_forward = False
    lg, ls, g, ran, (tr, _, xd) = _run(True, c["sd"], c["x"], c["y"], c["w"], dropout=False, prepare=nolif)
    assert {"node_scatter_kernel", "head_bwd_kernel"} <= ran and "tail_bwd64_kernel" not in ran, sorted(ran)
    assert _dxs_written(tr, *xd.shape)
    G.assert_grade("separate tail", G.grade(_got(lg, ls, g), c["ref"]))


def test_size_rule():
    """Below node_dx_shape (the value table's rule: a capacity of 64 table rows) the switch changes nothing: the dXs rows are written.
    hg38_1mb: 3 067 nodes; 4 096 rows of L = 5: capacity 20 481 >= 4 x 3 068 (node route), < 64 x 3 068."""
    _, _, sd = oracle_state(synth.LAYOUTS["hg38_1mb"], 64, "table", 72)
    x, y, w = G.make_case_batch("hg38_1mb", [2, 3, 4, 5], 1024, 572, 5)
    assert x.shape == (4096, 5) and 4 * 3068 <= 4096 * 5 + 1 < 64 * 3068
    out = {}
    for dx in (True, False):
        lg, ls, g, ran, (tr, _, xd) = _run(dx, sd, x, y, w, dropout=False, layout="hg38_1mb", seed=72)
        assert "node_scatter_kernel" in ran and _dxs_written(tr, *xd.shape), (dx, sorted(ran))
        out[dx] = (lg, ls, g, ran)
    assert _bitwise(out[True][0], out[False][0]) and _bitwise(out[True][1], out[False][1]) and out[True][3] == out[False][3]
    _compare("below the rule", out[True][2], out[False][2])


def test_graph_replay_equals_eager():
    from matcha_amd.engine import Trainer
    c = _c23()
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
    _no_dropout(clf)
    clf.train()
    tr = Trainer(clf, lr=1e-3, base_seed=11)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))

    def grads():
        return {n: (None if v is None else v.cpu().double().numpy()) for n, v in _trainer_grads(tr, clf).items()}
    with _lib.launch_log() as log:
        eager = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0).clone()
    torch.cuda.synchronize()
    assert log.counts.get("node_scatter_kernel", 0) == 1 and not _dxs_written(tr, *xd.shape), log.counts
    g_eager = grads()
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
    graph.replay()
    torch.cuda.synchronize()
    assert _bitwise(out.cpu().numpy(), eager.cpu().numpy())
    _compare("one replay against eager", grads(), g_eager)
