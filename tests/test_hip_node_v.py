"""The value table of the node route (fused_fwd32.hip: node_r_kernel's V role; fused_bwd.hip: fused_bwdh_kernel<ML, true, true>; DESIGN.md
4.3): a differentiated forward on the route also writes y = M_h x_hat per (node, head), and the backward gathers the rows -- d_j = dDyn_i . y_j,
d x_hat = [dR | U] [B_h ; M_h] + GK, dM_h = U^T x_hat + u_pad (x) x_hat_pad -- instead of forming dZ = dDyn M_h and Z per token.  Against the
same route without the table (option disable_node_v), with r rows per token (disable_node_r) and against the per-token route
(disable_node_front): the forward does not change, so logits and losses are compared BITWISE; the backward computes the same gradients in another
association, so it is held to fp64 grade (tests/fp64_grade.py, K = 8) and to the repository's route-against-route bound, 2e-5 of each tensor's
largest element.  The table is built from a capacity of 64 table rows on (node_v_shape; test_size_rule).  Shape: test_hip_node_r.py's (c23,
150 nodes, 3 072 mixed-k rows, L = 5), its helpers re-used; one L = 8 batch of 2 048 rows for the ML = 8 instance.  GPU only (-m gpu).
"""
import contextlib

import numpy as np
import pytest
import torch

from matcha_amd import synth, _lib
from tests import fp64_grade as G
from tests.helpers import oracle_state
from tests.test_hip_model import hip_model, _trainer_grads
from tests.test_hip_node_front import _bitwise, _c23, _eval_logits, _id_batch, _no_dropout, _step
from tests.test_hip_node_r import _close, _ids as _r_ids

pytestmark = pytest.mark.gpu

SETTINGS = ("default", "disable_node_v", "disable_node_r", "disable_node_front")


def _setting(name):
    return _lib.option(name) if name in ("disable_node_v", "disable_node_r") else contextlib.nullcontext()


def _run(name, sd, x, y, w, *, dropout):
    """One step under a setting; the launch log says which tables the forward built: node_r_kernel ONCE (forward only: the backward
    rebuilds no table) with the r table, never without."""
    from matcha_amd.engine import Trainer
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=sd)
    if not dropout:
        _no_dropout(clf)
    clf.train()
    with _setting(name), (_lib.option("disable_node_front") if name == "disable_node_front" else contextlib.nullcontext()):
        tr = Trainer(clf, lr=1e-3, base_seed=11)
        xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (x, y, w))
        with _lib.launch_log() as log:
            logits = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
            torch.cuda.synchronize()
    cnt = log.counts
    assert cnt.get("node_r_kernel", 0) == (1 if name in ("default", "disable_node_v") else 0), (name, cnt)
    assert cnt.get("node_scatter_kernel", 0) == (0 if name == "disable_node_front" else 1), (name, cnt)
    assert cnt.get("fused_fwd32_kernel", 0) == 1 and cnt.get("fused_bwdh_kernel", 0) == 1, (name, cnt)
    grads = {n: (None if v is None else v.cpu().double().numpy()) for n, v in _trainer_grads(tr, clf).items()}
    return logits.cpu().numpy().copy(), tr.losses.cpu().numpy().copy(), grads, tr


_L8 = {}


def _l8():
    """c23, 2 048 rows of k in {2..8} at L = 8: capacity 16 385 >= 4 x 151 and 683 half tiles (the large-batch kernels), instance ML = 8."""
    if not _L8:
        _, fe, sd = oracle_state(synth.LAYOUTS["c23"], 64, "table", 71)
        x, y, w = G.make_case_batch("c23", [2, 3, 4, 5, 6, 7, 8, 8], 256, 577, 8)
        assert x.shape == (2048, 8) and {int(k) for k in (x != 0).sum(1)} == set(range(2, 9))
        _L8.update(sd=sd, fe=fe, x=x, y=y, w=w)
    return _L8


def _batch(kind):
    c = _c23()
    if kind == "mixed":
        return c["sd"], c["fe"], c["x"], c["y"], c["w"]
    if kind == "all_k2":                                   # n_pad = 3 in every row: both padding terms at their largest
        x, y, w = G.make_case_batch("c23", [2], 3072, 576, 5)
        assert x.shape == (3072, 5) and ((x != 0).sum(1) == 2).all()
        return c["sd"], c["fe"], x, y, w
    if kind == "l8":
        d = _l8()
        return d["sd"], d["fe"], d["x"], d["y"], d["w"]
    if kind == "foreign":
        return c["sd"], c["fe"], _id_batch("foreign"), c["y"], c["w"]
    x, y, w = _r_ids(kind)                                 # all_k5 (no padding key anywhere), last_row (node 150: the table's last row)
    return c["sd"], c["fe"], x, y, w


def test_forward_is_bitwise_the_same_in_the_four_settings():
    c = _c23()
    out = {s: _run(s, c["sd"], c["x"], c["y"], c["w"], dropout=True) for s in SETTINGS}
    for s in SETTINGS[1:]:
        assert _bitwise(out["default"][0], out[s][0]), s
        assert _bitwise(out["default"][1], out[s][1]), (s, out["default"][1], out[s][1])
    ev = {}
    for s in SETTINGS:
        with _setting(s):
            ev[s], cnt = _eval_logits("c23", c["sd"], c["x"], node=s != "disable_node_front")
        assert cnt.get("node_r_kernel", 0) == (1 if s in ("default", "disable_node_v") else 0), (s, cnt)
        assert cnt.get("fused_fwd32_kernel", 0) == 1, (s, cnt)
    for s in SETTINGS[1:]:
        assert _bitwise(ev["default"], ev[s]), s


@pytest.mark.parametrize("kind", ["mixed", "all_k5", "all_k2", "last_row", "foreign", "l8"])
def test_gradients(kind):
    """Per batch: the forward bitwise in all four settings (dropout on); dropout-free, the default's gradients at fp64 grade (where the oracle
    takes the batch: not the foreign ids) and within 2e-5 of each tensor's largest element of disable_node_v's."""
    sd, fe, x, y, w = _batch(kind)
    out = {}
    for s in SETTINGS:
        lg, ls, _, tr = _run(s, sd, x, y, w, dropout=True)
        if kind == "foreign":
            with pytest.raises(IndexError):
                tr.check_status()
        else:
            tr.check_status()
        assert np.isfinite(lg).all()
        out[s] = (lg, ls)
    for s in SETTINGS[1:]:
        assert _bitwise(out["default"][0], out[s][0]) and _bitwise(out["default"][1], out[s][1]), (kind, s)
    lg, ls, g, _ = _run("default", sd, x, y, w, dropout=False)
    lg1, ls1, g1, _ = _run("disable_node_v", sd, x, y, w, dropout=False)
    assert _bitwise(lg, lg1) and _bitwise(ls, ls1)
    if kind != "foreign":
        ref = _c23()["ref"] if kind == "mixed" else G.references(sd, fe, x, y, w, chrom=0)
        got = G.StepOut(lg.astype(np.float64), {"bce": float(ls[0]), "recon": float(ls[1])}, g)
        G.assert_grade(f"{kind}: node route with the value table", G.grade(got, ref))
    _close(f"{kind}: value table against dZ per token", g, g1)


def test_size_rule():
    """model.hip node_v_shape: the value table is built from a token capacity of 64 table rows on (below it the A/B against the parent's library
    showed no gain).  The instance has the other one's name in the launch log; what tells them apart is the rounding of the encoder's own
    gradients: with the same kernels (below the rule) default and disable_node_v agree BITWISE there -- the heads' float atomics reach only
    the front end's gradients --, with the value table (c23: capacity 15 361 >= 64 x 151) they are equal to rounding and not bitwise."""
    enc = ("encode1.mul_head_attn.w_qs.weight", "encode1.mul_head_attn.w_ks.weight", "encode1.mul_head_attn.w_vs.weight", "encode1.mul_head_attn.fc1.weight")

    def pair(layout, sd, x, y, w):
        out = []
        for name in ("default", "disable_node_v"):
            with _setting(name):
                lg, ls, g, ran, _ = _step(layout, sd, x, y, w, node=True, dropout=False, seed=72)
            assert {"node_r_kernel", "node_scatter_kernel", "fused_bwdh_kernel"} <= ran, sorted(ran)
            out.append((lg, ls, g))
        assert _bitwise(out[0][0], out[1][0]) and _bitwise(out[0][1], out[1][1])
        return [bool(np.array_equal(out[0][2][n], out[1][2][n])) for n in enc]

    # hg38_1mb: 3 067 nodes; 4 096 rows of L = 5: capacity 20 481 >= 4 x 3 068 (node route), < 64 x 3 068 (no value table)
    _, _, sd = oracle_state(synth.LAYOUTS["hg38_1mb"], 64, "table", 72)
    x, y, w = G.make_case_batch("hg38_1mb", [2, 3, 4, 5], 1024, 572, 5)
    assert x.shape == (4096, 5) and 4 * 3068 <= 4096 * 5 + 1 < 64 * 3068
    assert all(pair("hg38_1mb", sd, x, y, w))
    c = _c23()
    assert c["x"].shape[0] * 5 + 1 >= 64 * 151
    assert not any(pair("c23", c["sd"], c["x"], c["y"], c["w"]))


def test_tables_are_rebuilt_from_the_current_weights(monkeypatch):
    """Three optimiser steps on one Trainer whose workspace starts as NaN: finite losses and logits that move.  A value table left over from
    other weights, read before it is written, or an LDS region the instance reads past what it staged cannot pass."""
    from matcha_amd.engine import Trainer
    monkeypatch.setenv("MATCHA_POISON_WS", "nan")
    c = _c23()
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
    clf.train()
    tr = Trainer(clf, lr=1e-3, base_seed=11)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))
    seen = []
    for _ in range(3):
        with _lib.launch_log() as log:
            tr.step(xd, yd, wd, 1.0, 0.001, 0)
            torch.cuda.synchronize()
        assert log.counts.get("node_r_kernel", 0) == 1 and log.counts.get("fused_bwdh_kernel", 0) == 1, log.counts
        assert np.isfinite(tr.losses.cpu().numpy()).all()
        assert all(bool(torch.isfinite(p).all()) for p in clf.parameters())
        clf.eval()
        with torch.no_grad():
            seen.append(clf(xd).cpu().numpy().copy())
        clf.train()
        assert np.isfinite(seen[-1]).all()
    assert not _bitwise(seen[0], seen[1]) and not _bitwise(seen[1], seen[2])      # the weights did move


def test_sequences_on_one_workspace():
    """default, disable_node_v, default on ONE Trainer (one workspace, gradients re-zeroed in between) equal fresh runs."""
    from matcha_amd.engine import Trainer
    c = _c23()
    fresh = {s: _run(s, c["sd"], c["x"], c["y"], c["w"], dropout=False) for s in SETTINGS[:2]}
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
    _no_dropout(clf)
    clf.train()
    tr = Trainer(clf, lr=1e-3, base_seed=11)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))
    for s in ("default", "disable_node_v", "default"):
        tr.gflat.zero_()
        with _setting(s), _lib.launch_log() as log:
            lg = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
            torch.cuda.synchronize()
        assert log.counts.get("node_r_kernel", 0) == 1, (s, log.counts)
        f_lg, f_ls, f_g, _ = fresh[s]
        assert _bitwise(lg.cpu().numpy(), f_lg) and _bitwise(tr.losses.cpu().numpy(), f_ls), s
        _close(f"{s} in sequence", {n: (None if v is None else v.cpu().double().numpy()) for n, v in _trainer_grads(tr, clf).items()}, f_g)


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
    assert log.counts.get("node_r_kernel", 0) == 1 and log.counts.get("node_scatter_kernel", 0) == 1, log.counts
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _bitwise(out.cpu().numpy(), eager.cpu().numpy())
