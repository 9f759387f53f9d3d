"""The r table of the node route (fused_fwd32.hip: node_r_kernel): r = B_h x_hat + b_h once per (node, head), gathered by
both encoder kernels, against the same route with the rows computed per token (option disable_node_r) and against the per-token route
(disable_node_front).  The forward is the same function evaluated from the same bits -- an MFMA output column depends on the same column of
the token-side operand only -- so logits and losses are compared BITWISE; the backward reads the same r rows from another place and differs
in the order of its float atomics only: fp64 grade (tests/fp64_grade.py, K = 8) and the repository's route-against-route bound, 2e-5 of the
tensor's largest element.  Shape: the smallest node-route case of tests/test_hip_node_front.py (c23, 150 nodes, 3 072 mixed-k rows, L = 5).
GPU only (-m gpu).
"""
import contextlib

import numpy as np
import pytest
import torch

from matcha_amd import synth, _lib
from tests import fp64_grade as G
from tests.test_hip_model import hip_model, _trainer_grads
from tests.test_hip_node_front import _bitwise, _c23, _eval_logits, _id_batch, _no_dropout, _step

pytestmark = pytest.mark.gpu

SETTINGS = ("default", "disable_node_r", "disable_node_front")


def _setting(name):
    """Context of one of the three settings; the helpers of test_hip_node_front take ``node`` (False = disable_node_front)."""
    return _lib.option("disable_node_r") if name == "disable_node_r" else contextlib.nullcontext()


def _run(name, x, y, w, *, dropout):
    c = _c23()
    with _setting(name):
        lg, ls, g, ran, keep = _step("c23", c["sd"], x, y, w, node=name != "disable_node_front", dropout=dropout)
    assert ("node_r_kernel" in ran) == (name == "default"), (name, sorted(ran))
    assert ("node_scatter_kernel" in ran) == (name != "disable_node_front"), (name, sorted(ran))
    assert {"fused_fwd32_kernel", "fused_bwdh_kernel"} <= ran, sorted(ran)
    return lg, ls, g, keep


def _close(label, got, want):
    """route against route: 2e-5 of the tensor's largest element, the gauge parameter (true gradient 0) excluded"""
    for n, b in want.items():
        a = got[n]
        assert (a is None) == (b is None), (label, n)
        if b is None or n == G.GAUGE:
            continue
        err, top = float(np.abs(a - b).max()), float(np.abs(b).max())
        print(f"{label} {n}: max |diff| {err:.3e}, largest element {top:.3e}")
        assert err <= 2e-5 * top + 1e-9, (label, n, err, top)


def test_forward_is_bitwise_the_same_in_the_three_settings():
    c = _c23()
    out = {s: _run(s, c["x"], c["y"], c["w"], dropout=True) for s in SETTINGS}
    for s in SETTINGS[1:]:
        assert _bitwise(out["default"][0], out[s][0]), s
        assert _bitwise(out["default"][1], out[s][1]), (s, out["default"][1], out[s][1])
    ev = {}
    for s in SETTINGS:
        with _setting(s):
            ev[s], cnt = _eval_logits("c23", c["sd"], c["x"], node=s != "disable_node_front")
        assert cnt.get("node_r_kernel", 0) == (1 if s == "default" else 0), (s, cnt)     # the inference forward takes the table too
        assert cnt.get("fused_fwd32_kernel", 0) == 1, (s, cnt)
    for s in SETTINGS[1:]:
        assert _bitwise(ev["default"], ev[s]), s


def test_gradients_at_fp64_grade_and_against_the_per_token_rows():
    c = _c23()
    lg, ls, g, _ = _run("default", c["x"], c["y"], c["w"], dropout=False)
    got = G.StepOut(lg.astype(np.float64), {"bce": float(ls[0]), "recon": float(ls[1])}, g)
    G.assert_grade("node route with the r table", G.grade(got, c["ref"]))
    lg1, ls1, g1, _ = _run("disable_node_r", c["x"], c["y"], c["w"], dropout=False)
    assert _bitwise(lg, lg1) and _bitwise(ls, ls1)
    _close("r table against per-token r", g, g1)


def _ids(kind):
    c = _c23()
    if kind in ("five", "few", "foreign"):
        return _id_batch(kind), c["y"], c["w"]
    if kind == "all_k5":                                   # every row full: no padding key anywhere in the batch
        x, y, w = G.make_case_batch("c23", [5], 3072, 574, 5)
        assert x.shape == (3072, 5) and (x != 0).all()
        return x, y, w
    assert kind == "last_row"                              # node 150 = row n_nodes of the table, the last one
    rng = np.random.default_rng(575)
    x = c["x"].copy()
    for i in rng.choice(len(x), size=400, replace=False):
        k = int((x[i] != 0).sum())
        if 150 not in x[i]:
            x[i, k - 1] = 150                              # the largest id: the row stays sorted
    assert int((x == 150).sum()) >= 400 and x.max() == 150
    return x, c["y"], c["w"]


@pytest.mark.parametrize("kind", ["five", "few", "foreign", "all_k5", "last_row"])
def test_ids(kind):
    x, y, w = _ids(kind)
    out = {}
    for s in SETTINGS:
        lg, ls, _, (tr, _, _) = _run(s, x, y, w, dropout=True)
        if kind == "foreign":                              # read as row 0 by every kernel, and still reported
            with pytest.raises(IndexError):
                tr.check_status()
        else:
            tr.check_status()
        assert np.isfinite(lg).all()
        out[s] = (lg, ls)
    for s in SETTINGS[1:]:
        assert _bitwise(out["default"][0], out[s][0]) and _bitwise(out["default"][1], out[s][1]), (kind, s)
    lg, ls, g, _ = _run("default", x, y, w, dropout=False)
    lg1, ls1, g1, _ = _run("disable_node_r", x, y, w, dropout=False)
    assert _bitwise(lg, lg1) and _bitwise(ls, ls1)
    _close(f"{kind}: r table against per-token r", g, g1)


def test_table_is_rebuilt_from_the_current_weights(monkeypatch):
    """Three optimiser steps on one Trainer whose workspace starts as NaN; after each, the SAME model's inference logits with the table and
    with per-token r rows are bit-equal -- a table left over from other weights, or never written, cannot pass."""
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
        assert log.counts.get("node_r_kernel", 0) == 1, log.counts
        clf.eval()
        ev = {}
        for s in SETTINGS[:2]:
            with _setting(s), _lib.launch_log() as log, torch.no_grad():
                ev[s] = clf(xd).cpu().numpy().copy()
            assert log.counts.get("node_r_kernel", 0) == (1 if s == "default" else 0), (s, log.counts)
        clf.train()
        assert np.isfinite(ev["default"]).all()
        assert _bitwise(ev["default"], ev["disable_node_r"])
        seen.append(ev["default"])
    assert not _bitwise(seen[0], seen[1]) and not _bitwise(seen[1], seen[2])      # the weights did move


def test_sequences_on_one_workspace():
    """default, disable_node_r, default on ONE Trainer (one workspace, gradients re-zeroed in between) equal three fresh runs."""
    from matcha_amd.engine import Trainer
    c = _c23()
    fresh = {s: _run(s, c["x"], c["y"], c["w"], dropout=False) for s in SETTINGS[:2]}
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
    _no_dropout(clf)
    clf.train()
    tr = Trainer(clf, lr=1e-3, base_seed=11)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (c["x"], c["y"], c["w"]))
    for s in ("default", "disable_node_r", "default"):
        tr.gflat.zero_()
        with _setting(s), _lib.launch_log() as log:
            lg = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
            torch.cuda.synchronize()
        assert (log.counts.get("node_r_kernel", 0) > 0) == (s == "default"), (s, log.counts)
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
