"""The value pass of fused_fwd32_kernel (fused_fwd32.hip; DESIGN.md 4.2, "y tile"): per head the kernel reads the keys' rows y_j = M_h x_hat_j from an
LDS tile and accumulates dyn_i += sum_j p_ij y_j + n_pad p_i,pad y_pad -- no M_h z product behind the attention.  A head's tile has three sources:
gathered from the per-node value table VN next to the r rows (the node route of a differentiated forward: node_r_kernel's V role wrote it for the
backward anyway), a product per token with the r rows gathered (the route without VN: disable_node_v, inference), or a second product per token
(the per-token route: disable_node_r, disable_node_front).  All three leave the same bits, so logits and both losses are BITWISE equal between the
four settings; the route record (matcha_route_read: `fwd_values`) says which source the forward took.

Shape: test_hip_node_v.py's (c23, 150 nodes, 3 072 mixed-k rows, L = 5: capacity 15 361 >= 64 x 151, the smallest that builds VN) and its helpers;
one batch of 2 048 rows at L = 8 for the ML = 8 instance.  GPU only (-m gpu).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from matcha_amd import synth, _lib
from tests import fp64_grade as G
from tests.helpers import logit_err
from tests.test_hip_bwd_waits import _batch as _waits_batch
from tests.test_hip_model import TOL, hip_model
from tests.test_hip_node_front import _bitwise, _c23, _eval_logits, _id_batch, _no_dropout
from tests.test_hip_node_v import SETTINGS, _batch as _v_batch, _run, _setting

pytestmark = pytest.mark.gpu

KINDS = ["mixed", "all_k2", "all_k5", "single", "pads_and_empty", "last_row", "five", "foreign", "l8"]
# StepRoute::fwd_values (layerwise.hpp): 1 a product per token, 2 a product per token with the r rows gathered, 3 gathered from VN
SOURCE = {"default": 3, "disable_node_v": 2, "disable_node_r": 1, "disable_node_front": 1}


def _batch(kind):
    """(state dict, front end, x, y, w).  single: ONE hyperedge of two nodes in 3 072 rows -- one half tile, 30 rows past its tokens; pads_and_empty: pads
    anywhere inside the rows, a run of all-padding rows and scattered ones (test_hip_bwd_waits.py); five: five ids hold every token."""
    c = _c23()
    if kind in ("single", "pads_and_empty"):
        x, y, w = _waits_batch(kind)
        return c["sd"], c["fe"], x, y, w
    if kind == "five":
        return c["sd"], c["fe"], _id_batch("five"), c["y"], c["w"]
    return _v_batch(kind)


def _all(setting):
    return (_setting(setting), _lib.option("disable_node_front")) if setting == "disable_node_front" else (_setting(setting),)


def _recorded_source(setting, sd, x, y, w):
    """One training forward through the C ABI under a setting, NO backward (which would consume the record): the record's value source."""
    from matcha_amd.engine import Trainer
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=sd)
    clf.train()
    ctx = _all(setting)
    for c_ in ctx:
        c_.__enter__()
    try:
        tr = Trainer(clf, lr=1e-3, base_seed=11)
        rt = tr.rt
        xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (x, y, w))
        B, L = xd.shape
        ws, logits = tr._buffers(B, L)
        opts = tr._opts(1.0, 0.001, 0)
        with _lib.launch_log() as log:
            _lib.check(tr.lib.matcha_forward(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(xd), B, L, _lib.ptr(yd),
                                             _lib.ptr(wd), _lib.ptr(logits), _lib.ptr(tr.losses), _lib.ptr(ws), ws.numel(), rt.stream()), "matcha_forward")
            torch.cuda.synchronize()
    finally:
        for c_ in reversed(ctx):
            c_.__exit__(None, None, None)
    assert log.counts.get("fused_fwd32_kernel", 0) == 1, log.counts
    rec = _lib.route_record(ws)
    assert rec["node_v"] == int(setting == "default") and rec["node_r"] == int(setting in ("default", "disable_node_v")), (setting, rec)
    assert rec["node"] == int(setting != "disable_node_front") and rec["fused"] == 1 and rec["small"] == 0, (setting, rec)
    return rec["fwd_values"]


@pytest.mark.parametrize("kind", KINDS)
def test_value_sources_agree(kind):
    sd, fe, x, y, w = _batch(kind)
    assert x.shape[0] * x.shape[1] + 1 >= 64 * 151
    for s in SETTINGS:
        assert _recorded_source(s, sd, x, y, w) == SOURCE[s], (kind, s)
    # dropout on: logits and both losses bitwise across the four settings
    out = {}
    for s in SETTINGS:
        lg, ls, _, tr = _run(s, sd, x, y, w, dropout=True)
        if kind == "foreign":
            with pytest.raises(IndexError):
                tr.check_status()
        else:
            tr.check_status()
        assert np.isfinite(lg).all() and np.isfinite(ls).all()
        out[s] = (lg, ls)
    for s in SETTINGS[1:]:
        assert _bitwise(out["default"][0], out[s][0]) and _bitwise(out["default"][1], out[s][1]), (kind, s, out["default"][1], out[s][1])
    # eval (a forward that keeps nothing: the route has no VN, so `default` runs the product with the r rows gathered)
    ev = {}
    if kind == "foreign":                                  # Classifier.forward reports the ids at once, as the reference's nn.Embedding does
        with pytest.raises(IndexError):
            _eval_logits("c23", sd, x, node=True)
    for s in SETTINGS if kind != "foreign" else ():
        with _setting(s):
            ev[s], cnt = _eval_logits("c23", sd, x, node=s != "disable_node_front")
        assert cnt.get("fused_fwd32_kernel", 0) == 1 and cnt.get("node_r_kernel", 0) == (1 if s in ("default", "disable_node_v") else 0), (s, cnt)
    for s in SETTINGS[1:] if ev else ():
        assert _bitwise(ev["default"], ev[s]), (kind, s)
    # dropout-free: the default's step at fp64 grade and within TOL of the oracle's logits
    lg, ls, g, _ = _run("default", sd, x, y, w, dropout=False)
    for s in SETTINGS[1:]:
        lg1, ls1, _, _ = _run(s, sd, x, y, w, dropout=False)
        assert _bitwise(lg, lg1) and _bitwise(ls, ls1), (kind, s)
    assert not ev or _bitwise(lg, ev["default"].reshape(-1))          # eval = the dropout-free training forward
    if kind != "foreign":
        ref = _c23()["ref"] if kind == "mixed" else G.references(sd, fe, x, y, w, chrom=0)
        got = G.StepOut(lg.astype(np.float64), {"bce": float(ls[0]), "recon": float(ls[1])}, g)
        G.assert_grade(f"{kind}: forward on the value table", G.grade(got, ref))
        err = logit_err(lg, ref.r64.logits)
        print(f"{kind}: logits against the fp64 oracle, element-wise {err:.2e} (bound {TOL:g})")
        assert err < TOL, (kind, err)
        assert abs(float(ls[0]) - ref.r64.losses["bce"]) < TOL * max(1.0, abs(ref.r64.losses["bce"])), (kind, ls, ref.r64.losses)


def _trainer(sd):
    from matcha_amd.engine import Trainer
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=sd)
    _no_dropout(clf)
    clf.train()
    return clf, Trainer(clf, lr=1e-3, base_seed=11)


def _source_of(tr, xd, yd, wd):
    """The value source of a training forward on THIS Trainer's workspace (no backward follows: it would consume the record)."""
    rt = tr.rt
    B, L = xd.shape
    ws, logits = tr._buffers(B, L)
    opts = tr._opts(1.0, 0.001, 0)
    _lib.check(tr.lib.matcha_forward(C.byref(rt.shape), C.byref(rt.params), C.byref(rt.frozen), C.byref(opts), _lib.ptr(xd), B, L, _lib.ptr(yd),
                                     _lib.ptr(wd), _lib.ptr(logits), _lib.ptr(tr.losses), _lib.ptr(ws), ws.numel(), rt.stream()), "matcha_forward")
    torch.cuda.synchronize()
    return _lib.route_record(ws)["fwd_values"]


def _status(tr, kind):
    if kind == "foreign":                                  # read as row 0 by every kernel, and still reported
        with pytest.raises(IndexError):
            tr.check_status()
    else:
        tr.check_status()


def _three_steps(kind, weights=None):
    """Three optimiser steps on a fresh model and Trainer: [(the weights the step ran on, its logits, its losses)].  ``weights``: the flat parameter
    buffer to run each step on, copied over in front of it (the Trainer's own AdamW state then no longer decides what the next forward sees)."""
    sd, _, x, y, w = _batch(kind)
    clf, tr = _trainer(sd)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (x, y, w))
    seen = []
    for step in range(3):
        if weights is not None:
            tr.rt.flat.copy_(weights[step])
        before = tr.rt.flat.clone()
        with _lib.launch_log() as log:
            tr.step(xd, yd, wd, 1.0, 0.001, 0)
            torch.cuda.synchronize()
        assert log.counts.get("node_r_kernel", 0) == 1 and log.counts.get("fused_fwd32_kernel", 0) == 1, log.counts
        seen.append((before, tr._buffers(*xd.shape)[1].cpu().numpy().copy(), tr.losses.cpu().numpy().copy()))
        assert np.isfinite(seen[-1][1]).all() and np.isfinite(seen[-1][2]).all()
    assert all(bool(torch.isfinite(p).all()) for p in clf.parameters())
    _status(tr, kind)
    assert _source_of(tr, xd, yd, wd) == 3                 # (behind the steps: this forward writes the workspace)
    return seen


@pytest.mark.parametrize("kind", KINDS)
def test_three_optimiser_steps_on_a_poisoned_workspace_equal_a_fresh_run(kind, monkeypatch):
    """A y tile, a bias row or a table row read before it is written shows up as NaN on the poisoned workspace, or as a difference to the clean one.
    The gradients are summed with float atomics, so two runs' weights part after the first update; the forward has none.  The clean run therefore
    takes, in front of each step, the weights the poisoned run had there: logits and losses of ALL three steps are then compared BITWISE."""
    monkeypatch.setenv("MATCHA_POISON_WS", "nan")
    poisoned = _three_steps(kind)
    monkeypatch.delenv("MATCHA_POISON_WS")
    clean = _three_steps(kind, weights=[p[0] for p in poisoned])
    assert not torch.equal(poisoned[0][0], poisoned[1][0]) and not torch.equal(poisoned[1][0], poisoned[2][0])      # the weights did move
    assert not _bitwise(poisoned[0][1], poisoned[1][1]) and not _bitwise(poisoned[1][1], poisoned[2][1])
    for step in range(3):
        assert torch.equal(clean[step][0], poisoned[step][0])
        assert _bitwise(clean[step][1], poisoned[step][1]) and _bitwise(clean[step][2], poisoned[step][2]), (kind, step, clean[step][2], poisoned[step][2])


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_equals_eager(kind):
    sd, _, x, y, w = _batch(kind)
    clf, tr = _trainer(sd)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (x, y, w))
    with _lib.launch_log() as log:
        eager = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0).clone()
    assert log.counts.get("node_r_kernel", 0) == 1 and log.counts.get("fused_fwd32_kernel", 0) == 1, log.counts
    eager_ls = tr.losses.clone()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), _lib.launch_log() as log:
        out = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
    assert log.counts.get("node_r_kernel", 0) == 1 and log.counts.get("fused_fwd32_kernel", 0) == 1, log.counts      # (a graph counts at capture)
    for _ in range(2):
        out.zero_()
        tr.losses.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _bitwise(out.cpu().numpy(), eager.cpu().numpy()) and _bitwise(tr.losses.cpu().numpy(), eager_ls.cpu().numpy()), kind
    _status(tr, kind)
    assert _source_of(tr, xd, yd, wd) == 3


@pytest.mark.parametrize("kind", KINDS)
def test_sequences_on_one_workspace(kind):
    """default, disable_node_v, default on ONE Trainer (one workspace: VN written, left stale, written again) equal fresh runs bitwise."""
    sd, _, x, y, w = _batch(kind)
    fresh = {s: _run(s, sd, x, y, w, dropout=False) for s in SETTINGS[:2]}
    clf, tr = _trainer(sd)
    xd, yd, wd = (torch.from_numpy(a).cuda().contiguous() for a in (x, y, w))
    for s in ("default", "disable_node_v", "default"):
        tr.gflat.zero_()
        with _setting(s), _lib.launch_log() as log:
            lg = tr.forward_backward(xd, yd, wd, 1.0, 0.001, 0)
            torch.cuda.synchronize()
            lg, ls = lg.cpu().numpy().copy(), tr.losses.cpu().numpy().copy()
            assert _source_of(tr, xd, yd, wd) == SOURCE[s], (kind, s)            # (behind the step, under the same setting; it overwrites logits and losses)
        assert log.counts.get("node_r_kernel", 0) == 2 and log.counts.get("fused_fwd32_kernel", 0) == 2, (s, log.counts)      # the step + the record's forward
        assert _bitwise(lg, fresh[s][0]) and _bitwise(ls, fresh[s][1]), (kind, s)
    _status(tr, kind)
