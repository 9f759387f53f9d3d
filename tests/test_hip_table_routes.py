"""The autograd path over the three routes of the d = 64 table front end, with the switches flipped BETWEEN model(x) and loss.backward().

matcha_forward and matcha_backward are two calls there, and the options (disable_node_r, disable_node_front) are process-wide, so the backward
must follow what the forward recorded for its workspace (model.hip: StepRoute::node and ::node_r in g_fwd_state), not the option table it finds: a backward that
believed the options would gather r rows nobody wrote, read X from the wrong table or run the front end's backward over the wrong rows.
All six ordered pairs of {default, disable_node_r, disable_node_front}, each against the un-flipped run of the forward's setting (logits and
losses bitwise, gradients to the repository's route-against-route bound) and against the fp64 oracle at fp32 grade (tests/fp64_grade.py, K = 8).
The workspace model(x) takes starts as NaN, so a row nobody wrote on the recorded route cannot pass.  Shape: the c23 batch of
tests/test_hip_node_front.py (3 072 rows; the grading of every route at the larger shapes is tests/test_hip_fp64_grade.py's).  GPU only (-m gpu).
"""
import contextlib
import itertools

import numpy as np
import pytest
import torch

from matcha_amd import synth, _lib
from tests import fp64_grade as G
from tests.test_hip_model import hip_model
from tests.test_hip_node_front import _bitwise, _c23, _no_dropout
from tests.test_hip_node_r import SETTINGS, _close

pytestmark = pytest.mark.gpu

_NODE_ROUTE = {"default": True, "disable_node_r": True, "disable_node_front": False}      # the forward's setting -> the front end ran per node


@pytest.fixture(autouse=True)
def _poisoned_workspace(monkeypatch):
    monkeypatch.setenv("MATCHA_POISON_WS", "nan")


def _ctx(setting):
    return contextlib.nullcontext() if setting == "default" else _lib.option(setting)


def _ran(log):
    return {k for k, n in log.counts.items() if n > 0}


def _forward_backward(fwd, bwd):
    """model(x) in train mode (dropout off) under ``fwd``, loss = bce + 0.001 recon as the oracle's step, loss.backward() under ``bwd``.
    Returns (logits, [bce, recon], gradients by name, kernels of the forward call, kernels of the backward call)."""
    c = _c23()
    clf, _ = hip_model(synth.LAYOUTS["c23"], 64, "table", 0, sd=c["sd"])
    _no_dropout(clf)
    clf.train()
    ws = clf._runtime().workspace(4, 5)
    assert bool((ws == 0xFF).all()), "the workspaces model(x) takes are not poisoned"
    xd = torch.from_numpy(c["x"]).cuda().contiguous()
    yd = torch.from_numpy(c["y"]).cuda().reshape(-1, 1)
    wd = torch.from_numpy(c["w"]).cuda().reshape(-1, 1)
    with _ctx(fwd), _lib.launch_log() as log_f:
        lg, rc = clf(xd, return_recon=True)
        bce = torch.nn.functional.binary_cross_entropy_with_logits(lg, yd, weight=wd)
        loss = bce * 1.0 + rc.sum() * 0.001
        torch.cuda.synchronize()
    with _ctx(bwd), _lib.launch_log() as log_b:
        loss.backward()
        torch.cuda.synchronize()
    grads = {n: (None if p.grad is None else p.grad.cpu().double().numpy()) for n, p in clf.named_parameters()}
    losses = np.array([float(bce.detach()), float(rc.detach().sum())], dtype=np.float32)
    return lg.detach().reshape(-1).cpu().numpy().copy(), losses, grads, _ran(log_f), _ran(log_b)


def _check_kernels(fwd, ran_f, ran_b):
    """The forward ran the route of ITS setting; the backward ran the route the forward recorded, whatever the options said by then."""
    node = _NODE_ROUTE[fwd]
    assert {"front_fwd3_kernel", "fused_fwd32_kernel"} <= ran_f, sorted(ran_f)
    assert ("node_xhat_kernel" in ran_f) == node and ("node_r_kernel" in ran_f) == (fwd == "default"), (fwd, sorted(ran_f))
    assert {"head_bwd_kernel", "fused_bwdh_kernel", "front_bwd_kernel"} <= ran_b, sorted(ran_b)      # no y / w in matcha_forward: the separate tail
    assert ("node_scatter_kernel" in ran_b) == node, (fwd, sorted(ran_b))
    assert not ({"node_r_kernel", "node_xhat_kernel", "front_fwd3_kernel"} & ran_b), sorted(ran_b)     # the backward rebuilds no table


def _graded(label, lg, grads):
    # (the bce of this path is torch's own reduction of the logits, not a kernel of the library: the logits and every gradient are graded)
    G.assert_grade(label, G.grade(G.StepOut(lg.astype(np.float64), {}, grads), _c23()["ref"]))


_PLAIN = {}


def _plain(setting):
    """The un-flipped run of a setting: forward and backward under it.  Computed once, itself held to the kernel sets and the oracle."""
    if setting not in _PLAIN:
        lg, ls, grads, ran_f, ran_b = _forward_backward(setting, setting)
        _check_kernels(setting, ran_f, ran_b)
        _graded(f"autograd, {setting}", lg, grads)
        _PLAIN[setting] = (lg, ls, grads)
    return _PLAIN[setting]


def test_the_autograd_path_takes_each_route():
    """All three routes are reachable through model(x) + backward(), and their forwards are bitwise the same function."""
    out = {s: _plain(s) for s in SETTINGS}
    for s in SETTINGS[1:]:
        assert _bitwise(out["default"][0], out[s][0]) and _bitwise(out["default"][1], out[s][1]), s


@pytest.mark.parametrize("fwd,bwd", list(itertools.permutations(SETTINGS, 2)))
def test_backward_follows_the_forwards_record(fwd, bwd):
    want_lg, want_ls, want_g = _plain(fwd)
    lg, ls, grads, ran_f, ran_b = _forward_backward(fwd, bwd)
    _check_kernels(fwd, ran_f, ran_b)
    assert _bitwise(lg, want_lg) and _bitwise(ls, want_ls), (fwd, bwd, ls, want_ls)
    assert all(np.isfinite(g).all() for g in grads.values() if g is not None), (fwd, bwd)
    _close(f"forward {fwd}, backward {bwd}", grads, want_g)
    _graded(f"forward {fwd}, backward {bwd}", lg, grads)
