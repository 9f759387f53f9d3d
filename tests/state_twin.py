"""Veterans and fresh twins: the machinery of tests/test_hip_state.py.

A *veteran* is a model / Trainer that has been through earlier calls.  The *fresh twin* of one call is a newly constructed Classifier
(+ Trainer) loaded with exactly the state the veteran had immediately before that call -- ``state_dict()`` values, the frozen attribute
table, on the adj front end the feature blocks and inter_initial, the runtime's autograd seed counter, and for a Trainer ``exp_avg``,
``exp_avg_sq``, ``seg_step`` and the value of the seed cell -- which then makes that one call.  A call's result must depend on its
inputs only, so veteran and twin agree: bitwise wherever the suite already asserts run-to-run bitwise reproducibility, and against the
oracle (tests/fp64_grade.py, or the 1e-4 parity with the kernels' dropout masks injected) where gradients go through float atomics.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from matcha_amd import synth, _lib
from oracle import hypersagnn as O
from oracle import rng as R
from tests import fp64_grade as G
from tests.helpers import logit_err

TOL = 1e-4                                            # the north star of tests/test_hip_model.py
FRONT = ("node_embedding.", "next_w.", "attribute_nn.")      # what lies in front of the encoder (test_full_size_train_step_is_reproducible)


@dataclass(frozen=True)
class Config:
    mode: str
    d: int
    layout: str
    seed: int
    deterministic: bool = True

    @property
    def num(self):
        return synth.LAYOUTS[self.layout]

    @property
    def n_nodes(self):
        return int(np.sum(self.num))

    def bitwise_tensor(self, name: str) -> bool:
        """Whether gradient / post-AdamW parameter ``name`` is bitwise reproducible from run to run, as the suite already asserts: the
        table front end with deterministic=True at embed_dim 64 (test_full_size_train_step_is_reproducible) and 16
        (test_graph_replayed_epoch_equals_the_step_by_step_epoch) entirely; with the default float atomics everything behind the front end
        (same test); nothing on the adj front end and in the embed_dim-128 attention block (float atomics in their weight gradients)."""
        if self.mode != "table" or self.d not in (16, 64):
            return False
        return self.deterministic or not name.startswith(FRONT)


def other_num(num):
    """A layout with the length and sum of ``num`` but other boundaries and another num[0]."""
    num = list(num)
    if num[::-1] != num:
        return num[::-1]
    q = num[0] // 4
    return [num[0] - q, num[1] + q] + num[2:]


# ---------------------------------------------------------------------------------------------------------------------------------
# state of a model / a Trainer, and twins built from it
# ---------------------------------------------------------------------------------------------------------------------------------
def _dropouts(clf):
    return [m for m in clf.modules() if isinstance(m, torch.nn.Dropout)]


def model_state(clf) -> dict:
    rt = clf.__dict__.get("_rt")
    ne = clf.node_embedding
    st = dict(sd={k: v.detach().clone() for k, v in clf.state_dict().items()}, training=clf.training, drop=[m.p for m in _dropouts(clf)],
              seed_counter=0 if rt is None else rt.seed_counter)
    if hasattr(ne, "embeddings"):
        st["feats"] = [e.embedding.detach().clone() for e in ne.embeddings]
        st["inter"] = ne.inter_initial.embedding.detach().clone()
    return st


def fresh_model(cfg: Config, st: dict):
    from tests.test_hip_model import hip_model
    clf, _ = hip_model(cfg.num, cfg.d, cfg.mode, cfg.seed, sd={k: v.cpu().numpy() for k, v in st["sd"].items()})
    if "feats" in st:
        ne = clf.node_embedding
        for e, f in zip(ne.embeddings, st["feats"]):
            e.embedding = f.clone()
        ne.inter_initial.embedding = st["inter"].clone()
    for m, p in zip(_dropouts(clf), st["drop"]):
        m.p = p
    clf.train(st["training"])
    clf._runtime().seed_counter = st["seed_counter"]
    return clf


def trainer_state(tr) -> dict:
    return dict(exp_avg=tr.exp_avg.clone(), exp_avg_sq=tr.exp_avg_sq.clone(), seg_step=tr.seg_step.clone(), seed=tr.seed.clone(),
                deterministic=tr.deterministic, loss_in_forward=tr.loss_in_forward, lr=tr.lr)


def load_trainer_state(tr, st: dict):
    tr.exp_avg.copy_(st["exp_avg"])
    tr.exp_avg_sq.copy_(st["exp_avg_sq"])
    tr.seg_step.copy_(st["seg_step"])
    tr.seed.copy_(st["seed"])
    tr.loss_in_forward = st["loss_in_forward"]


def fresh_trainer(clf, st: dict):
    from matcha_amd.engine import Trainer
    tr = Trainer(clf, lr=st["lr"], deterministic=st["deterministic"])
    load_trainer_state(tr, st)
    return tr


def set_dropout(clf, ps):
    """Set every Dropout.p (one value, or a list in modules() order); returns the previous values."""
    old = [m.p for m in _dropouts(clf)]
    for i, m in enumerate(_dropouts(clf)):
        m.p = ps[i] if isinstance(ps, (list, tuple)) else ps
    return old


# ---------------------------------------------------------------------------------------------------------------------------------
# calls: each returns {name: tensor} (clones); "grad/<tensor>" and "param/<tensor>" are compared by Config.bitwise_tensor
# ---------------------------------------------------------------------------------------------------------------------------------
def dev_batch(x, y, w):
    return (torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.ascontiguousarray(y).reshape(-1)).cuda(),
            torch.from_numpy(np.ascontiguousarray(w).reshape(-1)).cuda())


def trainer_grads(tr, clf) -> Dict[str, Optional[torch.Tensor]]:
    from tests.test_hip_model import _trainer_grads
    return _trainer_grads(tr, clf)


def train_call(clf, tr, batch, alpha=1.0, beta=0.001, chrom=0, optimizer=True) -> dict:
    """One Trainer step taken apart: forward_backward, the gradients read before AdamW zeroes them, optimizer_step."""
    x, y, w = batch
    logits = tr.forward_backward(x.contiguous(), y.contiguous(), w.contiguous(), alpha, beta, chrom)
    out = {"logits": logits.clone(), "losses": tr.losses.clone()}
    for n, g in trainer_grads(tr, clf).items():
        out["grad/" + n] = g
    if optimizer:
        tr.all_reduce()
        tr.optimizer_step()
        for n, p in clf.named_parameters():
            out["param/" + n] = p.detach().clone()
        out["seg_step"] = tr.seg_step.clone()
    torch.cuda.synchronize()
    return out


def eval_call(clf, x) -> dict:
    was = clf.training
    clf.eval()
    with torch.no_grad():
        out = {"logits": clf(x).reshape(-1).clone()}
    clf.train(was)
    torch.cuda.synchronize()
    return out


def autograd_call(clf, x, weight=None) -> dict:
    """model(x) with grad enabled, a backward through sum(logits * weight), p.grad of every live parameter (None = not reached)."""
    for p in clf.parameters():
        p.grad = None
    lg = clf(x)
    wv = torch.ones_like(lg) if weight is None else weight.reshape(lg.shape)
    (lg * wv).sum().backward()
    out = {"logits": lg.detach().reshape(-1).clone()}
    live = {id(p) for p in clf._runtime().live}
    for n, p in clf.named_parameters():
        if id(p) in live:
            out["grad/" + n] = None if p.grad is None else p.grad.detach().clone()
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------------------
def first_difference(a: dict, b: dict, cfg: Config, everything=False):
    """The first name (in a's order) whose tensors differ bitwise, among those that must agree bitwise under ``cfg`` (all of them with
    ``everything``); None when none does.  A gradient that is None on one side only always differs."""
    assert a.keys() == b.keys(), sorted(a.keys() ^ b.keys())
    for name, va in a.items():
        vb = b[name]
        if (va is None) != (vb is None):
            return name + " (None on one side only)"
        if va is None:
            continue
        if "/" in name and not everything and not cfg.bitwise_tensor(name.split("/", 1)[1]):
            continue
        if not torch.equal(va, vb):
            d = (va.double() - vb.double()).abs()
            return (f"{name} (max |diff| {float(d.max()):.3e} at max |twin| {float(vb.double().abs().max()):.3e}, "
                    f"{int((d > 0).sum())} of {d.numel()} elements differ)")
    return None


def assert_twin(label, veteran: dict, twin: dict, cfg: Config, everything=False):
    diff = first_difference(veteran, twin, cfg, everything)
    assert diff is None, f"{label}: the veteran differs from its fresh twin, first in {diff}"


def assert_params_to_rounding(label, veteran: dict, twin: dict, cfg: Config, lr: float):
    """The post-AdamW parameters that are NOT bitwise reproducible (float atomics in their gradients), veteran against twin after ONE step
    from identical state: the suite's single-step statement (test_full_size_train_step_is_reproducible) -- the typical element agrees to
    1e-6 and none moves further apart than the 2 lr an element whose gradient sits in AdamW's eps regime can (its step is lr g / (|g| + eps):
    the order of the atomics decides its sign).  Returns (largest median, largest maximum) over the tensors."""
    worst_med, worst_max = 0.0, 0.0
    for name, va in veteran.items():
        if not name.startswith("param/") or cfg.bitwise_tensor(name.split("/", 1)[1]):
            continue
        diff = (va.double() - twin[name].double()).abs().reshape(-1)
        med, mx = float(diff.median()), float(diff.max())
        assert med <= 1e-6, (label, name, "median |veteran - twin|", med)
        assert mx <= 2 * lr + 1e-5, (label, name, "max |veteran - twin|", mx)
        worst_med, worst_max = max(worst_med, med), max(worst_max, mx)
    return worst_med, worst_max


def oracle_front_end(cfg: Config, st: dict):
    if cfg.mode == "table":
        return O.FrontEnd(mode="table", bounds=synth.bounds(cfg.num))
    return O.FrontEnd(mode="adj", bounds=synth.bounds(cfg.num), feats=[f.cpu() for f in st["feats"]], inter=st["inter"].cpu())


def sd_numpy(st: dict):
    return {k: v.cpu().numpy() for k, v in st["sd"].items()}


def oracle_parity(label, cfg: Config, st: dict, batch, got: dict, *, alpha=1.0, beta=0.001, chrom=0, masks=None, backward=True,
                  dlogits=None):
    """A call against the fp32 oracle on the state ``st`` at the north-star tolerance: logits element-wise, the losses, every gradient
    (grad-None sets equal; the gauge direction excluded).  ``dlogits``: the call was the autograd route through sum(logits * dlogits)
    instead of the training loss.  Returns (worst relative error, the oracle's gradients)."""
    x, y, w = (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in batch)
    P = {k: v.cpu().clone().requires_grad_(backward and k not in G.FROZEN_NAMES) for k, v in st["sd"].items()}
    fe = oracle_front_end(cfg, st)
    xt, yt, wt = torch.from_numpy(x), torch.from_numpy(y.reshape(-1, 1)), torch.from_numpy(w.reshape(-1, 1))
    kw = dict(random_chrom=chrom)
    if masks:
        kw["masks"] = masks
    if not backward:
        with torch.no_grad():
            lg, _ = O.classifier_forward(P, fe, xt, **kw)
        e = logit_err(got["logits"].cpu().numpy(), lg.numpy())
        assert e < TOL, (label, "logits", e)
        return e, None
    if dlogits is not None:
        lg, _ = O.classifier_forward(P, fe, xt, **kw)
        names = [n for n, t in P.items() if t.requires_grad]
        gs = torch.autograd.grad((lg * dlogits.cpu().reshape(lg.shape)).sum(), [P[n] for n in names], allow_unused=True)
        grads, lg = dict(zip(names, gs)), lg.detach()
    else:
        _, bce, recon, lg, grads = O.loss_and_grads(P, fe, xt, yt, wt, alpha, beta, **kw)
    worst = logit_err(got["logits"].cpu().numpy(), lg.numpy())
    assert worst < TOL, (label, "logits", worst)
    if "losses" in got and dlogits is None:
        ls = got["losses"].cpu().numpy()
        rc = float(recon.reshape(-1)[0])
        assert abs(float(ls[0]) - float(bce)) <= TOL * max(1.0, abs(float(bce))), (label, "bce", float(ls[0]), float(bce))
        assert abs(float(ls[1]) - rc) <= TOL * max(1.0, abs(rc)), (label, "recon", float(ls[1]), rc)
    checked = 0
    for n, gref in grads.items():
        mine = got.get("grad/" + n)
        if gref is None:
            assert mine is None, (label, n, "the oracle's gradient is None, ours is not")
            continue
        assert mine is not None, (label, n, "gradient missing")
        if n == G.GAUGE:
            continue
        r = gref.numpy()
        e = float(np.abs(mine.cpu().numpy() - r).max()) / max(float(np.abs(r).max()), 1e-3)
        assert e <= TOL, (label, n, e)
        worst = max(worst, e)
        checked += 1
    assert checked >= 20, checked
    return worst, grads


def fp64_grade(label, cfg: Config, st: dict, batch, got: dict, *, alpha=1.0, beta=0.001, chrom=0):
    """A dropout-free training call held to fp32 grade (tests/fp64_grade.py: K = 8 on the fp32 oracle's own noise)."""
    x, y, w = (t.cpu().numpy() for t in batch)
    ref = G.references(sd_numpy(st), oracle_front_end(cfg, st), x, y, w, alpha=alpha, beta=beta, chrom=chrom)
    ls = got["losses"].cpu().numpy()
    grads = {n: None for n in ref.r64.grads}
    for k, v in got.items():
        if k.startswith("grad/"):
            grads[k[5:]] = None if v is None else v.cpu().double().numpy()
    step = G.StepOut(got["logits"].cpu().double().numpy(), {"bce": float(ls[0]), "recon": float(ls[1])}, grads)
    return G.assert_grade(label, G.grade(step, ref)), ref


def call_masks(cfg: Config, clf, seed: int, n_tokens: int):
    """The masks a training call with dropout seed ``seed`` draws (oracle/rng.py), for the model's current Dropout.p; None in eval
    mode or with every p at 0."""
    p_adj, p_fc1, p_pff = clf._dropout_p()
    if not clf.training or max(p_adj, p_fc1, p_pff) <= 0:
        return None
    return G.step_masks(seed, (p_adj, p_fc1, p_pff), n_tokens, cfg.d, cfg.num if cfg.mode == "adj" else None, wrap=torch.from_numpy)


def ran_kernels(log) -> set:
    return {k for k, n in log.counts.items() if n > 0}


def assert_kernels(label, ran, must=(), must_not=()):
    assert set(must) <= ran, (label, "kernels missing", sorted(set(must) - ran), "ran", sorted(ran))
    assert not (set(must_not) & ran), (label, "kernels unexpected", sorted(set(must_not) & ran))


def option(name):
    return _lib.option(name) if name else contextlib.nullcontext()
